// The one-launch step over the slide's full scores: pooling, loss, backward and the WHOLE Adam step in one kernel whose
// workgroups each repeat the slide's pooling (pool_phase, moc_step_shared.h) and own a part of W1.  Two splits of W1:
// narrow (pool_w1_step_kernel: by hidden unit, the pairs' rows in LDS) and wide (pool_w1_step_wide_kernel: by column,
// C <= 64).  Both can sum the gradient over a node's ranks inside the kernel (P2pArgs).  The one-launch step over the
// forward's tile records is moc_step_tiles.hip; which of them a shape gets: step_plan, moc_meta.hip.
#include "moc_step_shared.h"

namespace {

// ---- pooling + loss + backward + the WHOLE Adam step in one launch --------------------------------
// grid (H/4): every workgroup repeats the (cheap, latency-bound) pooling of the slide for itself --
// 16 workgroups doing it side by side cost no more time than one -- and then owns 4 hidden units of
// W1 (4 x D parameters): it forms their gradient from the <= C*K pairs it has just found and steps
// them.  No pair list goes through memory, no second launch, no dependent n_pair -> row -> load chain.
// Workgroup 0 also publishes the slide's outputs and steps b1, W2, b2; since every workgroup READS
// W2 (for dh) while workgroup 0 WRITES it, W2 is double buffered by the caller (W2 in, W2out out).
__global__ __launch_bounds__(1024) void pool_w1_step_kernel(FusedArgs g, float* pooled_out, int32_t* topk_idx_out,
                                                            int32_t* topk_cnt_out, int PS_CAP) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const FinishArgs& a = g.f;
    const int b = a.slide0, C = a.C, K = a.K, D = a.D;
    // HW hidden units of W1 per workgroup: 4 (16 workgroups: the in-kernel gradient exchange has 16 channels) or 2 (32
    // workgroups: half the Adam arithmetic per thread -- sixteen waves on one CU make that the kernel's last 2 us)
    const int HW = H / (int)gridDim.x, JN = HW >> 1;
    const int wg = blockIdx.x, h_lo = wg * HW;
    // (offsets from smem, which is 16-byte aligned, rounded in the layout -- not address arithmetic through integers: that
    // loses the LDS address space and every access through the pointer becomes a flat_ operation)
    const lds::NarrowStepLds Y = lds::narrow_step_lds(C, K, D, PS_CAP);
    const PoolLds L = pool_lds(smem, Y.pool);
    float* const dpool = L.dpool;
    int* const topk_s = L.topk_s;
    float* dz = reinterpret_cast<float*>(smem + Y.dz);
    float* H1s = reinterpret_cast<float*>(smem + Y.H1s);
    float* dhs = reinterpret_cast<float*>(smem + Y.dhs);
    float* W2s = reinterpret_cast<float*>(smem + Y.W2s);
    int64_t* row_s = reinterpret_cast<int64_t*>(smem + Y.row_s);
    float* xs = reinterpret_cast<float*>(smem + Y.xs);
    MOC_STAMP(10);
    // thread t: column d = t % D' of hidden units h_lo + JN*(t / D') + {0 .. JN-1}, D' = min(D, 512)
    const int t = threadIdx.x;
    const int dcols = D < 512 ? D : 512;                 // columns covered per sweep by 1024 threads (2 h each)
    const int hh = t / dcols, dl = t - hh * dcols;       // hh in {0, 1} when dcols == 512
    const bool own = hh < 2;                             // D < 512: the threads beyond 2*D idle in the W1 part
    const AdamCoef ak = step_coef(a);
    // The parameters and moments this workgroup steps are requested further down, just before the gradient loop that
    // hides them, and W2 with the pairs' gathers: at the top they sat in front of the slide's scores -- the first thing
    // the kernel waits for, and loads return in issue order -- and held 12 registers through the pooling.
    int64_t base;
    const int k = pool_phase(a, b, L, PS_CAP, wg == 0, pooled_out, topk_idx_out, topk_cnt_out, &base);
    __syncthreads();
    MOC_STAMP(15);
    // ---- pairs: TWO rounds of gathers.  Round 1 -- everything that needs only a pair's position among the selected
    // rows (its row id, its gate operands, its hidden row), W2 and the parameters this workgroup steps -- is requested in
    // one go, straight from topk_s; round 2 the bag rows, a wave per pair (two pairs in flight per wave).  Sixteen waves
    // share one CU here: an instruction every thread executes costs the workgroup 16 issue cycles, so each part runs on
    // the waves that have work for it and nowhere else, and nothing divides.
    const int P = C * k;
    float pw[2][2], pm[2][2], pv[2][2];                  // [h sub-index][d sweep]  (D <= 1024): consumed by the Adam update
    float pW = 0.f, pM = 0.f, pV = 0.f;                  // workgroup 0: W2 / b2 / b1 element of this thread
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int sw = 0; sw < 2; ++sw) pw[j][sw] = pm[j][sw] = pv[j][sw] = 0.f;
    if (P > 0) {                                         // (uniform)
        // pairs per class k <= 16, pair numbers < 256: p / k = (p * ceil(2^16 / k)) >> 16 exactly
        const unsigned kinv = (65536u + (unsigned)k - 1u) / (unsigned)k;
        auto topk_of = [&](int pp) { const int c = (int)(((unsigned)pp * kinv) >> 16); return topk_s[c * K + (pp - c * k)]; };
        int64_t rid = 0;
        if (t < P) rid = a.sel_row[base + topk_of(t)];
        float sc = 0.f, lam = 0.f;
        const int dp = t >> 2, di = t & 3, dc = (int)(((unsigned)dp * kinv) >> 16);     // P <= 256: one element of dz per thread
        if (t < P * 4) {
            const int dsidx = topk_s[dc * K + (dp - dc * k)];
            const int dcol = di == 0 ? dc : di == 1 ? C + dc : di == 2 ? 2 * C : 2 * C + 1;
            sc = a.cand[(int64_t)dcol * a.stride + base + dsidx];
            lam = a.gates[(base + dsidx) * 4 + di];
        }
        float w2r = 0.f;
        if (t < 4 * H) w2r = a.W2[t];
        // H1 of the pairs: workgroup 0 needs all H columns (b1, W2), the others their 4
        const int hsh = wg == 0 ? 6 : JN, hn = 1 << hsh, h0 = wg == 0 ? 0 : h_lo, nh = P << hsh;   // (HW = 4, 2 = 1 << JN)
        float hv0 = 0.f, hv1 = 0.f;
        if (t < nh) hv0 = a.H1[(base + topk_of(t >> hsh)) * H + h0 + (t & (hn - 1))];
        if (t + 1024 < nh) hv1 = a.H1[(base + topk_of((t + 1024) >> hsh)) * H + h0 + (t & (hn - 1))];
        if (a.apply_adam) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int sw = 0; sw < 2; ++sw) {
                    const int d = dl + sw * dcols;
                    if (own && d < D && j < JN) {
                        const int e = (h_lo + hh * JN + j) * D + d;
                        pw[j][sw] = g.W1[e]; pm[j][sw] = g.m_W1[e]; pv[j][sw] = g.v_W1[e];
                    }
                }
            if (wg == 0) {
                if (t < 4 * H) { pM = a.m_W2[t]; pV = a.v_W2[t]; }
                else if (t < 4 * H + 4) { pW = a.b2[t - 4 * H]; pM = a.m_b2[t - 4 * H]; pV = a.v_b2[t - 4 * H]; }
                else if (t >= 320 && t < 320 + H) { pW = a.b1[t - 320]; pM = a.m_b1[t - 320]; pV = a.v_b1[t - 320]; }
            }
        }
        if (t < P) row_s[t] = rid;
        if (t < P * 4) {
            const float dlam = (a.use_bits >> di & 1u) ? (dpool[dc] / (float)k) * sc : 0.f;
            dz[t] = dlam * lam * (1.f - lam);
        }
        if (t < 4 * H) {
            W2s[t] = w2r;
            if (wg == 0) pW = w2r;
        }
        if (t < nh) H1s[(t >> hsh) * H + h0 + (t & (hn - 1))] = hv0;
        if (t + 1024 < nh) H1s[((t + 1024) >> hsh) * H + h0 + (t & (hn - 1))] = hv1;
        for (int e = t + 2048; e < nh; e += 1024) {        // workgroup 0 with more than 32 pairs
            const int pp = e >> hsh, h = h0 + (e & (hn - 1));
            H1s[pp * H + h] = a.H1[(base + topk_of(pp)) * H + h];
        }
        __syncthreads();
        // bag rows of the pairs -> fp32 in LDS: wave w takes pairs w, w + 16 (both in flight), w + 32, ...; a lane the
        // 16-byte (16-bit storage: 8-byte) pieces lane, lane + 64, ... of the row -- D / 256 of them
        const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
        const int dq = D >> 8;                             // 1..4
        const int esz = a.xdt == MOC_F32 ? 4 : 2;
        for (int p0 = wave; p0 < P; p0 += 32) {
            const int p1 = p0 + 16;
            const bool two = p1 < P;
            const unsigned char* r0 = a.X + row_s[p0] * (int64_t)D * esz;
            const unsigned char* r1 = a.X + row_s[two ? p1 : p0] * (int64_t)D * esz;
            float* x0 = xs + (size_t)p0 * D + lane * 4;
            float* x1 = xs + (size_t)p1 * D + lane * 4;
            if (a.xdt == MOC_F32) {
                // (named pieces: hipcc keeps an array written under a condition in scratch)
                float4 a0 = {}, a1 = {}, a2 = {}, a3 = {}, b0 = {}, b1v = {}, b2v = {}, b3 = {};
                const float4* q0 = reinterpret_cast<const float4*>(r0) + lane;
                const float4* q1 = reinterpret_cast<const float4*>(r1) + lane;
                a0 = q0[0]; b0 = q1[0];
                if (dq > 1) { a1 = q0[64]; b1v = q1[64]; }
                if (dq > 2) { a2 = q0[128]; b2v = q1[128]; }
                if (dq > 3) { a3 = q0[192]; b3 = q1[192]; }
                float4* y0 = reinterpret_cast<float4*>(x0);
                float4* y1 = reinterpret_cast<float4*>(x1);
                y0[0] = a0;
                if (dq > 1) y0[64] = a1;
                if (dq > 2) y0[128] = a2;
                if (dq > 3) y0[192] = a3;
                if (two) {
                    y1[0] = b0;
                    if (dq > 1) y1[64] = b1v;
                    if (dq > 2) y1[128] = b2v;
                    if (dq > 3) y1[192] = b3;
                }
            } else {
                const bool f16 = a.xdt == MOC_F16;
                auto widen = [&](uint2 raw) {
                    float4 o;
                    if (f16) {
                        o.x = moc_f16_to_f32((uint16_t)raw.x); o.y = moc_f16_to_f32((uint16_t)(raw.x >> 16));
                        o.z = moc_f16_to_f32((uint16_t)raw.y); o.w = moc_f16_to_f32((uint16_t)(raw.y >> 16));
                    } else {
                        o.x = __uint_as_float(raw.x << 16); o.y = __uint_as_float(raw.x & 0xFFFF0000u);
                        o.z = __uint_as_float(raw.y << 16); o.w = __uint_as_float(raw.y & 0xFFFF0000u);
                    }
                    return o;
                };
                uint2 u0[4], u1[4];
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < dq) {
                        u0[i] = *reinterpret_cast<const uint2*>(r0 + (lane + i * 64) * 8);
                        u1[i] = *reinterpret_cast<const uint2*>(r1 + (lane + i * 64) * 8);
                    }
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < dq) {
                        *reinterpret_cast<float4*>(x0 + i * 256) = widen(u0[i]);
                        if (two) *reinterpret_cast<float4*>(x1 + i * 256) = widen(u1[i]);
                    }
            }
        }
    }
    __syncthreads();
    MOC_STAMP(16);
    {   // dh[p][h] = (sum_i dz[p][i] * W2[i][h]) * [H1 > 0]  for this workgroup's columns
        const int hn = wg == 0 ? H : HW, h0 = wg == 0 ? 0 : h_lo;
        for (int e = t; e < P * hn; e += 1024) {
            const int p = e / hn, h = h0 + (e - p * hn);
            float v = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) v = fmaf(dz[p * 4 + i], W2s[i * H + h], v);
            dhs[p * H + h] = H1s[p * H + h] > 0.f ? v : 0.f;
        }
    }
    __syncthreads();
    MOC_STAMP(17);
    // ---- gradients of the owned elements: JN x 2 of W1 per thread, one of b1 / W2 / b2 in workgroup 0
    const int ha = h_lo + hh * JN;
    float gr[2][2] = {{0.f, 0.f}, {0.f, 0.f}};           // [d sweep][h sub-index]
    if (own) {
#pragma unroll
        for (int sw = 0; sw < 2; ++sw) {
            const int d = dl + sw * dcols;
            if (d < D) {
                float g0 = 0.f, g1 = 0.f;
                for (int p = 0; p < P; ++p) {
                    const float xv = xs[(size_t)p * D + d];
                    g0 = fmaf(dhs[p * H + ha], xv, g0);
                    if (JN > 1) g1 = fmaf(dhs[p * H + ha + 1], xv, g1);
                }
                gr[sw][0] = g0; gr[sw][1] = g1;
            }
        }
    }
    // tail element: flat order W1 | b1 | W2 | b2 (the order of the exchange slots)
    float gt = 0.f;
    int tail = -1;
    if (wg == 0) {
        if (t < 4 * H) {
            const int i = t >> 6, h = t & 63;
            for (int p = 0; p < P; ++p) gt = fmaf(dz[p * 4 + i], H1s[p * H + h], gt);
            tail = H + t;
        } else if (t < 4 * H + 4) {
            const int i = t - 4 * H;
            for (int p = 0; p < P; ++p) gt += dz[p * 4 + i];
            tail = H + 4 * H + i;
        } else if (t >= 320 && t < 320 + H) {
            const int h = t - 320;
            for (int p = 0; p < P; ++p) gt += dhs[p * H + h];
            tail = h;
        }
    }
    if (!a.apply_adam) {                                  // gradient out (data-parallel step with a collective)
        if (own)
            for (int sw = 0; sw < 2; ++sw) {
                const int d = dl + sw * dcols;
                if (d < D) { g.g_W1[(ha + 0) * D + d] = gr[sw][0]; if (JN > 1) g.g_W1[(ha + 1) * D + d] = gr[sw][1]; }
            }
        if (tail >= H + 4 * H) a.g_b2[tail - 5 * H] = gt;
        else if (tail >= H) a.g_W2[tail - H] = gt;
        else if (tail >= 0) a.g_b1[tail] = gt;
        return;
    }
    if (g.x.world > 1) {                                  // one-shot exchange over xGMI (moc_p2p.h)
        __shared__ int p2p_ok;
        const int64_t nW1 = (int64_t)H * D;
        if (own)
#pragma unroll
            for (int sw = 0; sw < 2; ++sw) {
                const int d = dl + sw * dcols;
                if (d < D) { p2p_push(g.x, (int64_t)(ha + 0) * D + d, gr[sw][0]); if (JN > 1) p2p_push(g.x, (int64_t)(ha + 1) * D + d, gr[sw][1]); }
            }
        if (tail >= 0) p2p_push(g.x, nW1 + tail, gt);
        if (!p2p_signal_wait(g.x, wg, &p2p_ok)) return;   // time-out: reported through g.x.error, no update
        if (own)
#pragma unroll
            for (int sw = 0; sw < 2; ++sw) {
                const int d = dl + sw * dcols;
                if (d < D) {
                    gr[sw][0] = p2p_sum(g.x, (int64_t)(ha + 0) * D + d, gr[sw][0]);
                    if (JN > 1) gr[sw][1] = p2p_sum(g.x, (int64_t)(ha + 1) * D + d, gr[sw][1]);
                }
            }
        if (tail >= 0) gt = p2p_sum(g.x, nW1 + tail, gt);
    }
    // ---- Adam: parameter, moments, operand image
    const float gs = ak.grad_scale;
    if (own) {
#pragma unroll
        for (int sw = 0; sw < 2; ++sw) {
            const int d = dl + sw * dcols;
            if (d < D) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if (j >= JN) continue;
                    const int e = (ha + j) * D + d;
                    adam_update(pw[j][sw], pm[j][sw], pv[j][sw], gr[sw][j] * gs, ak);
                    g.W1[e] = pw[j][sw]; g.m_W1[e] = pm[j][sw]; g.v_W1[e] = pv[j][sw];
                    w1_image_store(g.img_dt, g.W1img, D, ha + j, d, pw[j][sw]);
                }
            }
        }
    }
    if (tail >= 0) {                                      // workgroup 0: b1, W2 (into the other buffer), b2
        adam_update(pW, pM, pV, gt * gs, ak);
        if (tail >= H + 4 * H) { const int i = tail - 5 * H; a.b2[i] = pW; a.m_b2[i] = pM; a.v_b2[i] = pV; }
        else if (tail >= H) { const int i = tail - H; g.W2out[i] = pW; a.m_W2[i] = pM; a.v_W2[i] = pV; }
        else { a.b1[tail] = pW; a.m_b1[tail] = pM; a.v_b1[tail] = pV; }
    }
    MOC_STAMP(18);
}

// ------------------------------------------------------------------ one-launch step, wide shapes
// C <= 64, K <= 16, S <= 8192 (EBRAINS-30, the 64-way stress shape): hundreds of gradient pairs, whose bag
// rows (P x D) and hidden activations (P x 64) do not fit in LDS.  Same grid as pool_w1_step_kernel (16
// workgroups of 1024 threads, every one repeats the pooling), different split of the backward pass:
// workgroup g owns the D/16 COLUMNS [g*D/16, ...) of W1 for all 64 hidden units, so it needs only a
// D/16-wide piece of every pair's row (64 B at D = 512 bf16: one gather round, P x 64 B of LDS), and
// instead of dh[P][64] it keeps per pair the four gate derivatives dz[p][0..3] and the 64-bit ReLU mask of
// its hidden row: dh[p][h] = mask_p[h] ? sum_i dz[p][i] W2[i][h] : 0 is re-formed on the fly.  The small
// tensors are split by hidden unit: workgroup g also owns W2[:, 4g..4g+3] and b1[4g..4g+3] (16 wave-wide
// reductions over the pairs), workgroup 0 b2.

__global__ __launch_bounds__(1024) void pool_w1_step_wide_kernel(FusedArgs g, float* pooled_out, int32_t* topk_idx_out,
                                                                 int32_t* topk_cnt_out, int PS_CAP, int region_bytes,
                                                                 int external_pool, int WD_PCH) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const FinishArgs& a = g.f;
    const int b = a.slide0, C = a.C, K = a.K, D = a.D;
    const int wg = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int DS = D / 16, d_lo = wg * DS;               // this workgroup's columns of W1
    moc_kernarg_touch<sizeof(FusedArgs)>();
    MOC_STAMP(40);
    const int esz = a.xdt == MOC_F32 ? 4 : 2;
    // ---- LDS carve
    const lds::WideStepLds Y = lds::wide_step_lds_behind(C, K, region_bytes);   // (the host's wide_step_lds: region_bytes is p.wide_region)
    unsigned char* region = smem + Y.region;
    const PoolLds L = pool_lds(smem, Y.pool);
    float* const pooled_s = L.pooled_s;
    float* const dpool = L.dpool;
    int* const topk_s = L.topk_s;
    float* dz = reinterpret_cast<float*>(smem + Y.dz);
    float* h1o = reinterpret_cast<float*>(smem + Y.h1o);
    const int PM = Y.PM;
    unsigned* mask = reinterpret_cast<unsigned*>(smem + Y.mask);
    int* sidx_s = reinterpret_cast<int*>(smem + Y.sidx_s);
    float* W2s = reinterpret_cast<float*>(smem + Y.W2s);
    float* red = reinterpret_cast<float*>(smem + Y.red);
    int64_t* prow_s = reinterpret_cast<int64_t*>(smem + Y.prow_s);

    // ---- operands that do not depend on this slide: requested first, consumed last.
    // The W1 gradient of this workgroup is a [64 x DS] tile product on the fp32 matrix cores: wave w < 4*DS/16
    // owns the 16 x 16 tile (hidden units 16 (w / NTN) .., columns d_lo + 16 (w % NTN) ..); lane l ends with
    // elements (h0 + (l >> 4) * 4 + i, d0 + (l & 15)), i < 4.
    const int NTN = DS / 16;                              // n-tiles (2 or 4)
    const bool has_tile = wave < 4 * NTN;
    // D = 512: eight tiles, sixteen waves -- waves 8..15 take the SECOND HALF of every chunk's pairs for the same tiles
    // (twave) and the halves meet in LDS behind the chunk loop (first + second: one fixed association); the chunk's MFMA
    // phase was 6.1 of the step's 26 us with half of the waves idle
    const bool ksplit = 4 * NTN <= 8;
    const int twave = ksplit ? (wave & 7) : wave;
    const bool in_product = ksplit || has_tile;
    const int h0 = (twave / NTN) * 16, d0 = d_lo + (twave % NTN) * 16;
    float pw[4], pm[4], pv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        pw[i] = pm[i] = pv[i] = 0.f;
        if (has_tile && a.apply_adam) {
            const int e = (h0 + (lane >> 4) * 4 + i) * D + d0 + (lane & 15);
            pw[i] = g.W1[e]; pm[i] = g.m_W1[e]; pv[i] = g.v_W1[e];
        }
    }
    const AdamCoef ak = step_coef(a);
    // (W2 through a register: stored to LDS below, once the pooling's own first loads are under way -- a store here would
    // wait for everything requested above before the slide's data is even asked for)
    const float w2r = t < 4 * H ? a.W2[t] : 0.f;
    // small tensors: threads 0..15 -> W2[i][4 wg + jj] (i = t >> 2, jj = t & 3); 16..19 -> b1[4 wg + jj]; 20..23 -> b2 (wg 0)
    float pS = 0.f, pSm = 0.f, pSv = 0.f;
    int small = -1;                                       // flat tail index (b1 | W2 | b2), as in the narrow kernel
    if (t < 16) small = H + (t >> 2) * H + wg * 4 + (t & 3);
    else if (t < 20) small = wg * 4 + (t - 16);
    else if (t < 24 && wg == 0) small = H + 4 * H + (t - 20);
    if (small >= 0 && a.apply_adam) {
        if (small >= 5 * H) { pS = a.b2[small - 5 * H]; pSm = a.m_b2[small - 5 * H]; pSv = a.v_b2[small - 5 * H]; }
        else if (small >= H) { pS = a.W2[small - H]; pSm = a.m_W2[small - H]; pSv = a.v_W2[small - H]; }
        else { pS = a.b1[small]; pSm = a.m_b1[small]; pSv = a.v_b1[small]; }
    }
    int64_t base;
    int k, P;
    unsigned kinv;
    float4 hv_pre[5];
    // the pairs' hidden rows: requested as soon as the pooled rows' indices are in LDS, their ReLU bits ORed into the masks
    // further down
    auto request_hidden = [&]() {
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const int e = t + q * 1024;
            hv_pre[q] = float4{0.f, 0.f, 0.f, 0.f};
            if (e < P * 16) {
                const int p = e >> 4, c = (int)(((unsigned)p * kinv) >> 16);
                hv_pre[q] = *reinterpret_cast<const float4*>(a.H1 + (base + topk_s[c * K + (p - c * k)]) * H + (e & 15) * 4);
            }
        }
    };
    auto zero_masks = [&]() {
        for (int p = t; p < 2 * P; p += 1024) mask[(p >= P ? PM - P : 0) + p] = 0u;
        if (t < 64) dz[P * 4 + t] = 0.f;                   // the slack rows: pairs P .. P + 15 contribute nothing
    };
    if (external_pool) {
        // more than 8192 selected rows possible: the top-K came from topk_mean_kernel (one workgroup per class); pick it up,
        // add loss / argmax / d loss.  Thread e < C K owns the pooled row (class e / K, place e % K): its operands -- row id,
        // four candidate scores, gates -- are requested from the REGISTER that holds its index, before the index has even
        // been to LDS, and are under way while wave 0 does the cross entropy; the hidden rows (which need other threads'
        // indices) follow behind the first barrier.  (Before: indices -> LDS -> barrier -> cross entropy -> barrier -> the
        // operands' round trip -> barrier: 5.4 of the step's 15.7 us by the stamps.)
        base = a.base_host >= 0 ? a.base_host : a.row_off[b];
        const int y = (int)a.labels[b];
        const int PK = C * K;
        const int own_idx = a.topk_idx[(int64_t)b * PK + (t < PK ? t : PK - 1)];
        k = a.topk_cnt[(int64_t)b * C];
        const float pooled_v = a.pooled[(int64_t)b * C + (t < C ? t : 0)];
        P = C * k;
        // pairs per class k <= 16, pair numbers < 1024: p / k = (p * ceil(2^16 / k)) >> 16 exactly (no integer division)
        kinv = k > 0 ? (65536u + (unsigned)k - 1u) / (unsigned)k : 0u;
        const unsigned kinvK = (65536u + (unsigned)K - 1u) / (unsigned)K;
        const int own_c = (int)(((unsigned)t * kinvK) >> 16), own_pos = t - own_c * K;
        const bool own = t < PK && own_pos < k;
        int64_t own_row = 0;
        float sc[4] = {0.f, 0.f, 0.f, 0.f};
        float4 lam = {0.f, 0.f, 0.f, 0.f};
        if (own) {
            own_row = a.sel_row[base + own_idx];
            const float* cd = a.cand + base + own_idx;
            sc[0] = cd[(int64_t)own_c * a.stride]; sc[1] = cd[(int64_t)(C + own_c) * a.stride];
            sc[2] = cd[(int64_t)(2 * C) * a.stride]; sc[3] = cd[(int64_t)(2 * C + 1) * a.stride];
            lam = *reinterpret_cast<const float4*>(a.gates + (base + own_idx) * 4);
        }
        if (t < PK) topk_s[t] = own_idx;
        if (t < C) pooled_s[t] = pooled_v;
        if (t < 4 * H) W2s[t] = w2r;
        zero_masks();
        __syncthreads();
        request_hidden();
        ce_wave0<32>(a, b, C, y, pooled_s, dpool, wg == 0);
        __syncthreads();
        MOC_STAMP(41);
        if (own) {
            const int pr = own_c * k + own_pos;
            sidx_s[pr] = own_idx;
            prow_s[pr] = own_row;
            const float lv[4] = {lam.x, lam.y, lam.z, lam.w};
            const float gk = dpool[own_c] / (float)k;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                dz[pr * 4 + i] = (a.use_bits >> i & 1u) ? gk * sc[i] * lv[i] * (1.f - lv[i]) : 0.f;
        }
    } else {
        k = pool_phase<8, 32, 2>(a, b, L, PS_CAP, wg == 0, pooled_out, topk_idx_out, topk_cnt_out, &base);
        if (t < 4 * H) W2s[t] = w2r;
        __syncthreads();
        MOC_STAMP(41);
        // ---- pairs
        P = C * k;
        kinv = k > 0 ? (65536u + (unsigned)k - 1u) / (unsigned)k : 0u;
        zero_masks();
        request_hidden();
        for (int p = t; p < P; p += 1024) {
            const int c = (int)(((unsigned)p * kinv) >> 16), sidx = topk_s[c * K + (p - c * k)];
            sidx_s[p] = sidx;
            prow_s[p] = a.sel_row[base + sidx];
            const float* cd = a.cand + base + sidx;
            const float sc[4] = {cd[(int64_t)c * a.stride], cd[(int64_t)(C + c) * a.stride],
                                 cd[(int64_t)(2 * C) * a.stride], cd[(int64_t)(2 * C + 1) * a.stride]};
            const float4 lam = *reinterpret_cast<const float4*>(a.gates + (base + sidx) * 4);
            const float lv[4] = {lam.x, lam.y, lam.z, lam.w};
            const float gk = dpool[c] / (float)k;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                dz[p * 4 + i] = (a.use_bits >> i & 1u) ? gk * sc[i] * lv[i] * (1.f - lv[i]) : 0.f;
        }
    }
    __syncthreads();
    MOC_STAMP(42);
    // the first row pieces of the W1 gradient are requested below, right behind the hidden rows' ReLU bits (whose registers
    // they take over: both at once spill) and in front of the barrier and the small gradients: they land in LDS in the chunk loop
    const int DSb = DS * esz;                              // bytes of a pair's piece
    const int ppr = DSb / 16;                              // 16-B pieces per pair: 4, 8 or 16 -- shifts, no division
    const int ppr_sh = ppr == 4 ? 2 : ppr == 8 ? 3 : ppr == 16 ? 4 : ppr == 2 ? 1 : 0;
    // (one piece per call, returned by value, the four of a batch in named variables: an array filled under a branch, or
    // handed to a lambda by reference, goes to scratch memory)
    auto request_piece = [&](int c0, int n, int e) -> uint4 {
        const int ec = e < n * ppr ? e : n * ppr - 1;
        const int pp = ec >> ppr_sh, v = ec - (pp << ppr_sh);
        return *reinterpret_cast<const uint4*>(a.X + (prow_s[c0 + pp] * D + d_lo) * esz + v * 16);
    };
    // hidden rows of the pairs: ReLU mask (64 bits) and the four values this workgroup owns
    auto take_hidden = [&](int e, const float4& hv) {
        const int p = e >> 4, v = e & 15;
        const unsigned bits = (hv.x > 0.f ? 1u : 0u) | (hv.y > 0.f ? 2u : 0u) | (hv.z > 0.f ? 4u : 0u) | (hv.w > 0.f ? 8u : 0u);
        if (bits) atomicOr(&mask[(v >> 3) * PM + p], bits << ((v & 7) * 4));
        if (v == wg) *reinterpret_cast<float4*>(h1o + p * 4) = hv;
    };
#pragma unroll
    for (int q = 0; q < 5; ++q)
        if (t + q * 1024 < P * 16) take_hidden(t + q * 1024, hv_pre[q]);
    for (int e = t + 5 * 1024; e < P * 16; e += 1024)           // more than 320 pairs
        take_hidden(e, *reinterpret_cast<const float4*>(a.H1 + (base + sidx_s[e >> 4]) * H + (e & 15) * 4));
    const int n_first = P < WD_PCH ? P : WD_PCH;
    uint4 pre0 = {}, pre1 = {}, pre2 = {}, pre3 = {};
    if (P > 0) {
        pre0 = request_piece(0, n_first, t); pre1 = request_piece(0, n_first, t + 1024);
        pre2 = request_piece(0, n_first, t + 2048); pre3 = request_piece(0, n_first, t + 3072);
    }
    __syncthreads();                                       // masks complete
    MOC_STAMP(43);
    // ---- small gradients: 16 + 4 (+ 4) sums over the pairs, one or two per wave, pairs strided over the lanes.  They run
    // inside the W1 gradient's first gather round trip (called below between the requests for the first row pieces and
    // their stores) and need no barrier of their own (dz, h1o and W2s are complete; `red` is read behind the product's
    // barriers) -- instead of two barriers and 1.4 us behind the product.
    auto small_gradients = [&]() {
        float part = 0.f;
        {   // wave w: W2[i][4 wg + jj] with (i, jj) = (w >> 2, w & 3)
            const int i = wave >> 2, jj = wave & 3;
            for (int p = lane; p < P; p += 64) part = fmaf(dz[p * 4 + i], h1o[p * 4 + jj], part);
            for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
            if (lane == 0) red[wave] = part;
        }
        part = 0.f;
        if (wave >= 8 && wave < 12) {                      // b1[4 wg + (wave - 8)] = sum_p dh[p][h]
            const int hj = wave - 8, hq = wg * 4 + hj;
            for (int p = lane; p < P; p += 64) {
                const float4 z = *reinterpret_cast<const float4*>(dz + p * 4);
                const float dh = fmaf(z.w, W2s[3 * H + hq], fmaf(z.z, W2s[2 * H + hq], fmaf(z.y, W2s[H + hq], z.x * W2s[hq])));
                part += h1o[p * 4 + hj] > 0.f ? dh : 0.f;
            }
            for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
            if (lane == 0) red[16 + hj] = part;
        } else if (wave >= 12) {                           // b2[i] = sum_p dz[p][i]
            const int i = wave - 12;
            for (int p = lane; p < P; p += 64) part += dz[p * 4 + i];
            for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
            if (lane == 0) red[20 + i] = part;
        }
    };
    // ---- W1 gradient: dW1[h][d] = sum_p dh[p][h] x[p][d], pairs in chunks of WD_PCH through `region`:
    // [PCH][DS] pieces of the pairs' rows as stored, then v_mfma_f32_16x16x4_f32 over p.  dh is never staged: per group of
    // sixteen pairs a tile wave forms dh[16 pairs][its 16 hidden units] = dz[16][4] W2[4][16] with ONE matrix instruction
    // (k = the four gates), whose result registers are, lane for lane, the A operands of the group's four gradient
    // instructions -- lane (li, kq) ends with dh[pair 4 kq + i][h0 + li] in register i, which is A[m = li][k = kq] of the
    // instruction that takes the pairs {i, 4 + i, 8 + i, 12 + i} of the group as its k.  The ReLU mask is one AND per
    // element (a sign-extended bit of the pair's mask word).  What this replaced: every workgroup writing all P x 64
    // values of dh to LDS first (19 rounds x ~25 instructions x 16 waves on one CU: 7.0 of the step's 25 us by the stamps,
    // instruction issue, not latency) and reading them back as A fragments.  (Forming dh in the loop with the VALU -- the
    // old fmaf chain per element -- was measured first: 18 us, sixteen waves x 18 vector instructions per MFMA.)
    f32x4_t gacc = {0.f, 0.f, 0.f, 0.f};
    if (P == 0) small_gradients();                         // (no pair at all: the sums are zeros, but they are written)
    {
        unsigned char* xraw = region;                                              // [PCH][DS * esz]
        for (int c0 = 0; c0 < P; c0 += WD_PCH) {
            const int n = P - c0 < WD_PCH ? P - c0 : WD_PCH;
            const int n16 = (n + 15) & ~15;                // (<= WD_PCH: a multiple of 32)
            if (c0 > 0) __syncthreads();                   // previous chunk consumed
            // (up to four pieces per thread requested before the first is stored: one round trip for a whole chunk of
            // up to 4096 pieces; the first batch of the first chunk was requested above and the small gradients run in front
            // of its stores.  Requesting EVERY chunk's pieces a chunk ahead needs registers this 1024-thread kernel does not
            // have: at its 128-register cap hipcc waits for them at once and parks them in scratch -- measured 3 % slower)
            unsigned char* xr = region;
            auto store_batch = [&](int e0, uint4 q0, uint4 q1, uint4 q2, uint4 q3) {
                const int e = e0 + t;
                if (e < n * ppr) *reinterpret_cast<uint4*>(xr + (size_t)e * 16) = q0;
                if (e + 1024 < n * ppr) *reinterpret_cast<uint4*>(xr + (size_t)(e + 1024) * 16) = q1;
                if (e + 2048 < n * ppr) *reinterpret_cast<uint4*>(xr + (size_t)(e + 2048) * 16) = q2;
                if (e + 3072 < n * ppr) *reinterpret_cast<uint4*>(xr + (size_t)(e + 3072) * 16) = q3;
            };
            int e0 = 0;
            if (c0 == 0) {                                 // the batch requested above
                small_gradients();
                store_batch(0, pre0, pre1, pre2, pre3);
                e0 = 4096;
            }
            for (; e0 < n * ppr; e0 += 4096) {
                const uint4 q0 = request_piece(c0, n, e0 + t), q1 = request_piece(c0, n, e0 + t + 1024);
                const uint4 q2 = request_piece(c0, n, e0 + t + 2048), q3 = request_piece(c0, n, e0 + t + 3072);
                store_batch(e0, q0, q1, q2, q3);
            }
            // the rows behind the last pair of a group of sixteen: zero (their dh is zero, but 0 x whatever bytes lie here is not)
            for (int e = n * ppr + t; e < n16 * ppr; e += 1024) *reinterpret_cast<uint4*>(xraw + (size_t)e * 16) = uint4{0u, 0u, 0u, 0u};
            if (c0 == 0) MOC_STAMP(50);
            __syncthreads();
            if (c0 == 0) MOC_STAMP(52);
            if (in_product) {
                const int kq = lane >> 4, li = lane & 15, cc = (d0 - d_lo) + li;
                const int hh = h0 + li;                                 // this lane's hidden unit
                const float w2b = W2s[kq * H + hh];                     // B of the dh product: [gate kq][hidden unit]
                const unsigned msh = (unsigned)(hh & 31);
                // this wave's share of the chunk's groups: all of them, or (ksplit) the first / second half
                const int half = (((n16 >> 4) + 1) >> 1) << 4;
                const int kb = (ksplit && wave >= 8) ? half : 0, ke = (ksplit && wave < 8) ? half : n16;
                const float* dzp = dz + (size_t)(c0 + li) * 4 + kq;                           // A of the dh product: [pair li][gate kq]
                const uint4* mkp = reinterpret_cast<const uint4*>(mask + (size_t)(hh >> 5) * PM + c0 + 4 * kq);   // words of the lane's four pairs
                auto product = [&](auto kind) {
                    constexpr int XK = decltype(kind)::value;           // 0 fp32, 1 bf16, 2 fp16
                    typedef typename std::conditional<XK == 0, float, uint16_t>::type xs_t;
                    const xs_t* xp = reinterpret_cast<const xs_t*>(xraw) + (size_t)(4 * kq) * DS + cc;   // row ks + 4 kq + i: + (ks + i) * DS
                    auto xcv = [&](xs_t v) -> float {
                        if constexpr (XK == 0) return v;
                        else if constexpr (XK == 2) return moc_f16_to_f32(v);
                        else return moc_bf16_to_f32(v);
                    };
                    const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
                    // (no unroll pragma: the optimizer cannot honour one on this loop -- it warned three times per build and
                    // gave the same code)
                    for (int ks = kb; ks < ke; ks += 16) {
                        const float za = dzp[ks * 4];
                        const uint4 m = mkp[ks >> 2];
                        const xs_t x0 = xp[(size_t)(ks + 0) * DS], x1 = xp[(size_t)(ks + 1) * DS], x2 = xp[(size_t)(ks + 2) * DS],
                                   x3 = xp[(size_t)(ks + 3) * DS];
                        const f32x4_t dh = __builtin_amdgcn_mfma_f32_16x16x4f32(za, w2b, zero4, 0, 0, 0);
                        const unsigned mk[4] = {m.x, m.y, m.z, m.w};
                        const float xv[4] = {xcv(x0), xcv(x1), xcv(x2), xcv(x3)};
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const unsigned on = (unsigned)__builtin_amdgcn_sbfe((int)mk[i], msh, 1u);      // 0 or all ones
                            gacc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(__float_as_uint(dh[i]) & on), xv[i], gacc, 0, 0, 0);
                        }
                    }
                };
                if (a.xdt == MOC_F32) product(std::integral_constant<int, 0>{});
                else if (a.xdt == MOC_F16) product(std::integral_constant<int, 2>{});
                else product(std::integral_constant<int, 1>{});
            }
            if (c0 == 0) MOC_STAMP(53);
        }
    }
    __syncthreads();
    if (ksplit) {                                          // second halves -> LDS (the chunk buffers are free), first halves add them
        float* part = reinterpret_cast<float*>(smem + Y.part);   // [8 tiles][4][64]
        if (wave >= 8) {
#pragma unroll
            for (int i = 0; i < 4; ++i) part[(twave * 4 + i) * 64 + lane] = gacc[i];
        }
        __syncthreads();
        if (wave < 8) {
#pragma unroll
            for (int i = 0; i < 4; ++i) gacc[i] = moc_fadd(gacc[i], part[(twave * 4 + i) * 64 + lane]);
        }
    }
    MOC_STAMP(44);
    MOC_STAMP(45);
    // ---- outputs
    const float gs = ak.grad_scale;
    float gv = 0.f;
    if (small >= 0) gv = t < 16 ? red[(t >> 2) * 4 + (t & 3)] : t < 20 ? red[16 + (t - 16)] : red[20 + (t - 20)];
    if (!a.apply_adam) {                                   // gradients out (data-parallel step with a collective)
        if (has_tile)
            for (int i = 0; i < 4; ++i) g.g_W1[(h0 + (lane >> 4) * 4 + i) * D + d0 + (lane & 15)] = gacc[i];
        if (small >= 5 * H) a.g_b2[small - 5 * H] = gv;
        else if (small >= H) a.g_W2[small - H] = gv;
        else if (small >= 0) a.g_b1[small] = gv;
        return;
    }
    if (g.x.world > 1) {                                   // one-shot exchange over xGMI (moc_p2p.h), as in the narrow kernel
        __shared__ int p2p_ok;
        const int64_t nW1 = (int64_t)H * D;
        if (has_tile)
#pragma unroll
            for (int i = 0; i < 4; ++i) p2p_push(g.x, (int64_t)(h0 + (lane >> 4) * 4 + i) * D + d0 + (lane & 15), gacc[i]);
        if (small >= 0) p2p_push(g.x, nW1 + small, gv);
        if (!p2p_signal_wait(g.x, wg, &p2p_ok)) return;   // time-out: reported through g.x.error, no update
        if (has_tile)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                gacc[i] = p2p_sum(g.x, (int64_t)(h0 + (lane >> 4) * 4 + i) * D + d0 + (lane & 15), gacc[i]);
        if (small >= 0) gv = p2p_sum(g.x, nW1 + small, gv);
    }
    if (has_tile) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int h = h0 + (lane >> 4) * 4 + i, d = d0 + (lane & 15), e = h * D + d;
            adam_update(pw[i], pm[i], pv[i], gacc[i] * gs, ak);
            g.W1[e] = pw[i]; g.m_W1[e] = pm[i]; g.v_W1[e] = pv[i];
            w1_image_store(g.img_dt, g.W1img, D, h, d, pw[i]);
        }
    }
    if (small >= 0) {
        adam_update(pS, pSm, pSv, gv * gs, ak);
        if (small >= 5 * H) { const int i = small - 5 * H; a.b2[i] = pS; a.m_b2[i] = pSm; a.v_b2[i] = pSv; }
        else if (small >= H) { const int i = small - H; g.W2out[i] = pS; a.m_W2[i] = pSm; a.v_W2[i] = pSv; }
        else { a.b1[small] = pS; a.m_b1[small] = pSm; a.v_b1[small] = pSv; }
    }
    MOC_STAMP(46);
}

}  // namespace

void moc_meta_internal::fused_step_attrs(raise_lds_fn raise) {
    raise("pool_w1_step_kernel", (const void*)pool_w1_step_kernel, lds::NARROW_MAX_LDS);
    raise("pool_w1_step_wide_kernel", (const void*)pool_w1_step_wide_kernel, lds::WIDE_MAX_LDS);
}

int moc_meta_internal::launch_fused_kernel(const StepPlan& p, const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws,
                                           const int64_t* labels, int slide, uint32_t use_bits, const AdamCoef& k, float* W2out,
                                           hipStream_t s, int apply_adam, const P2pArgs* x, const StepTab* tab) {
    FusedArgs g = {};
    if (x) g.x = *x;
    g.f = finish_args(B, M, ws, labels, slide, 1, apply_adam, use_bits, k);
    FinishArgs& a = g.f;
    finish_rows(a, B, ws, slide, true);
    if (tab) { a.adam_tab = tab->tab; a.adam_ctr = tab->ctr; a.adam_pos = tab->pos; }
    g.g_W1 = M->g_W1; g.W1 = M->W1; g.m_W1 = M->m_W1; g.v_W1 = M->v_W1; g.W1img = (unsigned char*)M->W1_image;
    g.W2out = W2out; g.img_dt = B->dtype;
    if (p.kind == STEP_WIDE) {
        if (p.external) {                                  // pooling by topk_mean_kernel first
            if (int rc = launch_pool(B, ws, slide, 1, s)) return rc;
            a.topk_idx = ws->topk_idx; a.topk_cnt = ws->topk_cnt;
        }
        MOC_REQUIRE(p.smem == (size_t)wide_lds(B, p.pch).bytes && p.wide_region == wide_lds(B, p.pch).region_bytes && p.smem <= (size_t)lds::WIDE_MAX_LDS,
                    "pool_w1_step_wide_kernel: C = %d, topk = %d, D = %d, pch = %d need %zu B of LDS (> %d)", B->C, B->topk, B->D, p.pch,
                    p.smem, lds::WIDE_MAX_LDS);
        pool_w1_step_wide_kernel<<<H / 4, 1024, p.smem, s>>>(g, ws->pooled, ws->topk_idx, ws->topk_cnt, p.wide_cap, p.wide_region,
                                                             p.external, p.pch);
        MOC_CHECK_LAUNCH("moc_fused_step(wide)");
        return MOC_OK;
    }
    MOC_REQUIRE(p.smem == (size_t)lds::narrow_step_lds(B->C, B->topk, B->D, p.cap).bytes && p.smem <= (size_t)lds::NARROW_MAX_LDS,
                "pool_w1_step_kernel: C = %d, topk = %d, D = %d, cap = %d need %zu B of LDS (> %d)", B->C, B->topk, B->D, p.cap, p.smem,
                lds::NARROW_MAX_LDS);
    // 32 workgroups of two hidden units each, unless the gradient is exchanged inside the kernel (16 channels)
    pool_w1_step_kernel<<<g.x.world > 1 ? H / 4 : H / 2, 1024, p.smem, s>>>(g, ws->pooled, ws->topk_idx, ws->topk_cnt, p.cap);
    MOC_CHECK_LAUNCH("moc_fused_step");
    return MOC_OK;
}
