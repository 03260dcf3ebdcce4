// The three-launch step and the loss-only entries.  A meta-step outside the one-launch kernels' shapes is
//   pooling + loss + pair gradients + Adam on b1 / W2 / b2: pool_step_kernel (one workgroup per slide; C, K <= 16), or
//       topk_mean_kernel (moc_select.hip, one workgroup per class) -> finish_kernel;
//   W1 gradient from the <= K*C gathered rows + Adam: w1_update_kernel (one thread per element).
// Evaluation takes the first of the two with train = 0 (moc_pool_loss).  Here too: Adam over gradients a caller has
// reduced himself (adam_all_kernel) and the senet backward for a caller-written loop (senet_bwd_rows_kernel).
#include "moc_step_shared.h"

int moc_launch_topk_mean(const float* keys, int64_t key_stride, const float* vals, int64_t val_stride,
                         const int64_t* seg_off, const int32_t* seg_len, int seg0, int n_seg, int C, int K,
                         int smallest, float* pooled, int32_t* idx_out, int32_t* cnt_out, hipStream_t s);

namespace {

// ------------------------------------------------------------------ loss (+ pair gradients)
// grid (n): one workgroup per slide.  Eval: CE + argmax only.  Train (n == 1): also the
// gradient "pairs" and the gradient/Adam of b1, W2, b2.
__global__ __launch_bounds__(256) void finish_kernel(FinishArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ float dpool[256];   // d loss / d pooled[c]
    const int b = a.slide0 + blockIdx.x, C = a.C;
    const float* x = a.pooled + (int64_t)b * C;
    const int y = (int)a.labels[b];
    if (threadIdx.x == 0) {
        float mx = -INFINITY;
        int arg = 0;
        for (int c = 0; c < C; ++c) if (x[c] > mx) { mx = x[c]; arg = c; }
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += expf(x[c] - mx);
        const float lse = mx + logf(se);
        a.loss[b] = lse - x[y];
        a.pred[b] = arg;
        if (a.train) for (int c = 0; c < C; ++c) dpool[c] = expf(x[c] - lse) - (c == y ? 1.f : 0.f);
    }
    if (!a.train) return;
    // Adam operands: requested now, consumed at the very end
    float oW = 0.f, oM = 0.f, oV = 0.f, oW2 = 0.f, oM2 = 0.f, oV2 = 0.f;
    if (a.apply_adam) {
        const int tt = threadIdx.x;
        oW = a.W2[tt]; oM = a.m_W2[tt]; oV = a.v_W2[tt];
        if (tt < 4) { oW2 = a.b2[tt]; oM2 = a.m_b2[tt]; oV2 = a.v_b2[tt]; }
        else if (tt >= 64 && tt < 64 + H) { oW2 = a.b1[tt - 64]; oM2 = a.m_b1[tt - 64]; oV2 = a.v_b1[tt - 64]; }
    }
    const int64_t base = a.row_off[b];
    const int cnt = a.topk_cnt[(int64_t)b * C];
    __syncthreads();

    // pairs p = (c, r): r-th pooled row of class c.  n_pair = sum_c cnt[c] <= C*K
    const lds::FinishLds Y = lds::finish_lds(C, a.K, 1);
    float* dz = reinterpret_cast<float*>(smem + Y.dz);
    int* prow = reinterpret_cast<int*>(smem + Y.prow);
    // every class pools the same number of rows: cnt = min(K, S)
    const int P = C * cnt;
    for (int p = threadIdx.x; p < P; p += 256) {
        const int c = p / cnt, r = p - c * cnt;
        const int s = a.topk_idx[((int64_t)b * C + c) * a.K + r];
        prow[p] = s;
        const float g = dpool[c] / (float)cnt;
        const float* cd = a.cand + base + s;
        const float sc[4] = {cd[(int64_t)c * a.stride], cd[(int64_t)(C + c) * a.stride],
                             cd[(int64_t)(2 * C) * a.stride], cd[(int64_t)(2 * C + 1) * a.stride]};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float lam = a.gates[(base + s) * 4 + i];
            const float dlam = (a.use_bits >> i & 1u) ? g * sc[i] : 0.f;
            dz[p * 4 + i] = dlam * lam * (1.f - lam);
        }
        a.pair_row[p] = a.sel_row[base + s];
    }
    if (threadIdx.x == 0) *a.n_pair = P;
    // H1 rows of the pairs go through LDS in chunks of FIN_CHUNK pairs (one coalesced round of gathers
    // per chunk): read per element from global memory, the W2 / b1 reductions below were P dependent
    // gathers long (68 us at C*K = 300).
    float* H1s = reinterpret_cast<float*>(smem + Y.H1s);
    float* W2s = reinterpret_cast<float*>(smem + Y.W2s);
    const int t = threadIdx.x, h = t & 63, g4 = t >> 6;
    W2s[t] = a.W2[t];
    float gW2 = 0.f, gb1 = 0.f;                 // W2[g4][h]; partial of b1[h] over the pairs p = g4 (mod 4)
    for (int c0 = 0; c0 < P; c0 += FIN_CHUNK) {
        const int n = P - c0 < FIN_CHUNK ? P - c0 : FIN_CHUNK;
        __syncthreads();                        // previous chunk consumed (first pass: dz / prow / W2s written)
        for (int e0 = 0; e0 < n * H; e0 += 16 * 256) {          // 16 independent gathers in flight per thread
            float r[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int e = e0 + q * 256 + t;
                r[q] = e < n * H ? a.H1[(base + prow[c0 + (e >> 6)]) * H + h] : 0.f;
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int e = e0 + q * 256 + t;
                if (e < n * H) H1s[e] = r[q];
            }
        }
        __syncthreads();
        for (int pp = g4; pp < n; pp += 4) {    // dh[p][h] = (sum_i dz[p][i] * W2[i][h]) * [H1 > 0]
            const float* dzp = dz + (size_t)(c0 + pp) * 4;
            float v = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) v = fmaf(dzp[i], W2s[i * H + h], v);
            v = H1s[pp * H + h] > 0.f ? v : 0.f;
            a.pair_dh[(size_t)(c0 + pp) * H + h] = v;
            gb1 += v;
        }
        for (int pp = 0; pp < n; ++pp) gW2 = fmaf(dz[(size_t)(c0 + pp) * 4 + g4], H1s[pp * H + h], gW2);
    }
    __syncthreads();
    H1s[t] = gb1;                               // b1[h] = the four partial sums, in a fixed order
    __syncthreads();
    const float gs = a.adam.grad_scale;
    if (a.apply_adam) {
        adam_update(oW, oM, oV, gW2 * gs, a.adam);
        a.W2[t] = oW; a.m_W2[t] = oM; a.v_W2[t] = oV;
    } else a.g_W2[t] = gW2;
    if (t < 4) {
        float g = 0.f;
        for (int p = 0; p < P; ++p) g += dz[p * 4 + t];
        if (a.apply_adam) {
            adam_update(oW2, oM2, oV2, g * gs, a.adam);
            a.b2[t] = oW2; a.m_b2[t] = oM2; a.v_b2[t] = oV2;
        } else a.g_b2[t] = g;
    }
    if (t >= 64 && t < 64 + H) {
        const int hh = t - 64;
        const float g = ((H1s[hh] + H1s[64 + hh]) + H1s[128 + hh]) + H1s[192 + hh];
        if (a.apply_adam) {
            adam_update(oW2, oM2, oV2, g * gs, a.adam);
            a.b1[hh] = oW2; a.m_b1[hh] = oM2; a.v_b1[hh] = oV2;
        } else a.g_b1[hh] = g;
    }
}

// ------------------------------------------------------------------ fused pooling + loss (+ step): pool_phase, moc_step_shared.h
// grid (n): one workgroup (1024 threads) per slide
__global__ __launch_bounds__(1024) void pool_step_kernel(FinishArgs a, float* pooled_out, int32_t* topk_idx_out,
                                                         int32_t* topk_cnt_out, int PS_CAP) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = a.slide0 + blockIdx.x, C = a.C, K = a.K;
    // LDS carve (all dynamic)
    const lds::PoolStepLds Y = lds::pool_step_lds(C, K, PS_CAP, 1);   // (evaluation returns before it touches the train part)
    float* dz = reinterpret_cast<float*>(smem + Y.dz);
    float* H1s = reinterpret_cast<float*>(smem + Y.H1s);
    float* dhs = reinterpret_cast<float*>(smem + Y.dhs);
    float* W2s = reinterpret_cast<float*>(smem + Y.W2s);
    MOC_STAMP(10);
    // operands that do not depend on this slide's scores: requested first, consumed last
    float pW = 0.f, pM = 0.f, pV = 0.f;       // parameter / exp_avg / exp_avg_sq this thread will step
    if (a.train) {
        const int t = threadIdx.x;
        if (t < 4 * H) { W2s[t] = pW = a.W2[t]; if (a.apply_adam) { pM = a.m_W2[t]; pV = a.v_W2[t]; } }
        else if (t < 4 * H + 4) { pW = a.b2[t - 4 * H]; if (a.apply_adam) { pM = a.m_b2[t - 4 * H]; pV = a.v_b2[t - 4 * H]; } }
        else if (t >= 320 && t < 320 + H) { pW = a.b1[t - 320]; if (a.apply_adam) { pM = a.m_b1[t - 320]; pV = a.v_b1[t - 320]; } }
    }
    int64_t base;
    const PoolLds L = pool_lds(smem, Y.pool);
    float* const dpool = L.dpool;
    int* const topk_s = L.topk_s;
    const int k = pool_phase(a, b, L, PS_CAP, true, pooled_out, topk_idx_out, topk_cnt_out, &base);
    MOC_STAMP(14);
    if (!a.train) return;
    __syncthreads();
    MOC_STAMP(15);
    // ---- pairs p = (class c, r-th pooled row): dz and the gathered H1 rows, one round of loads.
    // Entries p >= P (a slide with fewer than K selected rows) are zero / repeat pair 0's row so the
    // W1 kernel can run over the static bound C*K without reading n_pair.
    const int P = C * k, Pmax = C * K;
    // two (pair, hidden) elements per thread per sweep, both gathers in flight together
    for (int e0 = threadIdx.x; e0 < Pmax * H; e0 += 2048) {
        float hv[2];
        int sx[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int e = e0 + t * 1024;
            const int p = e >> 6, h = e & 63;
            const int pp = p < P ? p : 0;
            sx[t] = (P > 0 && e < Pmax * H) ? topk_s[(pp / k) * K + (pp - (pp / k) * k)] : 0;
            hv[t] = (p < P && e < Pmax * H) ? a.H1[(base + sx[t]) * H + h] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int e = e0 + t * 1024;
            if (e >= Pmax * H) continue;
            const int p = e >> 6, h = e & 63, sidx = sx[t];
            H1s[e] = hv[t];
            if (h < 4) {
                const int i = h;
                float dzv = 0.f;
                if (p < P) {
                    const int c = p / k;
                    const float g = dpool[c] / (float)k;
                    const float* cd = a.cand + base + sidx;
                    const float sc = i == 0 ? cd[(int64_t)c * a.stride] : i == 1 ? cd[(int64_t)(C + c) * a.stride]
                                   : i == 2 ? cd[(int64_t)(2 * C) * a.stride] : cd[(int64_t)(2 * C + 1) * a.stride];
                    const float lam = a.gates[(base + sidx) * 4 + i];
                    const float dlam = (a.use_bits >> i & 1u) ? g * sc : 0.f;
                    dzv = dlam * lam * (1.f - lam);
                }
                dz[p * 4 + i] = dzv;
            }
            if (h == 4) a.pair_row[p] = P > 0 ? a.sel_row[base + sidx] : 0;
        }
    }
    if (threadIdx.x == 0) *a.n_pair = P;
    __syncthreads();
    MOC_STAMP(16);
    // dh[p][h] = (sum_i dz[p][i] * W2[i][h]) * [H1 > 0]
    for (int e = threadIdx.x; e < Pmax * H; e += 1024) {
        const int p = e >> 6, h = e & 63;
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) v = fmaf(dz[p * 4 + i], W2s[i * H + h], v);
        v = H1s[e] > 0.f ? v : 0.f;
        dhs[e] = v;
        a.pair_dh[e] = v;
    }
    __syncthreads();
    MOC_STAMP(17);
    const float gs = a.adam.grad_scale;
    if (threadIdx.x < 4 * H) {          // W2 [4][H]
        const int i = threadIdx.x >> 6, h = threadIdx.x & 63;
        float g = 0.f;
        for (int p = 0; p < P; ++p) g = fmaf(dz[p * 4 + i], H1s[p * H + h], g);
        if (a.apply_adam) {
            adam_update(pW, pM, pV, g * gs, a.adam);
            a.W2[threadIdx.x] = pW; a.m_W2[threadIdx.x] = pM; a.v_W2[threadIdx.x] = pV;
        } else a.g_W2[threadIdx.x] = g;
    } else if (threadIdx.x < 4 * H + 4) {
        const int i = threadIdx.x - 4 * H;
        float g = 0.f;
        for (int p = 0; p < P; ++p) g += dz[p * 4 + i];
        if (a.apply_adam) {
            adam_update(pW, pM, pV, g * gs, a.adam);
            a.b2[i] = pW; a.m_b2[i] = pM; a.v_b2[i] = pV;
        } else a.g_b2[i] = g;
    } else if (threadIdx.x >= 320 && threadIdx.x < 320 + H) {
        const int h = threadIdx.x - 320;
        float g = 0.f;
        for (int p = 0; p < P; ++p) g += dhs[p * H + h];
        if (a.apply_adam) {
            adam_update(pW, pM, pV, g * gs, a.adam);
            a.b1[h] = pW; a.m_b1[h] = pM; a.v_b1[h] = pV;
        } else a.g_b1[h] = g;
    }
    MOC_STAMP(18);
}

// ------------------------------------------------------------------ W1 gradient (+ Adam)
struct W1Args {
    const unsigned char* X;
    const float* pair_dh;
    const int64_t* pair_row;
    const int32_t* n_pair;
    float *W1, *m_W1, *v_W1, *g_W1;
    unsigned char* W1img;   // kept in sync with W1 when the step is applied (nullable)
    int D, apply_adam;
    int P_static;           // >= 0: pair count known to the host (padded list), else read n_pair
    AdamCoef adam;
};

// dW1[h][d] = sum_p dh[p][h] * x_p[d] over the <= K*C gradient pairs, then Adam in place.
// grid (D/256, H/8): a workgroup owns 256 columns d and 8 hidden units.  Everything it needs is
// requested at once: its 8 x 256 parameters and moments, and the pairs' row segments (P x 256
// elements, via LDS) -- with `P_static` >= 0 (the fused step pads its pair list to C*K entries with
// zero dh) not even n_pair has to arrive first.
constexpr int W1_MAXP = 64;
template <bool BF16, bool F16 = false>
__global__ __launch_bounds__(256) void w1_update_kernel(W1Args a) {
    __shared__ __attribute__((aligned(16))) float xs[W1_MAXP][256];
    __shared__ float dh_s[W1_MAXP][8];
    __shared__ int64_t prow_s[W1_MAXP];
    const int d = blockIdx.x * 256 + threadIdx.x, h0 = blockIdx.y * 8;
    MOC_STAMP(20);
    float pw[8], pm[8], pv[8];
    if (a.apply_adam) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int e = (h0 + j) * a.D + d;
            pw[j] = a.W1[e]; pm[j] = a.m_W1[e]; pv[j] = a.v_W1[e];
        }
    }
    const int P = a.P_static >= 0 ? a.P_static : *a.n_pair;
    float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int p0 = 0; p0 < P; p0 += W1_MAXP) {
        const int np = P - p0 < W1_MAXP ? P - p0 : W1_MAXP;
        if (p0 > 0) __syncthreads();
        {
            // 16-B loads, all independent: LPR lanes cover one row's 256 columns, 256/LPR rows per round
            if (threadIdx.x < np) prow_s[threadIdx.x] = a.pair_row[p0 + threadIdx.x];
            __syncthreads();
            constexpr int EPL = BF16 ? 8 : 4, LPR = 256 / EPL, RPR = 256 / LPR;   // elements/lane, lanes/row, rows/round
            const int v = threadIdx.x % LPR, pr = threadIdx.x / LPR;
            const int64_t col = (int64_t)blockIdx.x * 256 + v * EPL;
#pragma unroll
            for (int r = 0; r < W1_MAXP / RPR; ++r) {
                const int p = r * RPR + pr;
                if (p < np) {
                    const int64_t row = prow_s[p];
                    float* dst = &xs[p][v * EPL];
                    if constexpr (BF16) {
                        const uint4 raw = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(a.X) + row * a.D + col);
                        float4 lo, hi;
                        lo.x = moc_half_to_f32<F16>((uint16_t)raw.x); lo.y = moc_half_to_f32<F16>((uint16_t)(raw.x >> 16));
                        lo.z = moc_half_to_f32<F16>((uint16_t)raw.y); lo.w = moc_half_to_f32<F16>((uint16_t)(raw.y >> 16));
                        hi.x = moc_half_to_f32<F16>((uint16_t)raw.z); hi.y = moc_half_to_f32<F16>((uint16_t)(raw.z >> 16));
                        hi.z = moc_half_to_f32<F16>((uint16_t)raw.w); hi.w = moc_half_to_f32<F16>((uint16_t)(raw.w >> 16));
                        reinterpret_cast<float4*>(dst)[0] = lo;
                        reinterpret_cast<float4*>(dst)[1] = hi;
                    } else {
                        *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(a.X) + row * a.D + col);
                    }
                }
            }
        }
        for (int e = threadIdx.x; e < np * 8; e += 256) dh_s[e >> 3][e & 7] = a.pair_dh[(p0 + (e >> 3)) * H + h0 + (e & 7)];
        __syncthreads();
        MOC_STAMP(21);
        for (int p = 0; p < np; ++p) {
            const float xv = xs[p][threadIdx.x];
#pragma unroll
            for (int j = 0; j < 8; ++j) g[j] = fmaf(dh_s[p][j], xv, g[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int e = (h0 + j) * a.D + d;
        if (a.apply_adam) {
            adam_update(pw[j], pm[j], pv[j], g[j] * a.adam.grad_scale, a.adam);
            a.W1[e] = pw[j]; a.m_W1[e] = pm[j]; a.v_W1[e] = pv[j];
            if (a.W1img) {
                if constexpr (F16) w1_image_store_half<true>(a.W1img, a.D, h0 + j, d, pw[j]);
                else if constexpr (BF16) w1_image_store_half<false>(a.W1img, a.D, h0 + j, d, pw[j]);
                else w1_image_store_f32(a.W1img, a.D, h0 + j, d, pw[j]);
            }
        } else a.g_W1[e] = g[j];
    }
    MOC_STAMP(22);
}

// gradients already in g_* (e.g. after an all-reduce): plain Adam over all four tensors
// (+ the W1 image when `img` is given, so that the next forward needs no rebuild)
__global__ __launch_bounds__(256) void adam_all_kernel(moc_meta_t M, int D, AdamCoef k, unsigned char* img, int img_dt) {
    const int nW1 = H * D, n = nW1 + H + 4 * H + 4;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float *p, *m, *v, *g;
    int o = e;
    if (o < nW1) { p = M.W1; m = M.m_W1; v = M.v_W1; g = M.g_W1; }
    else if ((o -= nW1) < H) { p = M.b1; m = M.m_b1; v = M.v_b1; g = M.g_b1; }
    else if ((o -= H) < 4 * H) { p = M.W2; m = M.m_W2; v = M.v_W2; g = M.g_W2; }
    else { o -= 4 * H; p = M.b2; m = M.m_b2; v = M.v_b2; g = M.g_b2; }
    adam_update(p[o], m[o], v[o], g[o] * k.grad_scale, k);
    if (img && e < nW1) {
        w1_image_store(img_dt, img, D, e / D, e % D, p[o]);
    }
}

// ------------------------------------------------------------------ senet backward for a caller-written loop
// `lambdas = model(selected_feat)` kept by a caller who wrote the reference's loop body himself (main_moc.py:390-410):
// autograd hands back d loss / d lambdas [S, 4] -- zero except on the <= K*C rows that reached a class's top-K.  One
// workgroup lists the rows that carry gradient (ascending), forms dz = g * lam * (1 - lam), dh = (dz W2) * [H1 > 0] and
// the gradients of b1 / W2 / b2; the W1 gradient is w1_update_kernel over that list, as in the three-launch step.
// A dense d lambdas (some other loss) is the same code with a list of S rows.
__global__ __launch_bounds__(1024) void senet_bwd_rows_kernel(const float* H1, const float* gates, const float* gg, const float* W2,
                                                              int64_t S, float* pair_dz, float* pair_dh, int64_t* pair_row,
                                                              int32_t* n_pair, float* g_b1, float* g_W2, float* g_b2) {
    __shared__ int wcnt[16];
    __shared__ int total_s;
    __shared__ float W2s[4 * H];
    __shared__ float red[16][5 * H];                         // per p-group partials: W2 gradient [4][H] | b1 gradient [H]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t < 4 * H) W2s[t] = W2[t];
    if (t == 0) total_s = 0;
    __syncthreads();
    for (int64_t r0 = 0; r0 < S; r0 += 1024) {
        const int64_t r = r0 + t;
        float4 g = {0.f, 0.f, 0.f, 0.f}, lam = {0.f, 0.f, 0.f, 0.f};
        if (r < S) {
            g = reinterpret_cast<const float4*>(gg)[r];
            lam = reinterpret_cast<const float4*>(gates)[r];
        }
        const bool act = g.x != 0.f || g.y != 0.f || g.z != 0.f || g.w != 0.f;
        const unsigned long long bal = __ballot(act);
        if (lane == 0) wcnt[wave] = __popcll(bal);
        __syncthreads();
        int before = total_s;
        for (int w = 0; w < wave; ++w) before += wcnt[w];
        if (act) {
            const int pos = before + __popcll(bal & ((1ull << lane) - 1ull));
            pair_row[pos] = r;
            float4 dz;
            dz.x = g.x * lam.x * (1.f - lam.x); dz.y = g.y * lam.y * (1.f - lam.y);
            dz.z = g.z * lam.z * (1.f - lam.z); dz.w = g.w * lam.w * (1.f - lam.w);
            reinterpret_cast<float4*>(pair_dz)[pos] = dz;
        }
        __syncthreads();
        if (t == 0) { int a = total_s; for (int w = 0; w < 16; ++w) a += wcnt[w]; total_s = a; }
        __syncthreads();
    }
    const int P = total_s;
    if (t == 0) *n_pair = P;
    __threadfence_block();
    __syncthreads();
    // thread (p-group t >> 6, hidden unit t & 63): pairs p = group, group + 16, ...
    const int h = t & 63, grp = t >> 6;
    float gb1 = 0.f, gw[4] = {0.f, 0.f, 0.f, 0.f};
    for (int p = grp; p < P; p += 16) {
        const float4 dz = reinterpret_cast<const float4*>(pair_dz)[p];
        const float hv = H1[pair_row[p] * H + h];
        float v = 0.f;
        v = fmaf(dz.x, W2s[0 * H + h], v); v = fmaf(dz.y, W2s[1 * H + h], v);
        v = fmaf(dz.z, W2s[2 * H + h], v); v = fmaf(dz.w, W2s[3 * H + h], v);
        v = hv > 0.f ? v : 0.f;
        pair_dh[(int64_t)p * H + h] = v;
        gb1 += v;
        gw[0] = fmaf(dz.x, hv, gw[0]); gw[1] = fmaf(dz.y, hv, gw[1]);
        gw[2] = fmaf(dz.z, hv, gw[2]); gw[3] = fmaf(dz.w, hv, gw[3]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) red[grp][i * H + h] = gw[i];
    red[grp][4 * H + h] = gb1;
    __syncthreads();
    if (t < 5 * H) {                                          // the sixteen partial sums, in a fixed order
        float a = 0.f;
        for (int g16 = 0; g16 < 16; ++g16) a += red[g16][t];
        if (t < 4 * H) g_W2[t] = a; else g_b1[t - 4 * H] = a;
    } else if (t < 5 * H + 4) {
        const int i = t - 5 * H;
        float a = 0.f;
        for (int p = 0; p < P; ++p) a += pair_dz[(int64_t)p * 4 + i];
        g_b2[i] = a;
    }
}

int launch_finish(const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws, const int64_t* labels,
                  int slide0, int n, int train, int apply_adam, uint32_t use_bits, const AdamCoef& k, hipStream_t s) {
    FinishArgs a = finish_args(B, M, ws, labels, slide0, train, apply_adam, use_bits, k);
    a.topk_idx = ws->topk_idx; a.topk_cnt = ws->topk_cnt;
    a.pair_dh = ws->pair_dh; a.pair_row = ws->pair_row; a.n_pair = ws->n_pair;
    // (the layout counts in 32 bits, and topk has no bound of its own: the pairs are checked, which is the same check)
    MOC_REQUIRE(!train || (int64_t)B->C * B->topk <= lds::FINISH_MAX_PAIRS, "finish_kernel: C = %d, topk = %d: more than %d pairs (%d B of LDS)",
                B->C, B->topk, lds::FINISH_MAX_PAIRS, lds::FINISH_MAX_LDS);
    const int smem = lds::finish_lds(B->C, B->topk, train).bytes;
    finish_kernel<<<n, 256, smem, s>>>(a);
    MOC_CHECK_LAUNCH("moc_finish");
    return MOC_OK;
}

// the kernel of the bag's storage type over a filled argument block
int launch_w1_kernel(const W1Args& a, int dtype, hipStream_t s, const char* who) {
    const dim3 grid(a.D / 256, H / 8);
    if (dtype == MOC_F16) w1_update_kernel<true, true><<<grid, 256, 0, s>>>(a);
    else if (dtype == MOC_BF16) w1_update_kernel<true><<<grid, 256, 0, s>>>(a);
    else w1_update_kernel<false><<<grid, 256, 0, s>>>(a);
    MOC_CHECK_LAUNCH(who);
    return MOC_OK;
}

}  // namespace

void moc_meta_internal::pool_step_attrs(raise_lds_fn raise) {
    raise("finish_kernel", (const void*)finish_kernel, lds::FINISH_MAX_LDS);
    raise("pool_step_kernel", (const void*)pool_step_kernel, lds::POOL_STEP_MAX_LDS);
}

int moc_meta_internal::launch_pool(const moc_batch_t* B, const moc_meta_ws_t* ws, int slide0, int n, hipStream_t s) {
    return moc_launch_topk_mean(ws->mixed, B->total_rows, ws->mixed, B->total_rows, B->row_off, B->n_sel,
                                slide0, n, B->C, B->topk, 0, ws->pooled, ws->topk_idx, ws->topk_cnt, s);
}

int moc_meta_internal::launch_pool_finish(const StepPlan& p, const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws,
                                          const int64_t* labels, int slide0, int n, int train, int apply_adam, uint32_t use_bits,
                                          const AdamCoef& k, hipStream_t s) {
    if (!p.pool_one) {
        if (int rc = launch_pool(B, ws, slide0, n, s)) return rc;
        return launch_finish(B, M, ws, labels, slide0, n, train, apply_adam, use_bits, k, s);
    }
    FinishArgs a = finish_args(B, M, ws, labels, slide0, train, apply_adam, use_bits, k);
    finish_rows(a, B, ws, slide0, n == 1);
    a.pair_dh = ws->pair_dh; a.pair_row = ws->pair_row; a.n_pair = ws->n_pair;
    const int smem = lds::pool_step_lds(B->C, B->topk, p.cap, train).bytes;   // (pool_one: C, topk <= 16)
    MOC_REQUIRE(smem <= lds::POOL_STEP_MAX_LDS, "pool_step_kernel: C = %d, topk = %d, cap = %d, train = %d need %d B of LDS (> %d)",
                B->C, B->topk, p.cap, train, smem, lds::POOL_STEP_MAX_LDS);
    pool_step_kernel<<<n, 1024, smem, s>>>(a, ws->pooled, ws->topk_idx, ws->topk_cnt, p.cap);
    MOC_CHECK_LAUNCH("moc_pool_step");
    return MOC_OK;
}

int moc_meta_internal::launch_w1(const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws, int apply_adam,
                                 const AdamCoef& k, hipStream_t s, bool padded_pairs) {
    W1Args a;
    a.P_static = padded_pairs ? B->C * B->topk : -1;
    // (measured: gathering the pairs' rows in the single-workgroup step kernel for this kernel costs
    // more there (+2 us) than it saves here (-1.4 us): the rows are gathered here)
    a.W1img = (unsigned char*)M->W1_image;
    a.X = (const unsigned char*)B->X; a.pair_dh = ws->pair_dh; a.pair_row = ws->pair_row; a.n_pair = ws->n_pair;
    a.W1 = M->W1; a.m_W1 = M->m_W1; a.v_W1 = M->v_W1; a.g_W1 = M->g_W1; a.D = B->D; a.apply_adam = apply_adam; a.adam = k;
    return launch_w1_kernel(a, B->dtype, s, "moc_w1_update");
}

int moc_meta_internal::launch_adam_all(const moc_meta_t* M, const AdamCoef& k, unsigned char* img, int img_dt, hipStream_t s,
                                       const char* who) {
    adam_all_kernel<<<moc_cdiv(n_params(M->D), 256), 256, 0, s>>>(*M, M->D, k, img, img_dt);
    MOC_CHECK_LAUNCH(who);
    return MOC_OK;
}

extern "C" int moc_pool_loss(const moc_batch_t* B, const moc_meta_ws_t* ws, const int64_t* labels,
                             int slide0, int n, moc_stream_t stream) {
    if (int rc = moc_check_batch(B, "moc_pool_loss")) return rc;
    MOC_REQUIRE(ws && labels, "moc_pool_loss: null ws/labels");
    MOC_REQUIRE(slide0 >= 0 && n >= 1 && slide0 + n <= B->n_slides, "moc_pool_loss: bad slide range");
    MOC_REQUIRE(B->C <= 256, "moc_pool_loss: C > 256");
    hipStream_t s = (hipStream_t)stream;
    (void)step_attrs();   // (pool_step_kernel's limit is among them; a training kernel's failure is not this entry's error)
    moc_meta_t none = {};
    AdamCoef k = {};
    return launch_pool_finish(step_plan(B, ws, false, 0), B, &none, ws, labels, slide0, n, 0, 0, 0, k, s);
}

extern "C" int moc_ce_loss(const float* pooled, const int64_t* labels, int n, int C, float* loss, int32_t* pred,
                           moc_stream_t stream) {
    MOC_REQUIRE(pooled && labels && loss && pred, "moc_ce_loss: null pointer");
    MOC_REQUIRE(n >= 1 && C >= 1 && C <= 256, "moc_ce_loss: bad n=%d C=%d (C <= 256)", n, C);
    FinishArgs a = {};
    a.pooled = pooled; a.labels = labels; a.loss = loss; a.pred = pred; a.C = C; a.slide0 = 0; a.train = 0;
    finish_kernel<<<n, 256, 0, (hipStream_t)stream>>>(a);
    MOC_CHECK_LAUNCH("moc_ce_loss");
    return MOC_OK;
}

extern "C" int moc_senet_backward(const void* X, int dtype, int64_t S, int D, const float* H1, const float* gates,
                                  const float* grad_gates, const float* W2, float* g_W1, float* g_b1, float* g_W2, float* g_b2,
                                  float* pair_dz, float* pair_dh, int64_t* pair_row, int32_t* n_pair, moc_stream_t stream) {
    MOC_REQUIRE(X && H1 && gates && grad_gates && W2 && g_W1 && g_b1 && g_W2 && g_b2 && pair_dz && pair_dh && pair_row && n_pair,
                "moc_senet_backward: null pointer");
    MOC_REQUIRE(dtype == MOC_F32 || dtype == MOC_BF16 || dtype == MOC_F16, "moc_senet_backward: bad dtype %d", dtype);
    MOC_REQUIRE(S >= 1 && D > 0 && D % 256 == 0, "moc_senet_backward: bad shape S=%lld D=%d (D a multiple of 256)", (long long)S, D);
    hipStream_t s = (hipStream_t)stream;
    senet_bwd_rows_kernel<<<1, 1024, 0, s>>>(H1, gates, grad_gates, W2, S, pair_dz, pair_dh, pair_row, n_pair, g_b1, g_W2, g_b2);
    MOC_CHECK_LAUNCH("moc_senet_backward(rows)");
    W1Args a = {};
    a.P_static = -1;
    a.X = (const unsigned char*)X; a.pair_dh = pair_dh; a.pair_row = pair_row; a.n_pair = n_pair;
    a.g_W1 = g_W1; a.D = D; a.apply_adam = 0;
    return launch_w1_kernel(a, dtype, s, "moc_senet_backward(W1)");
}

extern "C" int moc_adam_step(const moc_meta_t* M, float grad_scale, moc_stream_t stream) {
    MOC_REQUIRE(M && M->H == H && M->D > 0, "moc_adam_step: bad meta");
    MOC_REQUIRE(M->W1 && M->m_W1 && M->v_W1 && M->g_W1 && M->b1 && M->m_b1 && M->v_b1 && M->g_b1 &&
                M->W2 && M->m_W2 && M->v_W2 && M->g_W2 && M->b2 && M->m_b2 && M->v_b2 && M->g_b2,
                "moc_adam_step: null tensor");
    const AdamCoef k = adam_coef(M, M->step + 1, grad_scale);
    return launch_adam_all(M, k, nullptr, 0, (hipStream_t)stream, "moc_adam_step");
}
