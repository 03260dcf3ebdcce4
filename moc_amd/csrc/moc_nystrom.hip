// Fused Nystrom attention forward for TransMIL's no-grad passes (moc_amd/nystrom.py).  One shape:
// 8 heads x 64, 256 landmarks, a residual convolution of up to 33 taps, batch 1.  Both kernels read qkv as to_qkv leaves
// it -- [n_pad, 1536] fp32, token-major: q of head h at columns 64 h, k at 512 + 64 h, v at 1024 + 64 h -- and neither
// forms a score matrix in memory.
//
//   A (landmark side):  W_h = softmax_over_tokens(q_l[h] k[h]^T) v[h]                                   [256, 64]
//   B (token side):     out[i, 64 h ..] = softmax_256(scale q[i, h] k_l[h]^T) Y_h + sum_t w[h, t] v[i + t - taps / 2, h]
//
// Arithmetic: the f32-input MFMA v_mfma_f32_16x16x4_f32 (an fp32 fmaf chain, bit for bit): no operand splitting, one VGPR
// per operand, and the 16 GFLOP of a 15,360-token layer are 0.1 ms at its peak -- the softmax's exponentials, not the
// products, are what the six-term bf16 form would have left on the critical path.  Lane l of a wave holds A[l & 15][l >> 4]
// and B[l >> 4][l & 15]; the result has its column on l & 15 and rows 4 (l >> 4) + 0..3 in its four registers.
//
// Both kernels compute the scores TRANSPOSED (keys or landmarks x queries), so that a score tile's register r of lane
// (g = l >> 4, c = l & 15) is the softmax weight of (row 4 g + r, column c): since the four K slots of an MFMA may stand for
// any four indices as long as both operands agree, register r IS the B operand of the step whose slot g means row 4 g + r
// of the tile -- the softmax result feeds the second product from where it lies, without LDS.  The other operand of that
// step is V (or Y) [row 4 g + r][4 c + 0..3], one float4 per lane, component dt going to output tile dt: output tile dt
// holds, in register r' of lane (g, c), feature 16 g + 4 r' + dt -- a lane ends with 16 consecutive features of ITS column
// (a landmark in A, a token in B) and stores four float4.  Maxima, sums and rescaling are per column, hence per lane
// (two cross-lane steps over g).  In the first product slot g of step s stands for feature 16 g + s: a lane loads 16
// consecutive floats of its row of k (or q).
//
// A: a workgroup is one head x one range of 512 tokens (NY_CHUNK); its eight waves own 32 landmarks each (two waves per SIMD: one's
// exponentials run beside the other's MFMAs) and walk the range 16 tokens at a time with a running maximum and sum.  Each range leaves (max, sum, accumulator) in the workspace; a
// second launch merges the ranges in index order: no atomics, the same bits on every call.
// B: a workgroup is one head x 256 tokens; k_l[h] and Y[h] (64 KiB each) are laid out in LDS in operand order (consecutive
// lanes read consecutive 16 bytes); each of eight waves takes two 16-token tiles: 256 landmark scores per token in
// registers, one softmax, the product with Y, then the residual convolution as 12 more MFMA steps over the 48 rows of v
// around the tile against the banded tap matrix T[i', i] = w[i' - i + taps / 2] (rows outside [0, n_pad) count as zero).
#include "moc_nystrom_shared.h"

namespace {

constexpr int NY_A_LT = 2;                               // 16-landmark tiles per wave of kernel A: eight waves, two per SIMD
constexpr int NY_A_THREADS = NY_M / (16 * NY_A_LT) * 64;
constexpr int NY_B_SMEM = 2 * NY_M * NY_D * 4 + 64 * 4;  // k_l image, Y image, tap table

size_t ny_ws_bytes(int64_t n_pad) { return (size_t)ny_chunks(n_pad) * NY_HEADS * NY_M * (NY_D + 2) * sizeof(float); }

struct NyAArgs {
    const float* qkv;      // [n_pad, 1536]
    const float* q_l;      // [8, 256, 64], scaled
    float* part;           // [8, chunks, 256, 64] accumulators, then [8, chunks, 256] maxima, then [8, chunks, 256] sums
    int64_t n_pad;
    int chunks;
};

__global__ __launch_bounds__(NY_A_THREADS) void nystrom_landmark_kernel(NyAArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int chunk = blockIdx.x, h = blockIdx.y;
    const int64_t t0 = (int64_t)chunk * NY_CHUNK;
    const int64_t t1 = t0 + NY_CHUNK < a.n_pad ? t0 + NY_CHUNK : a.n_pad;

    float ql[NY_A_LT][16];                                                  // B operand: q_l[landmark c of tile lt][16 g + s]
#pragma unroll
    for (int lt = 0; lt < NY_A_LT; ++lt) {
        const float* p = a.q_l + ((int64_t)h * NY_M + (wave * NY_A_LT + lt) * 16 + c) * NY_D + 16 * g;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 v = ny_ld4(p + 4 * j);
            ql[lt][4 * j] = v.x; ql[lt][4 * j + 1] = v.y; ql[lt][4 * j + 2] = v.z; ql[lt][4 * j + 3] = v.w;
        }
    }
    const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4_t acc[NY_A_LT][4];
    float mx[NY_A_LT], sm[NY_A_LT];                                               // sm: this lane's share (its rows 4 g + r) of the sum
#pragma unroll
    for (int lt = 0; lt < NY_A_LT; ++lt) {
        mx[lt] = -INFINITY; sm[lt] = 0.f;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) acc[lt][dt] = zero4;
    }
    const float* kp = a.qkv + 512 + 64 * h + 16 * g;                  // + (t + c) * 1536
    const float* vp = a.qkv + 1024 + 64 * h + 4 * c;                  // + (t + 4 g + r) * 1536
    float4 kn[4], vn[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        kn[j] = ny_ld4(kp + (t0 + c) * NY_ROW + 4 * j);
        vn[j] = ny_ld4(vp + (t0 + 4 * g + j) * NY_ROW);
    }
#pragma unroll 1
    for (int64_t t = t0; t < t1; t += 16) {
        float kc[16];
        float4 vc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            kc[4 * j] = kn[j].x; kc[4 * j + 1] = kn[j].y; kc[4 * j + 2] = kn[j].z; kc[4 * j + 3] = kn[j].w;
            vc[j] = vn[j];
        }
        const int64_t tn = t + 16 < t1 ? t + 16 : t;                  // the last tile re-reads itself: loads stay inside
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            kn[j] = ny_ld4(kp + (tn + c) * NY_ROW + 4 * j);
            vn[j] = ny_ld4(vp + (tn + 4 * g + j) * NY_ROW);
        }
        // scores^T: 16 tokens x this wave's 32 landmarks; two chains per tile (even / odd features)
        f32x4_t s0[NY_A_LT], s1[NY_A_LT];
#pragma unroll
        for (int lt = 0; lt < NY_A_LT; ++lt) { s0[lt] = zero4; s1[lt] = zero4; }
#pragma unroll
        for (int s = 0; s < 16; s += 2)
#pragma unroll
            for (int lt = 0; lt < NY_A_LT; ++lt) {
                s0[lt] = ny_mfma(kc[s], ql[lt][s], s0[lt]);
                s1[lt] = ny_mfma(kc[s + 1], ql[lt][s + 1], s1[lt]);
            }
        f32x4_t p[NY_A_LT];
#pragma unroll
        for (int lt = 0; lt < NY_A_LT; ++lt) {
            const f32x4_t sv = s0[lt] + s1[lt];
            const float tm = ny_col_max(fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3])));
            const float mn = fmaxf(mx[lt], tm);
            const float alpha = expf(mx[lt] - mn);                    // 0 on the first tile (mx = -inf)
            mx[lt] = mn;
#pragma unroll
            for (int r = 0; r < 4; ++r) p[lt][r] = expf(sv[r] - mn);
            sm[lt] = sm[lt] * alpha + ((p[lt][0] + p[lt][1]) + (p[lt][2] + p[lt][3]));
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) acc[lt][dt] *= alpha;
        }
        // W^T += v^T p^T: step r, slot g = token 4 g + r
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float vv[4] = {vc[r].x, vc[r].y, vc[r].z, vc[r].w};
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int lt = 0; lt < NY_A_LT; ++lt) acc[lt][dt] = ny_mfma(vv[dt], p[lt][r], acc[lt][dt]);
        }
    }
    const int64_t pi = (int64_t)h * a.chunks + chunk;
    float* pacc = a.part;
    float* pmx = a.part + (int64_t)NY_HEADS * a.chunks * NY_M * NY_D;
    float* psm = pmx + (int64_t)NY_HEADS * a.chunks * NY_M;
#pragma unroll
    for (int lt = 0; lt < NY_A_LT; ++lt) {
        const int64_t lm = pi * NY_M + (wave * NY_A_LT + lt) * 16 + c;
        const float tot = ny_col_sum(sm[lt]);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            *reinterpret_cast<float4*>(pacc + lm * NY_D + 16 * g + 4 * r) =
                float4{acc[lt][0][r], acc[lt][1][r], acc[lt][2][r], acc[lt][3][r]};
        if (g == 0) { pmx[lm] = mx[lt]; psm[lm] = tot; }
    }
}

// one thread per (head, landmark, four features): the ranges in index order; `lse` (or null) takes each landmark's
// log-sum-exp over the tokens, m + log(den), which the backward recomputes the weights from
__global__ __launch_bounds__(256) void nystrom_merge_kernel(const float* part, int chunks, float* W, float* lse) {
    const int idx = blockIdx.x * 256 + threadIdx.x;                   // < 8 * 256 * 16
    const int d4 = idx & 15, lm = (idx >> 4) & (NY_M - 1), h = idx >> 12;
    const float* pmx = part + (int64_t)NY_HEADS * chunks * NY_M * NY_D;
    const float* psm = pmx + (int64_t)NY_HEADS * chunks * NY_M;
    float m = -INFINITY;
    for (int k = 0; k < chunks; ++k) m = fmaxf(m, pmx[((int64_t)h * chunks + k) * NY_M + lm]);
    float den = 0.f;
    float4 num = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < chunks; ++k) {
        const int64_t row = ((int64_t)h * chunks + k) * NY_M + lm;
        const float w = expf(pmx[row] - m);
        const float4 v = ny_ld4(part + row * NY_D + 4 * d4);
        den += psm[row] * w;
        num.x += v.x * w; num.y += v.y * w; num.z += v.z * w; num.w += v.w * w;
    }
    *reinterpret_cast<float4*>(W + ((int64_t)h * NY_M + lm) * NY_D + 4 * d4) =
        float4{num.x / den, num.y / den, num.z / den, num.w / den};
    if (lse && d4 == 0) lse[h * NY_M + lm] = m + logf(den);
}

struct NyBArgs {
    const float* qkv;      // [n_pad, 1536]
    const float* k_l;      // [8, 256, 64]
    const float* Y;        // [8, 256, 64]
    const float* conv_w;   // [8, taps] or null
    float* out;            // [n_pad, 512]
    int64_t n_pad;
    int taps;
    float scale;
};

__global__ __launch_bounds__(512) void nystrom_token_kernel(NyBArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4* kimg = reinterpret_cast<float4*>(smem);                   // [landmark tile 16][j 4][lane 64]
    float4* yimg = kimg + NY_M * NY_D / 4;                            // [landmark tile 16][r 4][lane 64]
    float* wt = reinterpret_cast<float*>(yimg + NY_M * NY_D / 4);     // wt[32 + i' - i] = w[i' - i + taps / 2], or 0
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int h = blockIdx.y;
    const int64_t tok_base = (int64_t)blockIdx.x * NY_B_TOK;
    for (int idx = threadIdx.x; idx < NY_M * NY_D / 4; idx += 512) {
        const int ln = idx & 63, f = idx >> 6, lt = f >> 2, j = f & 3, cc = ln & 15, gg = ln >> 4;
        kimg[idx] = ny_ld4(a.k_l + ((int64_t)h * NY_M + lt * 16 + cc) * NY_D + 16 * gg + 4 * j);
        yimg[idx] = ny_ld4(a.Y + ((int64_t)h * NY_M + lt * 16 + 4 * gg + j) * NY_D + 4 * cc);
    }
    if (threadIdx.x < 64) {
        const int tap = (int)threadIdx.x - 32 + a.taps / 2;
        wt[threadIdx.x] = a.conv_w && tap >= 0 && tap < a.taps ? a.conv_w[h * a.taps + tap] : 0.f;
    }
    __syncthreads();
    const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int tile = wave; tile < NY_B_TOK / 16; tile += 8) {
        const int64_t tok0 = tok_base + tile * 16;
        float q[16];                                                  // B operand: scale q[token c][16 g + s]
        {
            const float* p = a.qkv + (tok0 + c) * NY_ROW + 64 * h + 16 * g;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 v = ny_ld4(p + 4 * j);
                q[4 * j] = moc_fmul(v.x, a.scale); q[4 * j + 1] = moc_fmul(v.y, a.scale);
                q[4 * j + 2] = moc_fmul(v.z, a.scale); q[4 * j + 3] = moc_fmul(v.w, a.scale);
            }
        }
        f32x4_t S[16];                                                // scores^T: landmark 16 lt + 4 g + r, token c
        float4 kf[4], kg[4];                                          // this tile's fragments and the next one's, read a step ahead
#pragma unroll
        for (int j = 0; j < 4; ++j) kf[j] = kimg[j * 64 + lane];
#pragma unroll
        for (int lt = 0; lt < 16; ++lt) {
            const int ln = lt + 1 < 16 ? lt + 1 : lt;
#pragma unroll
            for (int j = 0; j < 4; ++j) kg[j] = kimg[(ln * 4 + j) * 64 + lane];
            f32x4_t s0 = zero4, s1 = zero4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s0 = ny_mfma(kf[j].x, q[4 * j], s0);
                s1 = ny_mfma(kf[j].y, q[4 * j + 1], s1);
                s0 = ny_mfma(kf[j].z, q[4 * j + 2], s0);
                s1 = ny_mfma(kf[j].w, q[4 * j + 3], s1);
            }
            S[lt] = s0 + s1;
#pragma unroll
            for (int j = 0; j < 4; ++j) kf[j] = kg[j];
            __builtin_amdgcn_sched_barrier(0);          // keep each step's LDS reads beside the MFMAs they overlap
        }
        float m = -INFINITY;
#pragma unroll
        for (int lt = 0; lt < 16; ++lt) m = fmaxf(m, fmaxf(fmaxf(S[lt][0], S[lt][1]), fmaxf(S[lt][2], S[lt][3])));
        m = ny_col_max(m);
        float ps[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int lt = 0; lt < 16; ++lt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                S[lt][r] = expf(S[lt][r] - m);
                ps[r] += S[lt][r];
            }
        const float den = ny_col_sum((ps[0] + ps[1]) + (ps[2] + ps[3]));
        // out^T = Y^T p^T: step (lt, r), slot g = landmark 16 lt + 4 g + r; even / odd landmark tiles in chains of their own
        f32x4_t oe[4], oo[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) { oe[dt] = zero4; oo[dt] = zero4; }
        float4 yf[2], yg[2];
        yf[0] = yimg[lane]; yf[1] = yimg[4 * 64 + lane];
#pragma unroll
        for (int lt = 0; lt < 16; lt += 2)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int nr = (r + 1) & 3, nl = r == 3 ? (lt + 2 < 16 ? lt + 2 : lt) : lt;
                yg[0] = yimg[(nl * 4 + nr) * 64 + lane]; yg[1] = yimg[((nl + 1) * 4 + nr) * 64 + lane];
                oe[0] = ny_mfma(yf[0].x, S[lt][r], oe[0]); oe[1] = ny_mfma(yf[0].y, S[lt][r], oe[1]);
                oe[2] = ny_mfma(yf[0].z, S[lt][r], oe[2]); oe[3] = ny_mfma(yf[0].w, S[lt][r], oe[3]);
                oo[0] = ny_mfma(yf[1].x, S[lt + 1][r], oo[0]); oo[1] = ny_mfma(yf[1].y, S[lt + 1][r], oo[1]);
                oo[2] = ny_mfma(yf[1].z, S[lt + 1][r], oo[2]); oo[3] = ny_mfma(yf[1].w, S[lt + 1][r], oo[3]);
                yf[0] = yg[0]; yf[1] = yg[1];
                __builtin_amdgcn_sched_barrier(0);
            }
        f32x4_t o[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[dt][r] = moc_fdiv(oe[dt][r] + oo[dt][r], den);
        if (a.conv_w) {
            // + v^T T: step st, slot g = token tok0 - 16 + 4 st + g (zero outside the sequence)
#pragma unroll
            for (int st = 0; st < 12; ++st) {
                const int64_t tp = tok0 - 16 + 4 * st + g;
                const bool in = tp >= 0 && tp < a.n_pad;
                float4 v4 = ny_ld4(a.qkv + (in ? tp : tok0) * NY_ROW + 1024 + 64 * h + 4 * c);
                if (!in) v4 = float4{0.f, 0.f, 0.f, 0.f};
                const float b = wt[32 + (4 * st + g - 16) - c];
                o[0] = ny_mfma(v4.x, b, o[0]); o[1] = ny_mfma(v4.y, b, o[1]);
                o[2] = ny_mfma(v4.z, b, o[2]); o[3] = ny_mfma(v4.w, b, o[3]);
            }
        }
        float* op = a.out + (tok0 + c) * NY_OUT + 64 * h + 16 * g;
#pragma unroll
        for (int r = 0; r < 4; ++r) *reinterpret_cast<float4*>(op + 4 * r) = float4{o[0][r], o[1][r], o[2][r], o[3][r]};
    }
}

// both landmark-side entries: `lse` is null for the one that keeps no statistics
int ny_landmark_values(const char* fn, const float* qkv, int64_t n_pad, int heads, int dim_head, int landmarks, const float* q_l,
                       float* W, float* lse, bool want_lse, void* ws, size_t ws_bytes, moc_stream_t stream) {
    MOC_REQUIRE(qkv, "%s: qkv is null", fn);
    MOC_REQUIRE(q_l, "%s: q_l is null", fn);
    MOC_REQUIRE(W, "%s: W is null", fn);
    MOC_REQUIRE(lse || !want_lse, "%s: lse is null", fn);
    MOC_REQUIRE(ws, "%s: ws is null", fn);
    if (const int rc = ny_check_shape(fn, n_pad, heads, dim_head, landmarks)) return rc;
    MOC_REQUIRE(ny_aligned(qkv) && ny_aligned(q_l) && ny_aligned(W) && ny_aligned(ws),
                "%s: qkv, q_l, W and ws must be 16-byte aligned", fn);
    MOC_REQUIRE(ny_aligned(lse), "%s: lse must be 16-byte aligned", fn);
    MOC_REQUIRE(ws_bytes >= ny_ws_bytes(n_pad), "%s: ws_bytes=%zu, need %zu", fn, ws_bytes, ny_ws_bytes(n_pad));
    hipStream_t s = (hipStream_t)stream;
    NyAArgs a;
    a.qkv = qkv; a.q_l = q_l; a.part = (float*)ws; a.n_pad = n_pad; a.chunks = (int)ny_chunks(n_pad);
    nystrom_landmark_kernel<<<dim3(a.chunks, NY_HEADS), NY_A_THREADS, 0, s>>>(a);
    MOC_CHECK_LAUNCH(fn);
    nystrom_merge_kernel<<<NY_HEADS * NY_M * (NY_D / 4) / 256, 256, 0, s>>>((const float*)ws, a.chunks, W, lse);
    MOC_CHECK_LAUNCH(fn);
    return MOC_OK;
}

}  // namespace

extern "C" size_t moc_nystrom_workspace(int64_t n_pad, int heads, int dim_head, int landmarks) {
    return ny_shape_ok(n_pad, heads, dim_head, landmarks) ? ny_ws_bytes(n_pad) : 0;
}

extern "C" int moc_nystrom_landmark_values(const float* qkv, int64_t n_pad, int heads, int dim_head, int landmarks,
                                           const float* q_l, float* W, void* ws, size_t ws_bytes, moc_stream_t stream) {
    return ny_landmark_values("moc_nystrom_landmark_values", qkv, n_pad, heads, dim_head, landmarks, q_l, W, nullptr, false, ws,
                              ws_bytes, stream);
}

extern "C" int moc_nystrom_landmark_values_lse(const float* qkv, int64_t n_pad, int heads, int dim_head, int landmarks,
                                               const float* q_l, float* W, float* lse, void* ws, size_t ws_bytes,
                                               moc_stream_t stream) {
    return ny_landmark_values("moc_nystrom_landmark_values_lse", qkv, n_pad, heads, dim_head, landmarks, q_l, W, lse, true, ws,
                              ws_bytes, stream);
}

extern "C" int moc_nystrom_token_values(const float* qkv, int64_t n_pad, int heads, int dim_head, int landmarks,
                                        const float* k_l, const float* Y, const float* conv_w, int taps, float scale,
                                        float* out, moc_stream_t stream) {
    MOC_REQUIRE(qkv, "moc_nystrom_token_values: qkv is null");
    MOC_REQUIRE(k_l, "moc_nystrom_token_values: k_l is null");
    MOC_REQUIRE(Y, "moc_nystrom_token_values: Y is null");
    MOC_REQUIRE(out, "moc_nystrom_token_values: out is null");
    if (const int rc = ny_check_shape("moc_nystrom_token_values", n_pad, heads, dim_head, landmarks)) return rc;
    if (conv_w) {
        MOC_REQUIRE(taps >= 1 && (taps & 1), "moc_nystrom_token_values: taps=%d must be odd", taps);
        if (taps > NY_MAX_TAPS) MOC_FAIL(MOC_EUNSUPPORTED, "moc_nystrom_token_values: taps=%d above 33", taps);
    }
    MOC_REQUIRE(std::isfinite(scale), "moc_nystrom_token_values: scale is not finite");
    MOC_REQUIRE(ny_aligned(qkv) && ny_aligned(k_l) && ny_aligned(Y) && ny_aligned(out),
                "moc_nystrom_token_values: qkv, k_l, Y and out must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    NyBArgs a;
    a.qkv = qkv; a.k_l = k_l; a.Y = Y; a.conv_w = conv_w; a.out = out; a.n_pad = n_pad; a.taps = conv_w ? taps : 1; a.scale = scale;
    // (set on every call: cheap, and there is no once-only flag for two threads to race on)
    const hipError_t ea = hipFuncSetAttribute((const void*)nystrom_token_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, NY_B_SMEM);
    if (ea != hipSuccess) MOC_FAIL(MOC_ELAUNCH, "moc_nystrom_token_values: %s", hipGetErrorString(ea));
    nystrom_token_kernel<<<dim3((unsigned)(n_pad / NY_B_TOK), NY_HEADS), 512, NY_B_SMEM, s>>>(a);
    MOC_CHECK_LAUNCH("moc_nystrom_token_values");
    return MOC_OK;
}
