// Backward of the two fused Nystrom products (moc_nystrom.hip; moc_amd/nystrom.py: LandmarkValues, TokenValues; DESIGN.md
// section 8c, "training").  As a flash-attention backward does, the softmax weights are recomputed tile by tile from the
// operands and a per-row statistic; nothing of size n_pad x 256 is written to memory.
//
//   landmark side, per head: S = q_l k^T [256, n], P = exp(S - lse), W = P v.  Given dW:
//       delta[m] = dW[m] . W[m],  dP = dW v^T,  dS = P (dP - delta),  dv = P^T dW,  dk = dS^T q_l,  dq_l = dS k
//   token side, per head: P = softmax_256(scale q k_l^T), out = P Y.  Given dout:
//       dP = dout Y^T,  delta[i] = sum_m P[i, m] dP[i, m],  dS = P (dP - delta),  dq = scale dS k_l,
//       dk_l = dS^T (scale q),  dY = P^T dout
//
// Each side is a token-parallel kernel (its dqkv columns) and a landmark-parallel one (its [8, 256, 64] gradients), on the
// forward's lane conventions (moc_nystrom.hip's header): v_mfma_f32_16x16x4_f32, lane l holds A[l & 15][l >> 4] and
// B[l >> 4][l & 15], the result has its column on c = l & 15 and rows 4 g + r (g = l >> 4) in register r, so that a score
// tile computed transposed IS the B operand of the products that consume it.
//
// Token-parallel (shaped like kernel B): a workgroup is one head x 256 tokens; the two [256, 64] operands (q_l and dW, or
// k_l and Y) lie in LDS row-major with rows of 68 floats, which serves both reads without a second image: as the A operand
// of a score-type product lane (g, c) reads row 16 lt + c, floats 16 g .. 16 g + 15 (16-byte slot c + 4 g + j of the 256-byte
// bank row); as the A operand of a gradient-type product it reads row 16 lt + 4 g + r, floats 4 c .. 4 c + 3 (slot 4 g + r +
// c).  ds_read_b128 serves four groups of sixteen lanes that each mix two values of g, so both reads are two-way on a quarter
// of their slots and free on the rest; an XOR swizzle in place of the padding would free them all and is left undone.
// A wave takes 16-token tiles.  The landmark side knows lse, so a 16-landmark
// tile of P and dS is formed and consumed at once; the token side keeps its 256 weights in registers (one softmax), forms
// delta in a first walk over dP and dS in a second, and leaves (max, 1 / sum, delta) per token in the workspace.
// Landmark-parallel (shaped like kernel A): a workgroup is one head x one 512-token range x one half of the landmarks; its
// four waves own 32 landmarks each, hold their rows of both operands in registers and walk the range 16 tokens at a time;
// each range leaves partial [256, 64] sums in the workspace, which a merge launch adds in index order.  No atomics: two
// calls give the same bits.  Every load is of a token below n_pad (ranges end at n_pad, nothing is read ahead).
// The landmark side's weights exp(S - lse) inherit lse's rounding (half an ulp of a value near log n, several ulps of a
// weight): the landmark-parallel kernel, which runs first, also sums its weights per landmark; the merge divides dq_l by
// that sum Z (dS is linear in the weights) and leaves 1 / Z for the token-parallel kernel to scale its weights with.
#include "moc_nystrom_shared.h"

namespace {

constexpr int NYB_LDW = NY_D + 4;                                        // floats per row of an LDS operand image
constexpr int NYB_IMG = NY_M * NYB_LDW;                                  // floats per image
constexpr int NYB_SMEM = (2 * NYB_IMG + 3 * NY_M) * 4;                   // two images, three [256] statistics: 142,336 bytes
constexpr int NYB_LT = 2;                                                // 16-landmark tiles per wave, landmark-parallel
constexpr int NYB_L_THREADS = 256;                                       // four waves: half the landmarks

// workspace, in floats: the landmark side's delta and 1 / (sum of the recomputed weights), each [8, 256]; the token side's
// (max, 1 / sum, delta), each [8, n_pad]; the ranges' partial sums [2, 8, chunks, 256, 64]; the ranges' weight sums
// [8, chunks, 256]
constexpr int NYB_OFF_RZ = NY_HEADS * NY_M, NYB_OFF_STATS = 2 * NY_HEADS * NY_M;
__host__ __device__ inline size_t nyb_off_part(int64_t n_pad) { return (size_t)NYB_OFF_STATS + (size_t)3 * NY_HEADS * n_pad; }
__host__ __device__ inline size_t nyb_off_zsum(int64_t n_pad, int chunks) {
    return nyb_off_part(n_pad) + (size_t)2 * NY_HEADS * chunks * NY_M * NY_D;
}
size_t nyb_ws_bytes(int64_t n_pad) {
    const int chunks = (int)ny_chunks(n_pad);
    return (nyb_off_zsum(n_pad, chunks) + (size_t)NY_HEADS * chunks * NY_M) * sizeof(float);
}

// exp(s - l) with the rounding of the difference carried along (two-sum): near a row's largest score s - l is about
// -log(sum), a few units, and half an ulp of THAT would be the largest error of the recomputed weight
__device__ __forceinline__ float nyb_exp_diff(float s, float l) {
    const float b = -l, d = s + b, bb = d - s;
    const float err = (s - (d - bb)) + (b - bb);
    const float e = expf(d);
    return e + e * err;
}

__device__ __forceinline__ void nyb_ld16(const float* p, float* o) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 v = ny_ld4(p + 4 * j);
        o[4 * j] = v.x; o[4 * j + 1] = v.y; o[4 * j + 2] = v.z; o[4 * j + 3] = v.w;
    }
}
__device__ __forceinline__ void nyb_st4(float* p, float x, float y, float z, float w) {
    *reinterpret_cast<float4*>(p) = float4{x, y, z, w};
}
// rows [256, 64] of one head into an LDS image, by a whole workgroup of 512 threads
__device__ __forceinline__ void nyb_fill(float* img, const float* src) {
    for (int idx = threadIdx.x; idx < NY_M * NY_D / 4; idx += 512) {
        const int row = idx >> 4, c4 = idx & 15;
        *reinterpret_cast<float4*>(img + row * NYB_LDW + 4 * c4) = ny_ld4(src + row * NY_D + 4 * c4);
    }
}
// one 16 x 16 tile of a score-type product: rows 16 lt + (0..15) of the image against this lane's sixteen floats `b`
// (slot g of step s stands for feature 16 g + s; even and odd features in chains of their own, as in the forward)
__device__ __forceinline__ f32x4_t nyb_score_tile(const float* img, int lt, int c, int g, const float* b) {
    const float* p = img + (lt * 16 + c) * NYB_LDW + 16 * g;
    f32x4_t s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 a = ny_ld4(p + 4 * j);
        s0 = ny_mfma(a.x, b[4 * j], s0);
        s1 = ny_mfma(a.y, b[4 * j + 1], s1);
        s0 = ny_mfma(a.z, b[4 * j + 2], s0);
        s1 = ny_mfma(a.w, b[4 * j + 3], s1);
    }
    return s0 + s1;
}
// acc^T += image^T w^T over the tile's 16 landmarks: step r, slot g = landmark 16 lt + 4 g + r; output tile dt holds, in
// register r' of lane (g, c), feature 16 g + 4 r' + dt of token c
__device__ __forceinline__ void nyb_grad_tile(const float* img, int lt, int c, int g, f32x4_t w, f32x4_t* acc) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float4 a = ny_ld4(img + (lt * 16 + 4 * g + r) * NYB_LDW + 4 * c);
        acc[0] = ny_mfma(a.x, w[r], acc[0]); acc[1] = ny_mfma(a.y, w[r], acc[1]);
        acc[2] = ny_mfma(a.z, w[r], acc[2]); acc[3] = ny_mfma(a.w, w[r], acc[3]);
    }
}

// delta[h, m] = dW[h, m] . W[h, m]: one thread per landmark
__global__ __launch_bounds__(256) void nystrom_bwd_delta_kernel(const float* W, const float* dW, float* delta) {
    const int i = blockIdx.x * 256 + threadIdx.x;                        // < 8 * 256
    float s = 0.f;
    for (int j = 0; j < NY_D / 4; ++j) {
        const float4 a = ny_ld4(W + (int64_t)i * NY_D + 4 * j), b = ny_ld4(dW + (int64_t)i * NY_D + 4 * j);
        s += a.x * b.x; s += a.y * b.y; s += a.z * b.z; s += a.w * b.w;
    }
    delta[i] = s;
}

struct NyBwdArgs {
    const float* qkv;      // [n_pad, 1536]
    const float* m1;       // [8, 256, 64]: q_l (scaled) on the landmark side, k_l on the token side
    const float* m2;       // [8, 256, 64]: dW on the landmark side, Y on the token side
    const float* lse;      // [8, 256], landmark side
    const float* dout;     // [n_pad, 512], token side
    float* dqkv;           // [n_pad, 1536]
    float* ws;
    int64_t n_pad;
    int chunks;
    float scale;
};

// landmark side, token-parallel: dk and dv of one head x 256 tokens, zeros in the q columns
__global__ __launch_bounds__(512) void nystrom_bwd_landmark_tokens_kernel(NyBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* qimg = reinterpret_cast<float*>(smem);
    float* wimg = qimg + NYB_IMG;
    float* slse = wimg + NYB_IMG;
    float* sdel = slse + NY_M;
    float* srz = sdel + NY_M;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int h = blockIdx.y;
    const int64_t tok_base = (int64_t)blockIdx.x * NY_B_TOK;
    nyb_fill(qimg, a.m1 + (int64_t)h * NY_M * NY_D);
    nyb_fill(wimg, a.m2 + (int64_t)h * NY_M * NY_D);
    if (threadIdx.x < NY_M) {
        slse[threadIdx.x] = a.lse[h * NY_M + threadIdx.x];
        sdel[threadIdx.x] = a.ws[h * NY_M + threadIdx.x];
        srz[threadIdx.x] = a.ws[NYB_OFF_RZ + h * NY_M + threadIdx.x];
    }
    __syncthreads();
    const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int tile = wave; tile < NY_B_TOK / 16; tile += 8) {
        const int64_t tok0 = tok_base + tile * 16;
        float kb[16], vb[16];                                            // B operands: k, v [token c][16 g + s]
        nyb_ld16(a.qkv + (tok0 + c) * NY_ROW + 512 + 64 * h + 16 * g, kb);
        nyb_ld16(a.qkv + (tok0 + c) * NY_ROW + 1024 + 64 * h + 16 * g, vb);
        f32x4_t dk[4], dv[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) { dk[dt] = zero4; dv[dt] = zero4; }
#pragma unroll 2
        for (int lt = 0; lt < 16; ++lt) {
            const f32x4_t s = nyb_score_tile(qimg, lt, c, g, kb);        // landmark 16 lt + 4 g + r, token c
            const f32x4_t dp = nyb_score_tile(wimg, lt, c, g, vb);
            const float4 l4 = ny_ld4(slse + lt * 16 + 4 * g), d4 = ny_ld4(sdel + lt * 16 + 4 * g), z4 = ny_ld4(srz + lt * 16 + 4 * g);
            const float lr[4] = {l4.x, l4.y, l4.z, l4.w}, dr[4] = {d4.x, d4.y, d4.z, d4.w}, zr[4] = {z4.x, z4.y, z4.z, z4.w};
            f32x4_t p, ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                p[r] = nyb_exp_diff(s[r], lr[r]) * zr[r];
                ds[r] = p[r] * (dp[r] - dr[r]);
            }
            nyb_grad_tile(wimg, lt, c, g, p, dv);
            nyb_grad_tile(qimg, lt, c, g, ds, dk);
        }
        float* op = a.dqkv + (tok0 + c) * NY_ROW + 64 * h + 16 * g;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            nyb_st4(op + 4 * r, 0.f, 0.f, 0.f, 0.f);
            nyb_st4(op + 512 + 4 * r, dk[0][r], dk[1][r], dk[2][r], dk[3][r]);
            nyb_st4(op + 1024 + 4 * r, dv[0][r], dv[1][r], dv[2][r], dv[3][r]);
        }
    }
}

// token side, token-parallel: dq of one head x 256 tokens, zeros in the k and v columns; (max, 1 / sum, delta) per token
__global__ __launch_bounds__(512) void nystrom_bwd_token_tokens_kernel(NyBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* kimg = reinterpret_cast<float*>(smem);
    float* yimg = kimg + NYB_IMG;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int h = blockIdx.y;
    const int64_t tok_base = (int64_t)blockIdx.x * NY_B_TOK;
    nyb_fill(kimg, a.m1 + (int64_t)h * NY_M * NY_D);
    nyb_fill(yimg, a.m2 + (int64_t)h * NY_M * NY_D);
    __syncthreads();
    float* st_m = a.ws + NYB_OFF_STATS + (int64_t)h * a.n_pad;
    float* st_r = st_m + (int64_t)NY_HEADS * a.n_pad;
    float* st_d = st_r + (int64_t)NY_HEADS * a.n_pad;
    const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int tile = wave; tile < NY_B_TOK / 16; tile += 8) {
        const int64_t tok0 = tok_base + tile * 16;
        float qb[16], db[16];                                            // B operands: scale q, dout [token c][16 g + s]
        nyb_ld16(a.qkv + (tok0 + c) * NY_ROW + 64 * h + 16 * g, qb);
        nyb_ld16(a.dout + (tok0 + c) * NY_OUT + 64 * h + 16 * g, db);
#pragma unroll
        for (int j = 0; j < 16; ++j) qb[j] = moc_fmul(qb[j], a.scale);
        f32x4_t S[16];                                                   // landmark 16 lt + 4 g + r, token c
#pragma unroll
        for (int lt = 0; lt < 16; ++lt) {
            S[lt] = nyb_score_tile(kimg, lt, c, g, qb);
            __builtin_amdgcn_sched_barrier(0);          // keep each tile's LDS reads beside the MFMAs that consume them
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
        const float rden = moc_fdiv(1.f, ny_col_sum((ps[0] + ps[1]) + (ps[2] + ps[3])));
        float dl[4] = {0.f, 0.f, 0.f, 0.f};                              // delta: a first walk over dP
#pragma unroll
        for (int lt = 0; lt < 16; ++lt) {
            const f32x4_t dp = nyb_score_tile(yimg, lt, c, g, db);
#pragma unroll
            for (int r = 0; r < 4; ++r) dl[r] += S[lt][r] * dp[r];
            __builtin_amdgcn_sched_barrier(0);
        }
        const float delta = moc_fmul(ny_col_sum((dl[0] + dl[1]) + (dl[2] + dl[3])), rden);
        f32x4_t dq[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dq[dt] = zero4;
#pragma unroll
        for (int lt = 0; lt < 16; ++lt) {                                // dS from a second walk, consumed at once
            const f32x4_t dp = nyb_score_tile(yimg, lt, c, g, db);
            f32x4_t ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) ds[r] = (S[lt][r] * rden) * (dp[r] - delta);
            nyb_grad_tile(kimg, lt, c, g, ds, dq);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (g == 0) { st_m[tok0 + c] = m; st_r[tok0 + c] = rden; st_d[tok0 + c] = delta; }
        float* op = a.dqkv + (tok0 + c) * NY_ROW + 64 * h + 16 * g;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            nyb_st4(op + 4 * r, moc_fmul(dq[0][r], a.scale), moc_fmul(dq[1][r], a.scale), moc_fmul(dq[2][r], a.scale),
                    moc_fmul(dq[3][r], a.scale));
            nyb_st4(op + 512 + 4 * r, 0.f, 0.f, 0.f, 0.f);
            nyb_st4(op + 1024 + 4 * r, 0.f, 0.f, 0.f, 0.f);
        }
    }
}

// landmark-parallel, either side: one head x one 512-token range x 128 landmarks.
//   TOK = false: x1 = k, x2 = v, m1 = q_l, m2 = dW;  P = exp(S - lse[landmark]);  partial 0 += k^T dS   (dq_l)
//   TOK = true:  x1 = scale q, x2 = dout, m1 = k_l, m2 = Y;  P = exp(S - max[token]) / sum[token];
//                partial 0 += (scale q)^T dS (dk_l),  partial 1 += dout^T P (dY)
template <bool TOK>
__global__ __launch_bounds__(NYB_L_THREADS) void nystrom_bwd_landmarks_kernel(NyBwdArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int chunk = blockIdx.x, h = blockIdx.y, lt0 = (blockIdx.z * (NYB_L_THREADS / 64) + wave) * NYB_LT;
    const int64_t t0 = (int64_t)chunk * NY_CHUNK;
    const int64_t t1 = t0 + NY_CHUNK < a.n_pad ? t0 + NY_CHUNK : a.n_pad;
    float b1[NYB_LT][16], b2[NYB_LT][16];                                // B operands: m1, m2 [landmark c of tile lt][16 g + s]
    float lse_c[NYB_LT], del_c[NYB_LT];
#pragma unroll
    for (int lt = 0; lt < NYB_LT; ++lt) {
        const int64_t lm = (int64_t)h * NY_M + (lt0 + lt) * 16 + c;
        nyb_ld16(a.m1 + lm * NY_D + 16 * g, b1[lt]);
        nyb_ld16(a.m2 + lm * NY_D + 16 * g, b2[lt]);
        lse_c[lt] = TOK ? 0.f : a.lse[lm];
        del_c[lt] = TOK ? 0.f : a.ws[lm];
    }
    const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4_t acc1[NYB_LT][4], acc2[NYB_LT][4];
    float zs[NYB_LT] = {0.f, 0.f};                                       // this lane's share of its landmarks' weight sums
#pragma unroll
    for (int lt = 0; lt < NYB_LT; ++lt)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) { acc1[lt][dt] = zero4; acc2[lt][dt] = zero4; }
    const float* x1p = a.qkv + (TOK ? 0 : 512) + 64 * h;
    const float* x2p = TOK ? a.dout + 64 * h : a.qkv + 1024 + 64 * h;
    const int x2row = TOK ? NY_OUT : NY_ROW;
    const float* st_m = a.ws + NYB_OFF_STATS + (int64_t)h * a.n_pad;
    const float* st_r = st_m + (int64_t)NY_HEADS * a.n_pad;
    const float* st_d = st_r + (int64_t)NY_HEADS * a.n_pad;
#pragma unroll 1
    for (int64_t t = t0; t < t1; t += 16) {
        float x1[16], x2[16];                                            // A operands of the scores: [token c][16 g + s]
        nyb_ld16(x1p + (t + c) * NY_ROW + 16 * g, x1);
        nyb_ld16(x2p + (t + c) * x2row + 16 * g, x2);
        float4 x1t[4], x2t[4];                                           // A operands of the sums: [token 4 g + j][4 c ..]
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            x1t[j] = ny_ld4(x1p + (t + 4 * g + j) * NY_ROW + 4 * c);
            if (TOK) x2t[j] = ny_ld4(x2p + (t + 4 * g + j) * x2row + 4 * c);
        }
        float mr[4] = {0.f, 0.f, 0.f, 0.f}, rr[4] = {1.f, 1.f, 1.f, 1.f}, dr[4] = {0.f, 0.f, 0.f, 0.f};
        if (TOK) {
#pragma unroll
            for (int j = 0; j < 16; ++j) x1[j] = moc_fmul(x1[j], a.scale);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                x1t[j].x = moc_fmul(x1t[j].x, a.scale); x1t[j].y = moc_fmul(x1t[j].y, a.scale);
                x1t[j].z = moc_fmul(x1t[j].z, a.scale); x1t[j].w = moc_fmul(x1t[j].w, a.scale);
            }
            const float4 m4 = ny_ld4(st_m + t + 4 * g), r4 = ny_ld4(st_r + t + 4 * g), d4 = ny_ld4(st_d + t + 4 * g);
            mr[0] = m4.x; mr[1] = m4.y; mr[2] = m4.z; mr[3] = m4.w;
            rr[0] = r4.x; rr[1] = r4.y; rr[2] = r4.z; rr[3] = r4.w;
            dr[0] = d4.x; dr[1] = d4.y; dr[2] = d4.z; dr[3] = d4.w;
        }
        // scores^T and dP^T: token 4 g + r, landmark c of tile lt
        f32x4_t p[NYB_LT], ds[NYB_LT];
#pragma unroll
        for (int lt = 0; lt < NYB_LT; ++lt) {
            f32x4_t s0 = zero4, s1 = zero4, e0 = zero4, e1 = zero4;
#pragma unroll
            for (int s = 0; s < 16; s += 2) {
                s0 = ny_mfma(x1[s], b1[lt][s], s0);
                s1 = ny_mfma(x1[s + 1], b1[lt][s + 1], s1);
                e0 = ny_mfma(x2[s], b2[lt][s], e0);
                e1 = ny_mfma(x2[s + 1], b2[lt][s + 1], e1);
            }
            const f32x4_t sv = s0 + s1, dp = e0 + e1;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                p[lt][r] = TOK ? expf(sv[r] - mr[r]) * rr[r] : nyb_exp_diff(sv[r], lse_c[lt]);
                ds[lt][r] = p[lt][r] * (dp[r] - (TOK ? dr[r] : del_c[lt]));
            }
            if (!TOK) zs[lt] += (p[lt][0] + p[lt][1]) + (p[lt][2] + p[lt][3]);
        }
        // sums over the tile's tokens: step r, slot g = token 4 g + r
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float u[4] = {x1t[r].x, x1t[r].y, x1t[r].z, x1t[r].w};
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int lt = 0; lt < NYB_LT; ++lt) acc1[lt][dt] = ny_mfma(u[dt], ds[lt][r], acc1[lt][dt]);
            if (TOK) {
                const float w[4] = {x2t[r].x, x2t[r].y, x2t[r].z, x2t[r].w};
#pragma unroll
                for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                    for (int lt = 0; lt < NYB_LT; ++lt) acc2[lt][dt] = ny_mfma(w[dt], p[lt][r], acc2[lt][dt]);
            }
        }
    }
    float* part = a.ws + nyb_off_part(a.n_pad);
#pragma unroll
    for (int lt = 0; lt < NYB_LT; ++lt) {
        const int64_t row = ((int64_t)h * a.chunks + chunk) * NY_M + (lt0 + lt) * 16 + c;
        float* p1 = part + row * NY_D + 16 * g;
        if (!TOK) {
            const float z = ny_col_sum(zs[lt]);
            if (g == 0) a.ws[nyb_off_zsum(a.n_pad, a.chunks) + row] = z;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            nyb_st4(p1 + 4 * r, acc1[lt][0][r], acc1[lt][1][r], acc1[lt][2][r], acc1[lt][3][r]);
            if (TOK)
                nyb_st4(p1 + (int64_t)NY_HEADS * a.chunks * NY_M * NY_D + 4 * r, acc2[lt][0][r], acc2[lt][1][r], acc2[lt][2][r],
                        acc2[lt][3][r]);
        }
    }
}

// one thread per (output, head, landmark, four features): the ranges' partial sums in index order.  With `zsum` (the
// landmark side) the sums are divided by the landmark's summed weights Z, which also leaves 1 / Z in `rz` for the
// token-parallel kernel: the weights exp(S - lse) sum to 1 only as far as lse's own rounding allows, and dS is linear in them
__global__ __launch_bounds__(256) void nystrom_bwd_merge_kernel(const float* part, int chunks, float* out0, float* out1,
                                                                const float* zsum, float* rz) {
    const int idx = blockIdx.x * 256 + threadIdx.x;                      // < nout * 8 * 256 * 16
    const int d4 = idx & 15, lm = (idx >> 4) & (NY_M - 1), h = (idx >> 12) & (NY_HEADS - 1), o = idx >> 15;
    float4 s = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < chunks; ++k) {
        const float4 v = ny_ld4(part + ((((int64_t)o * NY_HEADS + h) * chunks + k) * NY_M + lm) * NY_D + 4 * d4);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    if (zsum) {
        float z = 0.f;
        for (int k = 0; k < chunks; ++k) z += zsum[((int64_t)h * chunks + k) * NY_M + lm];
        s.x /= z; s.y /= z; s.z /= z; s.w /= z;
        if (d4 == 0) rz[h * NY_M + lm] = 1.f / z;
    }
    *reinterpret_cast<float4*>((o ? out1 : out0) + ((int64_t)h * NY_M + lm) * NY_D + 4 * d4) = s;
}

template <typename K>
int nyb_big_lds(K kernel, const char* fn) {
    // (set on every call: cheap, and there is no once-only flag for two threads to race on)
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, NYB_SMEM);
    if (e != hipSuccess) MOC_FAIL(MOC_ELAUNCH, "%s: %s", fn, hipGetErrorString(e));
    return MOC_OK;
}

}  // namespace

extern "C" size_t moc_nystrom_backward_workspace(int64_t n_pad, int heads, int dim_head, int landmarks) {
    return ny_shape_ok(n_pad, heads, dim_head, landmarks) ? nyb_ws_bytes(n_pad) : 0;
}

extern "C" int moc_nystrom_landmark_backward(const float* qkv, int64_t n_pad, int heads, int dim_head, int landmarks,
                                             const float* q_l, const float* W, const float* lse, const float* dW, float* dqkv,
                                             float* dq_l, void* ws, size_t ws_bytes, moc_stream_t stream) {
    const char* fn = "moc_nystrom_landmark_backward";
    MOC_REQUIRE(qkv && q_l && W && lse && dW, "%s: a null input (qkv, q_l, W, lse, dW)", fn);
    MOC_REQUIRE(dqkv && dq_l, "%s: a null output (dqkv, dq_l)", fn);
    MOC_REQUIRE(ws, "%s: ws is null", fn);
    if (const int rc = ny_check_shape(fn, n_pad, heads, dim_head, landmarks)) return rc;
    MOC_REQUIRE(ny_aligned(qkv) && ny_aligned(q_l) && ny_aligned(W) && ny_aligned(lse) && ny_aligned(dW) && ny_aligned(dqkv) &&
                    ny_aligned(dq_l) && ny_aligned(ws),
                "%s: every pointer must be 16-byte aligned", fn);
    MOC_REQUIRE(ws_bytes >= nyb_ws_bytes(n_pad), "%s: ws_bytes=%zu, need %zu", fn, ws_bytes, nyb_ws_bytes(n_pad));
    hipStream_t s = (hipStream_t)stream;
    NyBwdArgs a;
    a.qkv = qkv; a.m1 = q_l; a.m2 = dW; a.lse = lse; a.dout = nullptr; a.dqkv = dqkv; a.ws = (float*)ws; a.n_pad = n_pad;
    a.chunks = (int)ny_chunks(n_pad); a.scale = 1.f;
    if (const int rc = nyb_big_lds(nystrom_bwd_landmark_tokens_kernel, fn)) return rc;
    nystrom_bwd_delta_kernel<<<NY_HEADS * NY_M / 256, 256, 0, s>>>(W, dW, a.ws);
    MOC_CHECK_LAUNCH(fn);
    nystrom_bwd_landmarks_kernel<false><<<dim3(a.chunks, NY_HEADS, 2), NYB_L_THREADS, 0, s>>>(a);
    MOC_CHECK_LAUNCH(fn);
    nystrom_bwd_merge_kernel<<<NY_HEADS * NY_M * (NY_D / 4) / 256, 256, 0, s>>>(
        a.ws + nyb_off_part(n_pad), a.chunks, dq_l, dq_l, a.ws + nyb_off_zsum(n_pad, a.chunks), a.ws + NYB_OFF_RZ);
    MOC_CHECK_LAUNCH(fn);
    nystrom_bwd_landmark_tokens_kernel<<<dim3((unsigned)(n_pad / NY_B_TOK), NY_HEADS), 512, NYB_SMEM, s>>>(a);   // reads 1 / Z
    MOC_CHECK_LAUNCH(fn);
    return MOC_OK;
}

extern "C" int moc_nystrom_token_backward(const float* qkv, int64_t n_pad, int heads, int dim_head, int landmarks,
                                          const float* k_l, const float* Y, float scale, const float* dout, float* dqkv,
                                          float* dk_l, float* dY, void* ws, size_t ws_bytes, moc_stream_t stream) {
    const char* fn = "moc_nystrom_token_backward";
    MOC_REQUIRE(qkv && k_l && Y && dout, "%s: a null input (qkv, k_l, Y, dout)", fn);
    MOC_REQUIRE(dqkv && dk_l && dY, "%s: a null output (dqkv, dk_l, dY)", fn);
    MOC_REQUIRE(ws, "%s: ws is null", fn);
    if (const int rc = ny_check_shape(fn, n_pad, heads, dim_head, landmarks)) return rc;
    MOC_REQUIRE(std::isfinite(scale), "%s: scale is not finite", fn);
    MOC_REQUIRE(ny_aligned(qkv) && ny_aligned(k_l) && ny_aligned(Y) && ny_aligned(dout) && ny_aligned(dqkv) && ny_aligned(dk_l) &&
                    ny_aligned(dY) && ny_aligned(ws),
                "%s: every pointer must be 16-byte aligned", fn);
    MOC_REQUIRE(ws_bytes >= nyb_ws_bytes(n_pad), "%s: ws_bytes=%zu, need %zu", fn, ws_bytes, nyb_ws_bytes(n_pad));
    hipStream_t s = (hipStream_t)stream;
    NyBwdArgs a;
    a.qkv = qkv; a.m1 = k_l; a.m2 = Y; a.lse = nullptr; a.dout = dout; a.dqkv = dqkv; a.ws = (float*)ws; a.n_pad = n_pad;
    a.chunks = (int)ny_chunks(n_pad); a.scale = scale;
    if (const int rc = nyb_big_lds(nystrom_bwd_token_tokens_kernel, fn)) return rc;
    nystrom_bwd_token_tokens_kernel<<<dim3((unsigned)(n_pad / NY_B_TOK), NY_HEADS), 512, NYB_SMEM, s>>>(a);
    MOC_CHECK_LAUNCH(fn);
    nystrom_bwd_landmarks_kernel<true><<<dim3(a.chunks, NY_HEADS, 2), NYB_L_THREADS, 0, s>>>(a);
    MOC_CHECK_LAUNCH(fn);
    nystrom_bwd_merge_kernel<<<2 * NY_HEADS * NY_M * (NY_D / 4) / 256, 256, 0, s>>>(a.ws + nyb_off_part(n_pad), a.chunks, dk_l, dY,
                                                                                       nullptr, nullptr);
    MOC_CHECK_LAUNCH(fn);
    return MOC_OK;
}
