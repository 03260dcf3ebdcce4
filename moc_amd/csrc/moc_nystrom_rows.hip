// Rows of the Nystrom attention matrix, for attention maps (moc_amd/nystrom.py: NystromAttention.forward_rows; DESIGN.md
// section 8c, "Attention rows").  The layer's attention is attn1 pinv attn3 with attn3 = softmax_over_tokens(q_l k^T); a wanted
// row i of it is coef[h, i, :] attn3[h], coef[h, i, :] = softmax_256(scale q[i, h] k_l[h]^T) pinv[h], a 256-vector that torch
// forms.  Kernel A (moc_nystrom.hip) already leaves each landmark's log-sum-exp over the tokens, so attn3's weights need no
// second reduction, and no running maximum either (s - lse <= 0 up to rounding):
//
//   out[h, r, j] = sum_m coef[h, r, m] exp(q_l[h, m] . k[j, h] - lse[h, m])        r < R <= 16, j < n_pad
//
// The shape is kernel B's (moc_nystrom.hip, whose head comment has the operand conventions): a workgroup is one head x 256
// tokens, q_l[h] (64 KiB) lies in LDS in operand order, the scores are computed landmarks x tokens, so that register r of lane
// (g, c) is (landmark 4 g + r of the tile, token c) and, after the exponential, IS the B operand of the second product's step
// r, whose A operand is coef[row l & 15][landmark 4 g + r] (zero for rows >= R).  Each of eight waves takes two 16-token tiles
// and walks them TOGETHER: one pull of a landmark tile's q_l fragments serves both, and the two tiles' chains are
// independent, which is what the f32 MFMA's 40-cycle dependent latency wants.  The weights are used tile by tile as they are
// formed: no [256 x 16] score block is held.  Per token tile 256 score MFMAs and 64 of the second product.  The score chains
// are kernel A's own (even / odd features, the same slots), so s is bit for bit the score lse was formed from: a weight that
// dominates its landmark's sum comes out as exp(0) however large the scores are.  An output is FOUR fp32 chains, landmark
// tile lt going to chain lt & 3 in index order (inside a tile: steps r = 0..3 over slots g, landmark 4 g + r), added pairwise
// at the end: coef has entries of either sign that cancel (sum |coef| is 4 to 5 where sum coef is 1), and one chain of 256
// terms alone carries two thirds of the error the tests allow (DESIGN.md section 8c has the figures).  No workspace, no
// atomics, one launch: the same bits on every call.
#include "moc_nystrom_shared.h"

namespace {

constexpr int NY_R_MAX = 16;                                          // wanted rows per call: one MFMA tile
constexpr int NY_R_SMEM = NY_M * NY_D * 4 + NY_M * 4;                 // q_l image, lse

struct NyRArgs {
    const float* qkv;      // [n_pad, 1536]
    const float* q_l;      // [8, 256, 64], scaled
    const float* lse;      // [8, 256]
    const float* coef;     // [8, R, 256]
    float* out;            // [8, R, n_pad]
    int64_t n_pad;
    int R;
};

__global__ __launch_bounds__(512) void nystrom_rows_kernel(NyRArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4* qimg = reinterpret_cast<float4*>(smem);                   // [landmark tile 16][j 4][lane 64], as kernel B's k_l image
    float4* limg = qimg + NY_M * NY_D / 4;                            // lse[h]: [landmark tile 16][g 4] float4 (r = 0..3)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int h = blockIdx.y;
    const int64_t tok0 = (int64_t)blockIdx.x * NY_B_TOK + wave * 32;  // this wave's two tiles: tok0, tok0 + 16
    // every key load of both tiles is requested first; the LDS fill and the coefficient loads run under them
    float4 kv[2][4];                                                  // B operand: k[token c of tile t][16 g + 4 j ..]
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) kv[t][j] = ny_ld4(a.qkv + (tok0 + 16 * t + c) * NY_ROW + 512 + 64 * h + 16 * g + 4 * j);
    float4 cf[16];                                                    // A operand of step (lt, r): coef[row c][16 lt + 4 g + r]
#pragma unroll
    for (int lt = 0; lt < 16; ++lt)
        cf[lt] = c < a.R ? ny_ld4(a.coef + ((int64_t)h * a.R + c) * NY_M + 16 * lt + 4 * g) : float4{0.f, 0.f, 0.f, 0.f};
    float4 qv[NY_M * NY_D / 4 / 512];                                 // this thread's eight pieces of the q_l image, requested together
#pragma unroll
    for (int i = 0; i < NY_M * NY_D / 4 / 512; ++i) {
        const int idx = threadIdx.x + 512 * i, ln = idx & 63, f = idx >> 6, lt = f >> 2, j = f & 3, cc = ln & 15, gg = ln >> 4;
        qv[i] = ny_ld4(a.q_l + ((int64_t)h * NY_M + lt * 16 + cc) * NY_D + 16 * gg + 4 * j);
    }
    if (threadIdx.x < NY_M / 4) limg[threadIdx.x] = ny_ld4(a.lse + h * NY_M + 4 * threadIdx.x);
#pragma unroll
    for (int i = 0; i < NY_M * NY_D / 4 / 512; ++i) qimg[threadIdx.x + 512 * i] = qv[i];
    __syncthreads();
    float k[2][16];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) { k[t][4 * j] = kv[t][j].x; k[t][4 * j + 1] = kv[t][j].y; k[t][4 * j + 2] = kv[t][j].z; k[t][4 * j + 3] = kv[t][j].w; }
    const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4_t o[2][4];                                                  // out^T: row 4 g + r', token c of tile t; chain lt & 3
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) o[t][ch] = zero4;
    float4 qf[4], qg[4];                                              // this landmark tile's fragments and the next one's
#pragma unroll
    for (int j = 0; j < 4; ++j) qf[j] = qimg[j * 64 + lane];
#pragma unroll
    for (int lt = 0; lt < 16; ++lt) {
        const int ln = lt + 1 < 16 ? lt + 1 : lt;
#pragma unroll
        for (int j = 0; j < 4; ++j) qg[j] = qimg[(ln * 4 + j) * 64 + lane];
        const float4 ls = limg[lt * 4 + g];                           // lse of landmarks 16 lt + 4 g + 0..3
        f32x4_t s0[2] = {zero4, zero4}, s1[2] = {zero4, zero4};       // scores^T: landmark 16 lt + 4 g + r, token c
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                s0[t] = ny_mfma(qf[j].x, k[t][4 * j], s0[t]);
                s1[t] = ny_mfma(qf[j].y, k[t][4 * j + 1], s1[t]);
                s0[t] = ny_mfma(qf[j].z, k[t][4 * j + 2], s0[t]);
                s1[t] = ny_mfma(qf[j].w, k[t][4 * j + 3], s1[t]);
            }
        const float cr[4] = {cf[lt].x, cf[lt].y, cf[lt].z, cf[lt].w}, lr[4] = {ls.x, ls.y, ls.z, ls.w};
        f32x4_t p[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                // exp(s - lse) with the difference's own rounding (half an ulp of lse ~ log n_pad: 2.4e-7 of the weight up to
                // 2,980 tokens, twice that above) put back: d + e = s - lse exactly (two-sum), exp(d + e) = exp(d) (1 + e)
                const float s = s0[t][r] + s1[t][r], d = s - lr[r], b = d - s, e = (s - (d - b)) - (lr[r] + b);
                const float w = expf(d);
                p[t][r] = fmaf(w, e, w);
            }
        // out^T += coef p: step r, slot g = landmark 16 lt + 4 g + r
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int t = 0; t < 2; ++t) o[t][lt & 3] = ny_mfma(cr[r], p[t][r], o[t][lt & 3]);
#pragma unroll
        for (int j = 0; j < 4; ++j) qf[j] = qg[j];
        __builtin_amdgcn_sched_barrier(0);              // keep each step's LDS reads beside the MFMAs they overlap
    }
    const f32x4_t o0 = (o[0][0] + o[0][1]) + (o[0][2] + o[0][3]), o1 = (o[1][0] + o[1][1]) + (o[1][2] + o[1][3]);
    // lanes c = 0..15 of a row write 16 consecutive floats; rows >= R are not written
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 4 * g + r;
        if (row < a.R) {
            float* op = a.out + ((int64_t)h * a.R + row) * a.n_pad + tok0 + c;
            op[0] = o0[r];
            op[16] = o1[r];
        }
    }
}

bool nr_overlap(const void* p, size_t np, const void* q, size_t nq) {
    const uintptr_t x = (uintptr_t)p, y = (uintptr_t)q;
    return x < y + nq && y < x + np;
}

}  // namespace

extern "C" int moc_nystrom_attention_rows(const float* qkv, int64_t n_pad, int heads, int dim_head, int landmarks, const float* q_l,
                                          const float* lse, const float* coef, int R, float* out, moc_stream_t stream) {
    const char* fn = "moc_nystrom_attention_rows";
    MOC_REQUIRE(qkv, "%s: qkv is null", fn);
    MOC_REQUIRE(q_l, "%s: q_l is null", fn);
    MOC_REQUIRE(lse, "%s: lse is null", fn);
    MOC_REQUIRE(coef, "%s: coef is null", fn);
    MOC_REQUIRE(out, "%s: out is null", fn);
    if (const int rc = ny_check_shape(fn, n_pad, heads, dim_head, landmarks)) return rc;
    MOC_REQUIRE(R >= 1 && R <= NY_R_MAX, "%s: R=%d must be 1..%d", fn, R, NY_R_MAX);
    MOC_REQUIRE(ny_aligned(qkv) && ny_aligned(q_l) && ny_aligned(lse) && ny_aligned(coef) && ny_aligned(out),
                "%s: qkv, q_l, lse, coef and out must be 16-byte aligned", fn);
    const size_t out_bytes = (size_t)NY_HEADS * R * n_pad * sizeof(float);
    MOC_REQUIRE(!nr_overlap(out, out_bytes, qkv, (size_t)n_pad * NY_ROW * sizeof(float)) &&
                    !nr_overlap(out, out_bytes, q_l, (size_t)NY_HEADS * NY_M * NY_D * sizeof(float)) &&
                    !nr_overlap(out, out_bytes, lse, (size_t)NY_HEADS * NY_M * sizeof(float)) &&
                    !nr_overlap(out, out_bytes, coef, (size_t)NY_HEADS * R * NY_M * sizeof(float)),
                "%s: out overlaps qkv, q_l, lse or coef", fn);
    NyRArgs a;
    a.qkv = qkv; a.q_l = q_l; a.lse = lse; a.coef = coef; a.out = out; a.n_pad = n_pad; a.R = R;
    // (set on every call: cheap, and there is no once-only flag for two threads to race on)
    const hipError_t ea = hipFuncSetAttribute((const void*)nystrom_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, NY_R_SMEM);
    if (ea != hipSuccess) MOC_FAIL(MOC_ELAUNCH, "%s: %s", fn, hipGetErrorString(ea));
    nystrom_rows_kernel<<<dim3((unsigned)(n_pad / NY_B_TOK), NY_HEADS), 512, NY_R_SMEM, (hipStream_t)stream>>>(a);
    MOC_CHECK_LAUNCH(fn);
    return MOC_OK;
}
