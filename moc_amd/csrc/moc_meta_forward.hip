// Phase B, the forward: the meta-learner ("senet") over the selected rows (or, dense, over every row) and the gated mix.
// The step that follows it in training -- pooling, cross entropy, the sparse backward, Adam -- is moc_meta.hip.
//
// Reference semantics:
//   senet ................ main_moc.py:299-312  (Linear D->64, ReLU, Linear 64->4, Sigmoid)
//   gated mix ............ main_moc.py:391-403 (train), :482-492 (eval)
//
// Four kernels give the same bits and differ in what they are fast at: meta_forward_kernel (16 rows per workgroup),
// meta_forward_ksplit_kernel (16 rows, fp32 bags, the columns over four wave groups), meta_forward64_kernel (64 rows) and
// meta_forward128_kernel (128 rows by LDS-DMA: evaluation, and the only one with the dense / models / ensemble / by-slide
// modes).  Host side, at the end of the file: fwd_args fills the argument block, launch_f128 / launch_ksplit own the
// instantiations, one launcher and one extern "C" entry per mode.
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include "moc_meta_internal.h"
#include "moc_scores_plan.h"

using namespace moc_meta_internal;

namespace {

// ------------------------------------------------------------------ forward
struct FwdArgs {
    const unsigned char* X;
    const int64_t* row_off;
    const int64_t* sel_row;
    const int32_t* n_sel;
    const float* cand;
    const float *W1, *b1, *W2, *b2;
    const unsigned char* W1img;     // W1 in MFMA B-operand order (w1_image_store_*, moc_meta_internal.h)
    float *H1, *gates, *mixed;
    int64_t stride;
    int64_t base_host;              // >= 0: first slot of the (single) slide, known to the host
    int D, C, slide0;
    uint32_t use_bits;
    // where the four candidate scores of a selected row come from (main_moc.py:359-366).  0: the materialised `cand`
    // columns (moc_gather_candidates).  1 / 2: straight from the score pass's statistics (full / compact layout) through
    // sel_idx -- MOC_CAND_FROM_STATS: evaluation passes, which then never write or read the [2C+2, S] candidate array
    // (at thirty classes 545 MB written and read back per 202 slides).  Same values, same bits.
    int cand_mode;
    const float* stats;
    const int32_t* sel_idx;
    // tile records for the step kernel (training step of ONE slide, base_host >= 0): tile_on != 0
    TileWs tile;
    int tile_on;
    union {
        int tile_cap;               // tile_cap = ceil(rows of the slide / 16)
        float ens_scale;            // moc_meta_forward_dense_models (no tile records): the softmax's temperature
    };
    int64_t tile_slot0;             // first slot of the slide's region
    // batched runs (round 4; n_runs > 0): ONE launch serves n_runs independent meta-learners, grid.y = run.  Run r works on
    // slide slide0 + r * slide_stride with its own parameters, par_stride floats (W2: w2_stride; operand image: img_stride
    // bytes) behind run 0's; the per-run scalars the host knows come as arrays (kernel arguments, indexed by the run)
    int n_runs, slide_stride;
    int64_t par_stride, w2_stride, img_stride;
    int64_t base_r[MOC_MAX_RUNS], tile_slot0_r[MOC_MAX_RUNS];
    int32_t tile_cap_r[MOC_MAX_RUNS];
    // the slide's selected-row count S when the HOST knows it (moc_batch_t.n_sel_host; -1: load n_sel[b]): arguments -> sel_row
    // -> rows is one dependent round trip less than arguments -> n_sel -> sel_row -> rows.  Runs: S_r[run] (S_host >= 0 says so).
    int S_host;
    int32_t S_r[MOC_MAX_RUNS];
    // the dense forward (moc_meta_forward_dense: every row of a slide, no sel_row gather): first row of each slide in X,
    // or NULL = row_off.  Unread by every other launch.
    union {
        const int64_t* x_off;
        // moc_meta_forward_by_slide (never dense): the model that scores each slide of the batch, device [n_slides]
        const int32_t* model_of_slide;
    };
};

// what a forward workgroup works on: its slide and, with batched runs, its run's tensors (the argument block is not modified)
struct FwdRun {
    int b, S;                      // S: the host-known row count, or -1
    int64_t base, tile_slot0;
    int tile_cap;
    const unsigned char* W1img;
    const float *W2, *b1, *b2;
};
__device__ __forceinline__ FwdRun fwd_run_setup(const FwdArgs& a) {
    FwdRun r;
    r.W1img = a.W1img; r.W2 = a.W2; r.b1 = a.b1; r.b2 = a.b2; r.tile_slot0 = a.tile_slot0; r.tile_cap = a.tile_cap;
    r.S = a.S_host;
    if (a.n_runs > 0) {
        const int run = blockIdx.y;
        if (a.S_host >= 0) r.S = kernarg_at<int32_t>(offsetof(FwdArgs, S_r) + 4 * (size_t)run);
        r.b = a.slide0 + run * a.slide_stride;
        r.base = kernarg_at<int64_t>(offsetof(FwdArgs, base_r) + 8 * (size_t)run);
        r.tile_slot0 = kernarg_at<int64_t>(offsetof(FwdArgs, tile_slot0_r) + 8 * (size_t)run);
        r.tile_cap = kernarg_at<int32_t>(offsetof(FwdArgs, tile_cap_r) + 4 * (size_t)run);
        r.W1img += (int64_t)run * a.img_stride;
        r.W2 += (int64_t)run * a.w2_stride;
        r.b1 += (int64_t)run * a.par_stride;
        r.b2 += (int64_t)run * a.par_stride;
    } else {
        r.b = a.slide0 + blockIdx.y;
        r.base = a.base_host >= 0 ? a.base_host : a.row_off[r.b];
    }
    return r;
}

// the row of a selected slot o in whichever array holds its candidate scores: column k of it is ptr[k * stride]
__device__ __forceinline__ const float* cand_row(const FwdArgs& a, int64_t base, int o) {
    if (a.cand_mode == 0) return a.cand + base + o;
    return a.stats + base + a.sel_idx[base + o];
}
// the two per-row scores s_delta = |top1 - top2| and s_beta = max background logit
__device__ __forceinline__ void cand_row_scores(const FwdArgs& a, const float* cd, float& s2, float& s3) {
    const int C = a.C;
    if (a.cand_mode == 2) { s2 = cd[(int64_t)(C + 2) * a.stride]; s3 = cd[(int64_t)(C + 4) * a.stride]; }
    else if (a.cand_mode == 1) { s2 = cd[(int64_t)(2 * C) * a.stride]; s3 = cd[(int64_t)(2 * C + 2) * a.stride]; }
    else { s2 = cd[(int64_t)(2 * C) * a.stride]; s3 = cd[(int64_t)(2 * C + 1) * a.stride]; }
}
// (m1, 1/den) of the row: only the compact statistics need them (s_sigma is re-formed)
__device__ __forceinline__ void cand_row_norm(const FwdArgs& a, const float* cd, float& m1, float& rden) {
    m1 = 0.f; rden = 0.f;
    if (a.cand_mode == 2) { m1 = cd[(int64_t)a.C * a.stride]; rden = cd[(int64_t)(a.C + 1) * a.stride]; }
}
// s_p and s_sigma of class c
__device__ __forceinline__ void cand_class_scores(const FwdArgs& a, const float* cd, int c, float m1, float rden, float& s0, float& s1) {
    s0 = cd[(int64_t)c * a.stride];
    if (a.cand_mode == 2) s1 = moc_softmax_from(s0, m1, rden);
    else s1 = cd[(int64_t)(a.C + c) * a.stride];
}

__global__ __launch_bounds__(256) void w1_image_kernel(const float* W1, int D, unsigned char* img, int dt, int64_t par_stride = 0,
                                                       int64_t img_stride = 0) {
    const int e = blockIdx.x * 256 + threadIdx.x;       // grid = (H*D/256, runs)
    const int h = e / D, d = e - h * D;
    w1_image_store(dt, img + (int64_t)blockIdx.y * img_stride, D, h, d, W1[(int64_t)blockIdx.y * par_stride + e]);
}

// ---- fp32 bags on the bf16 matrix cores ------------------------------------------------------------------------------
// fp32 has no fast matrix path on gfx950 (v_mfma_f32_16x16x4_f32: 32 cycles per 16x16x4, 1/16 of the bf16 rate).  So a
// row value x and a weight w are each held as three bf16 terms -- x == x0 + x1 + x2 exactly (the truncating split below:
// 8 + 8 + 8 significant bits), w == w0 + w1 + w2 exactly (moc_split3<false>, the W1 image) -- and the six products
// x_i w_j with i + j <= 2, each exact in fp32, go through v_mfma_f32_16x16x32_bf16 (16 cycles per 16x16x32).  The three
// dropped products are below 2^-16 of the leading one (2^-24 relative to x w, the size of one fp32 rounding).
// The split of four fp32 values into three bf16 terms each, packed two per dword in operand order (element 0 low):
// x0 = x with the low 16 bits cleared, r = x - x0 (exact), x1 = r truncated the same way, x2 = r - x1 (exact, <= 8 bits).
// v_perm_b32 selector 0x07060302: the upper halves of (odd, even) side by side.
__device__ __forceinline__ void fwd_split4(const uint4& v, uint2 (&o)[3]) {
    const unsigned e[4] = {v.x, v.y, v.z, v.w};
    unsigned m[4], l[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float r = moc_fsub(__uint_as_float(e[i]), __uint_as_float(e[i] & 0xFFFF0000u));
        m[i] = __float_as_uint(r);
        l[i] = __float_as_uint(moc_fsub(r, __uint_as_float(m[i] & 0xFFFF0000u)));
    }
    o[0] = make_uint2(__builtin_amdgcn_perm(e[1], e[0], 0x07060302u), __builtin_amdgcn_perm(e[3], e[2], 0x07060302u));
    o[1] = make_uint2(__builtin_amdgcn_perm(m[1], m[0], 0x07060302u), __builtin_amdgcn_perm(m[3], m[2], 0x07060302u));
    o[2] = make_uint2(__builtin_amdgcn_perm(l[1], l[0], 0x07060302u), __builtin_amdgcn_perm(l[3], l[2], 0x07060302u));
}
// eight fp32 values (an A fragment of one k-step of 32 columns, in two 16-byte pieces) -> its three bf16 terms
__device__ __forceinline__ void fwd_split8(const uint4& p0, const uint4& p1, uint4 (&o)[3]) {
    uint2 a[3], b[3];
    fwd_split4(p0, a);
    fwd_split4(p1, b);
#pragma unroll
    for (int t = 0; t < 3; ++t) o[t] = make_uint4(a[t].x, a[t].y, b[t].x, b[t].y);
}
// one k-step of 32 columns: the six products of x's terms (A) and W1's terms (B, the image's hi, mid, lo), smallest first --
// x2 w0, x1 w1, x0 w2, x1 w0, x0 w1, x0 w0 -- into one fp32 accumulator.  Every fp32-bag forward multiplies through this
// routine, k-steps in ascending order: the same bits from each of them.
template <typename W>
__device__ __forceinline__ f32x4_t fwd_mfma6(const uint4 (&x)[3], const W& w0, const W& w1, const W& w2, f32x4_t acc) {
#define MOC_MF6(X, Wt) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, X), __builtin_bit_cast(bf16x8_t, Wt), acc, 0, 0, 0)
    MOC_MF6(x[2], w0); MOC_MF6(x[1], w1); MOC_MF6(x[0], w2);
    MOC_MF6(x[1], w0); MOC_MF6(x[0], w1); MOC_MF6(x[0], w0);
#undef MOC_MF6
    return acc;
}

// fp32 bags: one quarter's chain joins the running sum (first quarter: taken as it is), the chain starts over
__device__ __forceinline__ void fwd_fold_quarter(f32x4_t& tot, f32x4_t& acc, bool first) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        tot[i] = first ? acc[i] : moc_fadd(tot[i], acc[i]);
        acc[i] = 0.f;
    }
}

// grid (ceil(S_bound/16), n): one workgroup = 16 selected rows, wave w = hidden units 16w..16w+15.
// TILES: the tile-record variant (training step over tile records, batched runs); without it the kernel is the round-3 code --
// the extra live values cost this 256-register kernel 4.6 us at thirty classes when they were unconditional
template <bool BF16, bool F16 = false, bool TILES = false>
__global__ __launch_bounds__(256, BF16 ? 1 : 3) void meta_forward_kernel(FwdArgs a) {
    // 16 rows x 1 KiB, chunk-swizzled; fp32 bags: the unit's three bf16 term planes, [3][16 rows][32 chunks]
    __shared__ __attribute__((aligned(16))) uint4 xt[BF16 ? 16 * 64 : 3 * 16 * 32];
    __shared__ float Hs[16][H + 1];
    __shared__ float Gs[16][4];
    __shared__ float W2s[4 * H];
    FwdRun fr;
    if constexpr (TILES) fr = fwd_run_setup(a);
    else {
        fr.b = a.slide0 + blockIdx.y;
        fr.base = a.base_host >= 0 ? a.base_host : a.row_off[fr.b];
        fr.W1img = a.W1img; fr.W2 = a.W2; fr.b1 = a.b1; fr.b2 = a.b2; fr.tile_slot0 = 0; fr.tile_cap = 0;
        fr.S = a.S_host;
    }
    const int b = fr.b;
    const int64_t base = fr.base;
    const int S = fr.S >= 0 ? fr.S : a.n_sel[b];            // (host-known: one dependent load less in front of the rows)
    const int row0 = blockIdx.x * 16;
    if (row0 >= S) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int ESZ = BF16 ? 2 : 4;
    MOC_STAMP(0);
    // Epilogue operands that do not depend on the product are requested first.
    const int C = a.C;
    float pre_c[4] = {0.f, 0.f, 0.f, 0.f};
    if (threadIdx.x < 16 * C && row0 + (threadIdx.x & 15) < S) {
        const int r = threadIdx.x & 15, c = threadIdx.x >> 4;
        const float* cd = cand_row(a, base, row0 + r);
        float m1, rden;
        cand_row_norm(a, cd, m1, rden);
        cand_class_scores(a, cd, c, m1, rden, pre_c[0], pre_c[1]);
        cand_row_scores(a, cd, pre_c[2], pre_c[3]);
    }
    const float w2_pre = fr.W2[threadIdx.x & 255];
    const float bias = fr.b1[wave * 16 + (lane & 15)];
    const float b2_pre = fr.b2[threadIdx.x & 3];
    int64_t rid_e = 0;                                               // tile records: the bag row of this thread's (row, class)
    if constexpr (TILES) { if (a.tile_on) rid_e = a.sel_row[base + min(row0 + (int)(threadIdx.x & 15), S - 1)]; }
    // The 16 x D tile of x goes through LDS once per workgroup: wave w fetches rows 4w..4w+3 with
    // whole-row contiguous loads (UB bytes per row per unit) and stores 16-B chunk c of row r at
    // chunk c ^ (r & 15), so that the A-fragment reads (lane l: row l&15, chunk 4*kk + (l>>4)) hit
    // distinct banks.  W1 comes from its fragment-ordered image: one contiguous 1 KiB per load.
    const int64_t row_bytes = (int64_t)a.D * ESZ;
    const int UB = (row_bytes % 1024 == 0) ? 1024 : 512;          // bytes of a row per unit
    const int U = (int)(row_bytes / UB), cpr = UB / 16;           // units, 16-B chunks per row per unit
    const int ksteps = UB / 64;                                   // MFMA k-steps (bf16: 32 el, f32: 16 el) per unit
    const unsigned char* rp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int sr = min(row0 + wave * 4 + i, S - 1);
        rp[i] = a.X + a.sel_row[base + sr] * row_bytes;
    }
    const int KST = (int)(row_bytes / 64);                        // k-steps over all of D
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    // fp32 bags: the sum over D is formed as ((p0 + p1) + p2) + p3, p_q = the MFMA chain over the q-th quarter of the
    // columns -- the association of meta_forward_ksplit_kernel, which runs the four chains side by side (same bits)
    f32x4_t tot = {0.f, 0.f, 0.f, 0.f};
    const int QS = a.D / 128;                                     // fp32 bags: k-steps of 32 columns per quarter
    int qc = 0, qi = 0;
    for (int u = 0; u < U; ++u) {
        if (u > 0) __syncthreads();                               // every wave is done reading the previous tile
        uint4 xv[4];
        const int xc = lane < cpr ? lane : 0;                     // lanes past the unit re-read chunk 0 (not stored)
#pragma unroll
        for (int i = 0; i < 4; ++i) xv[i] = *reinterpret_cast<const uint4*>(rp[i] + (int64_t)u * UB + xc * 16);
        if constexpr (BF16) {
            // this unit's W1 image: 16 (or 8) k-steps x 3 terms, all requested before the first MFMA
            uint4 wv[16 * 3];
            const uint4* wi = reinterpret_cast<const uint4*>(fr.W1img) + ((size_t)wave * KST + (size_t)u * ksteps) * 3 * 64 + lane;
#pragma unroll
            for (int q = 0; q < 16 * 3; ++q) if (q < ksteps * 3) wv[q] = wi[q * 64];
            if (lane < cpr) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = wave * 4 + i;
                    xt[r * 64 + (lane ^ (r & 15))] = xv[i];
                }
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
                if (kk < ksteps) {
                    const int r = lane & 15;
                    const uint4 A = xt[r * 64 + ((kk * 4 + (lane >> 4)) ^ r)];
#pragma unroll
                    for (int t = 0; t < 3; ++t) acc = moc_mfma_half<F16>(A, wv[kk * 3 + t], acc);
                }
            }
        } else {
            // fp32 bags: the three-term image (8 or 4 k-steps of 32 columns per unit); the fetching wave splits its rows
            // into bf16 terms once (fwd_split4: piece c of a row is half c & 1 of term chunk c >> 1), the six products by
            // fwd_mfma6 -- the sixteen-wave kernel's products in its order
            const int ks32 = UB / 128;
            uint4 wv[8 * 3];
            const uint4* wi = reinterpret_cast<const uint4*>(fr.W1img) + ((size_t)wave * (a.D / 32) + (size_t)u * ks32) * 3 * 64 + lane;
#pragma unroll
            for (int q = 0; q < 8 * 3; ++q) if (q < ks32 * 3) wv[q] = wi[q * 64];
            if (lane < cpr) {
                uint2* xt2 = reinterpret_cast<uint2*>(xt);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = wave * 4 + i;
                    uint2 tv[3];
                    fwd_split4(xv[i], tv);
#pragma unroll
                    for (int p = 0; p < 3; ++p) xt2[((p * 16 + r) * 32 + ((lane >> 1) ^ r)) * 2 + (lane & 1)] = tv[p];
                }
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) {
                if (kk < ks32) {
                    const int r = lane & 15, c = (kk * 4 + (lane >> 4)) ^ r;
                    const uint4 xa[3] = {xt[r * 32 + c], xt[(16 + r) * 32 + c], xt[(32 + r) * 32 + c]};
                    acc = fwd_mfma6(xa, wv[kk * 3], wv[kk * 3 + 1], wv[kk * 3 + 2], acc);
                    if (++qc == QS) {
                        qc = 0;
                        fwd_fold_quarter(tot, acc, qi++ == 0);
                    }
                }
            }
        }
    }
    if constexpr (!BF16) acc = tot;
    MOC_STAMP(1);
    {   // acc[i] = pre-activation of row (lane>>4)*4+i, hidden unit wave*16 + (lane&15)
        const int hcol = wave * 16 + (lane & 15);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float pre = F16 ? acc[i] * (1.f / MOC_F16_W1_SCALE) : acc[i];     // exact power-of-two scaling
            Hs[(lane >> 4) * 4 + i][hcol] = fmaxf(moc_fadd(pre, bias), 0.f);
        }
        W2s[threadIdx.x] = w2_pre;
    }
    __syncthreads();
    if (a.H1) {                          // needed by the backward pass only: evaluation passes NULL
        for (int e = threadIdx.x; e < 16 * H; e += 256) {
            const int r = e >> 6, h = e & 63;
            if (row0 + r < S) a.H1[(base + row0 + r) * H + h] = Hs[r][h];
        }
    }
    if (threadIdx.x < 64) {
        const int r = threadIdx.x >> 2, i = threadIdx.x & 3;
        float z = 0.f;
        for (int h = 0; h < H; ++h) z = fmaf(Hs[r][h], W2s[i * H + h], z);
        z += b2_pre;
        const float g = 1.f / (1.f + expf(-z));
        Gs[r][i] = g;
        if (a.gates && row0 + r < S) a.gates[(base + row0 + r) * 4 + i] = g;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 16 * C; e += 256) {
        const int r = e & 15, c = e >> 4;
        if (row0 + r >= S) continue;
        float s0 = pre_c[0], s1 = pre_c[1], s2 = pre_c[2], s3 = pre_c[3];
        if (e >= 256) {   // C > 16: beyond the prefetched element
            const float* cd = cand_row(a, base, row0 + r);
            float m1, rden;
            cand_row_norm(a, cd, m1, rden);
            cand_class_scores(a, cd, c, m1, rden, s0, s1);
            cand_row_scores(a, cd, s2, s3);
        }
        float v = 0.f;   // 0 + x == x exactly, so this is the reference's running sum in both modes
        if (a.use_bits & 1u) v = moc_fadd(v, moc_fmul(Gs[r][0], s0));
        if (a.use_bits & 2u) v = moc_fadd(v, moc_fmul(Gs[r][1], s1));
        if (a.use_bits & 4u) v = moc_fadd(v, moc_fmul(Gs[r][2], s2));
        if (a.use_bits & 8u) v = moc_fadd(v, moc_fmul(Gs[r][3], s3));
        a.mixed[(int64_t)c * a.stride + base + row0 + r] = v;
    }
    if (TILES && a.tile_on && threadIdx.x < 16 * C) {                // (C <= 16 here: one element per thread)
        const int r = threadIdx.x & 15, c = threadIdx.x >> 4;
        const bool ok = row0 + r < S;
        float v = 0.f;
        if (a.use_bits & 1u) v = moc_fadd(v, moc_fmul(Gs[r][0], pre_c[0]));
        if (a.use_bits & 2u) v = moc_fadd(v, moc_fmul(Gs[r][1], pre_c[1]));
        if (a.use_bits & 4u) v = moc_fadd(v, moc_fmul(Gs[r][2], pre_c[2]));
        if (a.use_bits & 8u) v = moc_fadd(v, moc_fmul(Gs[r][3], pre_c[3]));
        const float4 lam4 = {Gs[r][0], Gs[r][1], Gs[r][2], Gs[r][3]};
        const float4 sc4 = {pre_c[0], pre_c[1], pre_c[2], pre_c[3]};
        tile_emit(a.tile, fr.tile_slot0 / TILE_R + (int64_t)c * fr.tile_cap + blockIdx.x, ok, v, row0 + r, rid_e, lam4, sc4);
    }
    MOC_STAMP(2);
}

// ---- one slide, fp32 bags (the training step of the default storage): the columns split over four wave groups ------
// (round 3, when fp32 products ran on v_mfma_f32_16x16x4_f32) meta_forward_kernel<false> is a chain of D/4 v_mfma_f32_16x16x4_f32 per wave (128 x 32 cycles = 1.7 us at D = 512, with
// three of every four SIMD cycles idle: one wave per SIMD) behind TWO dependent rounds of row loads (2-KiB rows in two
// 1-KiB units, the second requested after the first has been multiplied) -- 5.5 us from kernel start to the last MFMA
// against 3.2 us for bf16 bags (phase stamps, profiles/NOTES.md round 3).  Here a workgroup is 16 waves: wave w holds
// hidden units 16 (w & 3) .. +15 and the (w >> 2)-th QUARTER of the columns, so that the four chains of a hidden tile run
// side by side on the four waves of a SIMD (32 MFMAs each), every row is requested whole at once (wave w fetches row w:
// D / 256 sixteen-byte loads per lane, one wave-uniform row id), and the four partial tiles meet in LDS as
// ((p0 + p1) + p2) + p3 -- the association the 16- and 128-row kernels keep for fp32 bags, hence the same bits.  The products
// run on the bf16 matrix cores (fwd_split4 / fwd_mfma6): per wave D / 128 k-steps x six v_mfma_f32_16x16x32_bf16 (24 x 16
// cycles at D = 512 instead of 32 x 32), the row split once by the wave that fetches it, the tile in LDS as three bf16 planes.
// grid (ceil(S_bound/16), n), 1024 threads; D <= 1024.
constexpr int GATE_STR = H + 4;                             // row stride of the gate chain's operands in LDS (floats; below)
constexpr int FKS_PSTR = H + 4;                             // row stride of a partial tile in LDS (floats)
__host__ __device__ constexpr int fks_lds_bytes(int D) {
    return 3 * 16 * D * 2 + 4 * 16 * FKS_PSTR * 4 + 16 * GATE_STR * 4 + 16 * 4 * 4 + 4 * GATE_STR * 4;
}
// (the score pass's ring form sizes its LDS to leave room for one of these workgroups on its CU: moc_scores_plan.h)
static_assert(fks_lds_bytes(512) == (int)SCORE_RING_BESIDE_LDS, "moc_scores_plan.h restates fks_lds_bytes(512)");
// The gate chain's operands in LDS: the hidden tile Hs [16] and W2 [4], rows of H floats at a stride of GATE_STR = H + 4
// floats -- 17 sixteen-byte slots, so chunk c of row r lies in slot (r + c) mod 16 of the 256-byte bank row.  The one wave
// that forms the 16 x 4 gates (lane = row * 4 + gate) reads a row as sixteen ds_read_b128 at immediate offsets from one
// address: the rows one 16-lane group of such a read touches (four hidden rows, four W2 rows; lanes of one row share an
// address) lie in distinct slots.  The writers keep storing one float per thread.
// z = sum over h, ascending, of fmaf(Hs[r][h], W2[i][h], z) from 0: the chain every forward kernel runs for gate i of row r
// (same order, same bits).  The operands come in groups of 3 + 3 reads through two buffers, a group requested before the
// group ahead of it is consumed: 48 registers (all 32 reads at once would be 128, and 64 already cost the kernel scratch).
template <int N>
__device__ __forceinline__ void gate_load(const float4* hr, const float4* wr, float4 (&hv)[3], float4 (&wv)[3]) {
#pragma unroll
    for (int c = 0; c < N; ++c) { hv[c] = hr[c]; wv[c] = wr[c]; }
}
template <int N>
__device__ __forceinline__ float gate_fma(const float4 (&hv)[3], const float4 (&wv)[3], float z) {
#pragma unroll
    for (int c = 0; c < N; ++c) {
        z = fmaf(hv[c].x, wv[c].x, z);
        z = fmaf(hv[c].y, wv[c].y, z);
        z = fmaf(hv[c].z, wv[c].z, z);
        z = fmaf(hv[c].w, wv[c].w, z);
    }
    return z;
}
__device__ __forceinline__ float gate_chain(const float* Hs, const float* W2s, int r, int i) {
    static_assert(H == 64, "sixteen chunks: five groups of three and one");
    const float4* hr = reinterpret_cast<const float4*>(Hs + r * GATE_STR);
    const float4* wr = reinterpret_cast<const float4*>(W2s + i * GATE_STR);
    float4 ha[3], wa[3], hb[3], wb[3];
    gate_load<3>(hr, wr, ha, wa);
    gate_load<3>(hr + 3, wr + 3, hb, wb);
    float z = gate_fma<3>(ha, wa, 0.f);
    gate_load<3>(hr + 6, wr + 6, ha, wa);
    z = gate_fma<3>(hb, wb, z);
    gate_load<3>(hr + 9, wr + 9, hb, wb);
    z = gate_fma<3>(ha, wa, z);
    gate_load<3>(hr + 12, wr + 12, ha, wa);
    z = gate_fma<3>(hb, wb, z);
    gate_load<1>(hr + 15, wr + 15, hb, wb);
    z = gate_fma<3>(ha, wa, z);
    z = gate_fma<1>(hb, wb, z);
    return z;
}
// DQ = D / 256: every loop over a row's pieces or a quarter's fragments has a compile-time trip count.  STATS: the candidate
// scores come from the score pass's statistics through sel_idx (cand_mode != 0: evaluation of a few slides); the training
// step reads the materialised columns -- no dependent load, no branch between the barrier and the chain.
// Waves per SIMD the kernel is held to (its own sixteen are four): 8 / 6 / 4 / 4 at D = 256 / 512 / 768 / 1024, what hipcc
// gave it unasked before the gate chain read wide -- with only "four" to aim at it spends registers freely there (84-101
// at D = 512, scratch at D >= 768: profiles/NOTES.md) and leaves fewer to whatever shares the compute unit with the forward.
constexpr int fks_waves(int dq) { return dq == 1 ? 8 : dq == 2 ? 6 : 4; }
template <int DQ, bool STATS>
__global__ __launch_bounds__(1024, fks_waves(DQ)) void meta_forward_ksplit_kernel(FwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int D = DQ * 256;
    uint4* xt = reinterpret_cast<uint4*>(smem);                                     // [3 terms][16][D/8] chunks, swizzled
    float* part = reinterpret_cast<float*>(smem + (size_t)3 * 16 * D * 2);          // [4][16][FKS_PSTR]
    float* Hs = part + 4 * 16 * FKS_PSTR;                                           // [16][GATE_STR]
    float4* Gs = reinterpret_cast<float4*>(Hs + 16 * GATE_STR);                     // [16] rows of four gates
    float* W2s = reinterpret_cast<float*>(Gs + 16);                                 // [4][GATE_STR]
    const FwdRun fr = fwd_run_setup(a);
    const int b = fr.b;
    const int64_t base = fr.base;
    const int S = fr.S >= 0 ? fr.S : a.n_sel[b];            // (host-known: one dependent load less in front of the rows)
    const int row0 = blockIdx.x * 16;
    if (row0 >= S) return;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int ht = wave & 3, kq = wave >> 2;
    MOC_STAMP(0);
    MOC_STAMP_MIN(31);                                      // (diagnostic: the first workgroup of the launch to start)
    MOC_STAMP_MAX(32);                                      // (... and the last one to start)
    // this wave's row, whole: the row id is one scalar load, the row D / 256 loads of 1 KiB per wave
    constexpr int64_t row_bytes = (int64_t)D * 4;
    constexpr int cpl = DQ;                                  // 16-byte chunks per lane
    const int sr = min(row0 + wave, S - 1);
    const int64_t rid = a.sel_row[base + sr];
    const unsigned char* rp = a.X + rid * row_bytes + lane * 16;
    MOC_STAMP_DRAIN(3);
    // W1 image of (hidden tile, quarter): D / 128 k-steps x 3 terms, fragments of 1 KiB.  (rid >> 63 is zero: the address is
    // made to depend on the row id so that hipcc cannot hoist these loads above the row id's wait -- they must queue BEHIND
    // the rows.)
    constexpr int QK = D / 128;                              // k-steps of 32 columns per quarter
    const uint4* wi = reinterpret_cast<const uint4*>(fr.W1img) + ((size_t)ht * (D / 32) + (size_t)kq * QK) * 3 * 64 + lane + (rid >> 63);
    // (the rows first: loads return in issue order, and the tile must be in LDS before the first MFMA, while the image
    // fragments -- 192 KiB per workgroup through one CU -- may keep arriving under the chain)
    uint4 xv[cpl];
#pragma unroll
    for (int i = 0; i < cpl; ++i) xv[i] = *reinterpret_cast<const uint4*>(rp + i * 1024);
    uint4 wv[QK * 3];
#pragma unroll
    for (int q = 0; q < QK * 3; ++q) wv[q] = wi[q * 64];
    // the row goes to LDS once, as its three bf16 terms: plane t = [16 rows][D / 8 chunks of 16 bytes], chunk c of row r at
    // c ^ r (r < 16) -- the 16-bit-bag tile's layout, so the A-fragment reads below hit distinct banks.  Piece i of this
    // lane (columns 4 (lane + 64 i) .. +3) is half (lane & 1) of chunk (lane + 64 i) / 2.
    constexpr int cpr = D / 8;                               // chunks per row and term
    uint2* xt2 = reinterpret_cast<uint2*>(smem);
#pragma unroll
    for (int i = 0; i < cpl; ++i) {
        uint2 tv[3];
        fwd_split4(xv[i], tv);
        const int o = (wave * cpr + (((lane + i * 64) >> 1) ^ wave)) * 2 + (lane & 1);
#pragma unroll
        for (int p = 0; p < 3; ++p) xt2[p * 16 * cpr * 2 + o] = tv[p];
    }
    MOC_STAMP(5);
    __syncthreads();
    MOC_STAMP(6);
    // epilogue operands that do not depend on the product: requested now (straight-line code up to the barrier), consumed
    // after the chain
    const int C = a.C;
    float pre_c[4] = {0.f, 0.f, 0.f, 0.f};
    const int er = t & 15, ec = t >> 4;
    const bool e_ok = ec < C && row0 + er < S;
    if constexpr (STATS) {
        if (e_ok) {
            const float* cd = cand_row(a, base, row0 + er);
            float m1, rden;
            cand_row_norm(a, cd, m1, rden);
            cand_class_scores(a, cd, ec, m1, rden, pre_c[0], pre_c[1]);
            cand_row_scores(a, cd, pre_c[2], pre_c[3]);
        }
    } else {                                                 // unconditional (clamped): exact vmcnt counts under the chain
        const float* cd = a.cand + base + min(row0 + er, S - 1);
        const int cc = ec < C ? ec : C - 1;
        pre_c[0] = cd[(int64_t)cc * a.stride];
        pre_c[1] = cd[(int64_t)(C + cc) * a.stride];
        pre_c[2] = cd[(int64_t)(2 * C) * a.stride];
        pre_c[3] = cd[(int64_t)(2 * C + 1) * a.stride];
    }
    const float w2_pre = fr.W2[t & 255];
    const float bias = fr.b1[t & 63];
    const float b2_pre = fr.b2[t & 3];
    int64_t rid_e = 0;                                       // tile records: the bag row of this thread's (row, class)
    if (a.tile_on) rid_e = a.sel_row[base + min(row0 + er, S - 1)];
    __builtin_amdgcn_sched_barrier(0);                       // (hipcc otherwise sinks these requests below the chain)
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    {
        const int r = lane & 15;
        const uint4* xr = xt + r * cpr;
        const int c0 = kq * QK * 4 + (lane >> 4);
#pragma unroll
        for (int kk = 0; kk < QK; ++kk) {
            const int c = (c0 + kk * 4) ^ r;
            const uint4 xa[3] = {xr[c], xr[16 * cpr + c], xr[32 * cpr + c]};
            acc = fwd_mfma6(xa, wv[kk * 3], wv[kk * 3 + 1], wv[kk * 3 + 2], acc);
        }
    }
#ifdef MOC_STAMPS
    asm volatile("v_add_f32 %0, %0, 0" : "+v"(acc[0]));      // the stamp waits for the chain
#endif
    MOC_STAMP(1);
    {   // acc[i] = partial pre-activation of row (lane>>4)*4+i, hidden unit ht*16 + (lane&15), quarter kq
        float* pp = part + (size_t)(kq * 16 + (lane >> 4) * 4) * FKS_PSTR + ht * 16 + (lane & 15);
#pragma unroll
        for (int i = 0; i < 4; ++i) pp[i * FKS_PSTR] = acc[i];
        if (t < 4 * H) W2s[(t >> 6) * GATE_STR + (t & 63)] = w2_pre;
    }
    __syncthreads();
    MOC_STAMP(7);
    {   // thread = (row t >> 6, hidden unit t & 63)
        const int r = t >> 6, h = t & 63;
        const float* pp = part + (size_t)r * FKS_PSTR + h;
        const float pre = moc_fadd(moc_fadd(moc_fadd(pp[0], pp[16 * FKS_PSTR]), pp[32 * FKS_PSTR]), pp[48 * FKS_PSTR]);
        const float hv = fmaxf(moc_fadd(pre, bias), 0.f);
        Hs[r * GATE_STR + h] = hv;
        if (a.H1 && row0 + r < S) a.H1[(base + row0 + r) * H + h] = hv;      // needed by the backward pass only
    }
    __syncthreads();
    MOC_STAMP(8);
    if (t < 64) {
        const int r = t >> 2, i = t & 3;
        float z = gate_chain(Hs, W2s, r, i);
        z += b2_pre;
        const float g = 1.f / (1.f + expf(-z));
        reinterpret_cast<float*>(Gs)[t] = g;
        if (a.gates && row0 + r < S) a.gates[(base + row0 + r) * 4 + i] = g;
    }
    __syncthreads();
    MOC_STAMP(9);
    if (ec < C) {                                            // (uniform over a class's sixteen lanes)
        const float4 lam4 = Gs[er];                          // the row's four gates: one 16-byte read
        float v = 0.f;   // 0 + x == x exactly, so this is the reference's running sum in both modes
        if (a.use_bits & 1u) v = moc_fadd(v, moc_fmul(lam4.x, pre_c[0]));
        if (a.use_bits & 2u) v = moc_fadd(v, moc_fmul(lam4.y, pre_c[1]));
        if (a.use_bits & 4u) v = moc_fadd(v, moc_fmul(lam4.z, pre_c[2]));
        if (a.use_bits & 8u) v = moc_fadd(v, moc_fmul(lam4.w, pre_c[3]));
        if (a.tile_on) {
            // the rank first, then the mixed score and the record: the lane's stores leave back to back
            const int rank = tile_rank16(e_ok, v, row0 + er);
            if (e_ok) a.mixed[(int64_t)ec * a.stride + base + row0 + er] = v;
            const float4 sc4 = {pre_c[0], pre_c[1], pre_c[2], pre_c[3]};
            tile_store(a.tile, fr.tile_slot0 / TILE_R + (int64_t)ec * fr.tile_cap + blockIdx.x, rank, e_ok, v, row0 + er, rid_e, lam4, sc4);
        } else if (e_ok) a.mixed[(int64_t)ec * a.stride + base + row0 + er] = v;
    }
    MOC_STAMP(2);
    MOC_STAMP_MAX(30);                                      // (diagnostic: the last workgroup of the launch to get here)
}

// Many slides at once (evaluation): 30,000 sixteen-row workgroups each re-read the whole 192 KiB W1 image and
// the pass is bound by L2 (5.9 GB at 29 TB/s for 202 slides).  Here a workgroup owns 64 rows (four row tiles):
// every W1 fragment a wave loads feeds four MFMAs, a quarter of the L2 traffic.  Units of 512 bytes of a row
// (8 k-steps: 96 registers of fragments, three workgroups per CU).  Same products in the same order per
// (row, hidden unit) as meta_forward_kernel: bit-identical outputs.  grid (ceil(S_bound/64), n); 16-bit storage.
template <bool F16>
__global__ __launch_bounds__(256) void meta_forward64_kernel(FwdArgs a) {
    __shared__ __attribute__((aligned(16))) uint4 xt[64 * 32];     // 64 rows x 512 B of the current unit, chunk-swizzled
    __shared__ float Hs[64][H + 1];
    __shared__ float Gs[64][4];
    __shared__ float W2s[4 * H];
    const int b = a.slide0 + blockIdx.y;
    const int64_t base = a.row_off[b];
    const int S = a.n_sel[b];
    const int row0 = blockIdx.x * 64;
    if (row0 >= S) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C = a.C;
    // Epilogue operands do not depend on the product: requested first.  Thread -> row tid & 63 (the same row in
    // every round), classes (tid >> 6) + 4 it: the two per-row scores once, the per-class pairs of the first
    // 32 classes here (later chunks of 32 are requested a chunk at a time, all loads before the first store).
    const int er = threadIdx.x & 63, ec0 = threadIdx.x >> 6;
    const bool erow_ok = row0 + er < S;
    const float* ecd = cand_row(a, base, erow_ok ? row0 + er : row0);
    float es2 = 0.f, es3 = 0.f, em1 = 0.f, erd = 0.f, es0[8], es1[8];
    if (erow_ok) {
        cand_row_scores(a, ecd, es2, es3);
        cand_row_norm(a, ecd, em1, erd);
    }
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int c = ec0 + 4 * it;
        es0[it] = es1[it] = 0.f;
        if (erow_ok && c < C) cand_class_scores(a, ecd, c, em1, erd, es0[it], es1[it]);
    }
    const float w2_pre = a.W2[threadIdx.x & 255];
    const float bias = a.b1[wave * 16 + (lane & 15)];
    const float b2_pre = a.b2[threadIdx.x & 3];
    const int64_t row_bytes = (int64_t)a.D * 2;
    const int U = (int)(row_bytes / 512), KST = (int)(row_bytes / 64);
    // wave w fetches rows 16w..16w+15 of the tile: one load = two rows x 512 B (lane l: row 2j + (l >> 5), chunk l & 31)
    const unsigned char* rp[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int sr = min(row0 + wave * 16 + 2 * j + (lane >> 5), S - 1);
        rp[j] = a.X + a.sel_row[base + sr] * row_bytes + (lane & 31) * 16;
    }
    f32x4_t acc[4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) acc[rt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    for (int u = 0; u < U; ++u) {
        if (u > 0) __syncthreads();                               // every wave is done reading the previous unit
        uint4 xv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) xv[j] = *reinterpret_cast<const uint4*>(rp[j] + (int64_t)u * 512);
        uint4 wv[8 * 3];
        const uint4* wi = reinterpret_cast<const uint4*>(a.W1img) + ((size_t)wave * KST + (size_t)u * 8) * 3 * 64 + lane;
#pragma unroll
        for (int q = 0; q < 8 * 3; ++q) wv[q] = wi[q * 64];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int r = wave * 16 + 2 * j + (lane >> 5);
            xt[r * 32 + ((lane & 31) ^ (r & 15))] = xv[j];
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) {
                const int r = rt * 16 + (lane & 15);
                const uint4 A = xt[r * 32 + ((kk * 4 + (lane >> 4)) ^ (r & 15))];
#pragma unroll
                for (int t = 0; t < 3; ++t) acc[rt] = moc_mfma_half<F16>(A, wv[kk * 3 + t], acc[rt]);
            }
        }
    }
    {   // acc[rt][i] = pre-activation of row rt*16 + (lane>>4)*4 + i, hidden unit wave*16 + (lane&15)
        const int hcol = wave * 16 + (lane & 15);
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float pre = F16 ? acc[rt][i] * (1.f / MOC_F16_W1_SCALE) : acc[rt][i];     // exact power-of-two scaling
                Hs[rt * 16 + (lane >> 4) * 4 + i][hcol] = fmaxf(moc_fadd(pre, bias), 0.f);
            }
        W2s[threadIdx.x] = w2_pre;
    }
    __syncthreads();
    if (a.H1) {                          // needed by the backward pass only: evaluation passes NULL
        for (int e = threadIdx.x; e < 64 * H; e += 256) {
            const int r = e >> 6, h = e & 63;
            if (row0 + r < S) a.H1[(base + row0 + r) * H + h] = Hs[r][h];
        }
    }
    {
        const int r = threadIdx.x >> 2, i = threadIdx.x & 3;
        float z = 0.f;
        for (int h = 0; h < H; ++h) z = fmaf(Hs[r][h], W2s[i * H + h], z);
        z += b2_pre;
        const float g = 1.f / (1.f + expf(-z));
        Gs[r][i] = g;
        if (a.gates && row0 + r < S) a.gates[(base + row0 + r) * 4 + i] = g;
    }
    __syncthreads();
    for (int cb = 0; cb < C; cb += 32) {
        if (cb > 0) {
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int c = cb + ec0 + 4 * it;
                if (erow_ok && c < C) cand_class_scores(a, ecd, c, em1, erd, es0[it], es1[it]);
            }
        }
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int c = cb + ec0 + 4 * it;
            if (!erow_ok || c >= C) continue;
            float v = 0.f;   // 0 + x == x exactly, so this is the reference's running sum in both modes
            if (a.use_bits & 1u) v = moc_fadd(v, moc_fmul(Gs[er][0], es0[it]));
            if (a.use_bits & 2u) v = moc_fadd(v, moc_fmul(Gs[er][1], es1[it]));
            if (a.use_bits & 4u) v = moc_fadd(v, moc_fmul(Gs[er][2], es2));
            if (a.use_bits & 8u) v = moc_fadd(v, moc_fmul(Gs[er][3], es3));
            a.mixed[(int64_t)c * a.stride + base + row0 + er] = v;
        }
    }
}

// ---- evaluation forward, 128 rows per workgroup, rows by LDS-DMA -------------------------------------------------
// meta_forward64_kernel re-reads the whole 192 KiB W1 image per 64 rows (3 KiB of image per 1 KiB of row, all of it L2 -> CU
// traffic), its loads, LDS stores, barrier and MFMAs run one after the other, and its mix waits for operands it asks for
// late: 1,000-1,070 us for the 2.0 M selected rows of a 202-slide thirty-class evaluation (1.9 TB/s of rows).  Peeling
// (scripts/bench_forward.py on a first, 256-row form of this kernel: 1,068 us whole, 724 without the mix, 336 with
// nothing but its skeleton) showed where the time is: NOT in the product (340 us of the 1,068) but in what a workgroup
// does alone on its CU before and after it -- the dependent first touches of its prologue and the mix's three round
// trips, 7 us per workgroup with nothing to hide them behind.  So:
//   * 128 rows per workgroup of four waves and 70 KiB of LDS: TWO workgroups per CU, one's prologue and epilogue beside
//     the other's product;
//   * the rows arrive by LDS-DMA (global_load_lds, 16 B per lane, per-lane source address = the gather through sel_row),
//     straight into MFMA A-fragment order -- one instruction = one 16-row x 32-column fragment, 1 KiB -- in chunks of four
//     k-steps (32 KiB), double buffered: chunk c+1 streams in while chunk c is multiplied;
//   * wave w owns hidden units 16 w .. +15 of all 128 rows: eight accumulator tiles, every W1 fragment it loads feeds
//     eight MFMAs (1.5 KiB of image per row instead of 3), the fragments of chunk c+1 requested together with its DMA,
//     so that the only vector-memory wait of the loop is the barrier's;
//   * A fragments are read from LDS by hand-issued ds_read_b128 in batches of four, one batch ahead of the MFMAs that
//     use them (an ordinary LDS read would make hipcc wait vmcnt(0) first: the DMA in flight writes LDS too);
//   * the mix's operands (the row's candidate scores, the first 16 classes) are requested at kernel start, consumed last.
// Same products in the same order per (row, hidden unit) as the 16- and 64-row kernels: bit-identical outputs.
// k-steps (64 bytes of every row) per chunk of the double-buffered row tile, and workgroups per CU.  The kernel is bound by
// dependent latency per tile (row ids -> rows -> product -> gates -> mix), not by bytes or MFMAs, so what pays is MORE
// workgroups per CU: small chunks (8 KiB per k-step) leave LDS and registers for four (16-bit bags: 128 VGPRs) or three
// (fp32 bags: 168; at one k-step per chunk they spill) instead of two with four k-steps per chunk (256 VGPRs).  Same box,
// 202 x 15,000: thirty classes bf16 868 -> 729-737 us, fp32 1,494 -> 1,375-1,396; two classes bf16 108 -> 99, fp32 290 -> 257-265.
constexpr int F128_ROWS = 128;
constexpr int f128_kc(int st) { return st == 2 ? 2 : 1; }
constexpr int f128_wgs(int st) { return st == 2 ? 3 : 4; }
constexpr int f128_buf(int kc) { return (F128_ROWS / 16) * kc * 1024; }       // one chunk of the workgroup's rows
constexpr int f128_xb(int kc) { return 2 * f128_buf(kc) > F128_ROWS * (H + 1) * 4 ? 2 * f128_buf(kc) : F128_ROWS * (H + 1) * 4; }
constexpr int f128_lds(int kc) { return f128_xb(kc) + F128_ROWS * 4 * 4 + 4 * H * 4; }     // + gates + W2: 35.5 KiB
typedef unsigned __attribute__((ext_vector_type(4))) fu32x4_t;
template <int OFF>
__device__ __forceinline__ void fwd_lds16(fu32x4_t& dst, unsigned addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=&v"(dst) : "v"(addr), "n"(OFF) : "memory");
}
__device__ __forceinline__ void fwd_touch4(fu32x4_t (&v)[4]) {
    asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]));
}

// ST: storage of the bag -- 0 bf16, 1 fp16 (three 16-bit terms of W1 per k-step of 32 columns, v_mfma_f32_16x16x32),
// 2 fp32 (the same image; a chunk = two 1-KiB fp32 pieces per row tile = one k-step of 32 columns, split into bf16
// terms as it is read from LDS: fwd_split8, fwd_mfma6)
// DENSE (moc_meta_forward_dense, patch maps): every row of the slide instead of its selected ones -- row i is X row
// x_off[b] + i (row_off[b] + i without x_off), slot row_off[b] + i, its candidate scores the statistics at that slot
// (cand_mode 1 / 2 with the identity in place of sel_idx).  Everything after the row addresses is the same code: a row
// gets the bits it gets when it is selected.
// MODELS (moc_meta_forward_models, prediction with an ensemble): a.n_runs meta-learners over the same tile, one after the
// other -- model m's parameters par_stride floats and its W1 image img_stride bytes behind model 0's, its mixed scores
// C x stride floats behind model 0's.  The prologue (row ids, candidate scores and norms) is paid once per tile; model
// m >= 1 re-streams the tile's rows by LDS-DMA (from L2 / MALL where they still hold them; bytes not yet measured).  Per model
// it is the same code: model m gets the bits it gets alone.  The mode is a flag inside the first template argument
// (F128_MODELS + storage) so that the existing instantiations keep their symbols and their code.
// ENSEMBLE (moc_meta_forward_dense_models, ensemble patch maps; always with MODELS and DENSE): the model loop over every row,
// the models reduced on chip.  Model m's mix goes to LDS ([128][C] over the free row tile, C <= 64), not to HBM; each row's
// softmax(scale * mixed) then updates a Welford mean / M2 per (class, row) kept in the output slots themselves (a.mixed =
// prob_mean, a.H1 = prob_std or NULL; a.gates = gates_mean or NULL, a running sum), by the thread that owns the slot for
// every model, in model order: deterministic.  The last model writes mean, sqrt(M2 / R) and sum / R.  Launch bounds of
// its own: one workgroup per CU fewer than the others (f128_bound), the registers the model loop keeps live.
// BY_SLIDE (moc_meta_forward_by_slide, the evaluation of several runs in one pass; never with MODELS or DENSE): ONE model per
// slide -- a workgroup works on one slide, so its model a.model_of_slide[b] is uniform: one scalar load, clamped into
// 0 .. a.n_runs - 1.  Only the bases differ (the parameters par_stride floats, the W1 image img_stride bytes behind model
// 0's); the outputs are where moc_meta_forward puts them.  Everything after the bases is the same code: a slide of model r
// gets the bits it gets from moc_meta_forward with model r alone.
constexpr int F128_MODELS = 4;
constexpr int F128_ENSEMBLE = 8;
constexpr int F128_BY_SLIDE = 16;
constexpr int F128_ENS_MAX_C = 64;
constexpr int f128_bound(int stm) { return (stm & F128_ENSEMBLE) ? f128_wgs(stm & 3) - 1 : f128_wgs(stm & 3); }
template <int STM, bool DENSE = false>
__global__ __launch_bounds__(256, f128_bound(STM)) void meta_forward128_kernel(FwdArgs a) {
    constexpr int ST = STM & 3;
    constexpr bool MODELS = (STM & F128_MODELS) != 0;
    constexpr bool ENS = (STM & F128_ENSEMBLE) != 0;
    constexpr bool BYS = (STM & F128_BY_SLIDE) != 0;
    static_assert(!ENS || (MODELS && DENSE), "the ensemble mode is a dense models mode");
    static_assert(!BYS || (!MODELS && !DENSE), "a model per slide: the union rows, one model each");
    constexpr int F128_KC = f128_kc(ST), F128_BUF = f128_buf(F128_KC), F128_XB = f128_xb(F128_KC);
    constexpr bool F16 = ST == 1;
    constexpr int WPC = 3 * (ST == 2 ? F128_KC / 2 : F128_KC);      // W1 fragments per chunk (three terms per 32 columns)
    constexpr int ESZ = ST == 2 ? 4 : 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float (*Hs)[H + 1] = reinterpret_cast<float (*)[H + 1]>(smem);          // [128][H + 1]: aliases the chunk buffers, after the loop
    float (*Gs)[4] = reinterpret_cast<float (*)[4]>(smem + F128_XB);         // [128][4]
    float* W2s = reinterpret_cast<float*>(smem + F128_XB + F128_ROWS * 4 * 4);      // [4][H]
    const int b = a.slide0 + blockIdx.y;
    const int64_t base = a.row_off[b];
    const int S = DENSE ? (int)(a.row_off[b + 1] - base) : a.n_sel[b];
    const int row0 = blockIdx.x * F128_ROWS;
    if (row0 >= S) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C = a.C;
#ifdef MOC_FWD_DIAG
    const unsigned diag = a.use_bits >> 8;                 // peeling experiments (scripts/bench_forward.py): 1 no MFMA, 2 no W1 loads, 4 no row DMA, 8 no mix
#else
    constexpr unsigned diag = 0;
#endif
    // ---- the mix's operands: thread -> row tid & 127, classes (tid >> 7) + 2 it.  Requested now, consumed at the end.
    const int er = threadIdx.x & 127, ec0 = threadIdx.x >> 7;
    const bool erow_ok = row0 + er < S;
    const float* ecd = DENSE ? a.stats + base + (erow_ok ? row0 + er : row0) : cand_row(a, base, erow_ok ? row0 + er : row0);
    // (s_p only: s_sigma is re-formed from it with the compact statistics, and loaded at the end otherwise -- the
    // registers of a second array are what the product needs)
    float es2 = 0.f, es3 = 0.f, em1 = 0.f, erd = 0.f, es0[8];
    if (erow_ok) {
        cand_row_scores(a, ecd, es2, es3);
        cand_row_norm(a, ecd, em1, erd);
    }
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int c = ec0 + 2 * it;
        es0[it] = 0.f;
        if (erow_ok && c < C) es0[it] = ecd[(int64_t)c * a.stride];
    }
    float w2_pre = a.W2[threadIdx.x & 255];               // (MODELS: model 0's; the others' at the top of their turn)
    float bias = a.b1[wave * 16 + (lane & 15)];
    float b2_pre = a.b2[threadIdx.x & 3];
    int bys_m = 0;
    if constexpr (BYS) {
        // this slide's model, uniform over the workgroup (one scalar load), clamped: nothing is read outside the arenas.
        // (Statements of this mode alone, not an offset folded into the lines above: a zero offset there changed the
        // register allocation of the existing instantiations.)
        bys_m = min(max(a.model_of_slide[b], 0), a.n_runs - 1);
        const int64_t po = (int64_t)bys_m * a.par_stride;
        w2_pre = a.W2[po + (threadIdx.x & 255)];
        bias = a.b1[po + wave * 16 + (lane & 15)];
        b2_pre = a.b2[po + (threadIdx.x & 3)];
    }
    const int64_t row_bytes = (int64_t)a.D * ESZ;
    const int KK = (int)(row_bytes / 64), nchunk = KK / F128_KC;      // k-steps of 64 bytes of a row
    // this wave fetches row tiles 2 wave, 2 wave + 1 of the workgroup: lane l = row (l & 15), 16-B piece (l >> 4) of a k-step
    const unsigned char* rp[2];
    int64_t xbase = 0;
    if constexpr (DENSE) xbase = a.x_off ? a.x_off[b] : base;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int sr = min(row0 + (wave * 2 + j) * 16 + (lane & 15), S - 1);
        rp[j] = a.X + (DENSE ? xbase + sr : a.sel_row[base + sr]) * row_bytes + (lane >> 4) * 16;
    }
    typedef const __attribute__((address_space(1))) void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    auto issue_x = [&](int c, int buf) {
        unsigned char* dst = smem + buf * F128_BUF;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int kl = 0; kl < F128_KC; ++kl)
                __builtin_amdgcn_global_load_lds((gptr_t)(rp[j] + ((int64_t)c * F128_KC + kl) * 64),
                                                 (lptr_t)(dst + ((wave * 2 + j) * F128_KC + kl) * 1024), 16, 0, 0);
    };
    // model m (MODELS: a backward jump to here, not a loop: the other instantiations keep the code they had before)
    int m = 0;
next_model:
    if (MODELS && m > 0) {                                 // model m's parameters (model 0's were requested above)
        const int64_t po = (int64_t)m * a.par_stride;
        const float *W2m = a.W2, *b1m = a.b1, *b2m = a.b2;
        if constexpr (ENS) asm volatile("" : "+s"(W2m), "+s"(b1m), "+s"(b2m));     // (not hoisted: see below)
        w2_pre = W2m[po + (threadIdx.x & 255)];
        bias = b1m[po + wave * 16 + (lane & 15)];
        b2_pre = b2m[po + (threadIdx.x & 3)];
    }
    int64_t cstride = a.stride;                            // (the class stride of stats and outputs)
    if constexpr (ENS) {
        // what the model loop would otherwise hoist out of it and keep live across the product (the 64-bit addresses of
        // every class of the row, of the rows): recomputed per model
        asm volatile("" : "+s"(cstride), "+v"(rp[0]), "+v"(rp[1]), "+v"(ecd));
    }
    const unsigned char* w1img = MODELS ? a.W1img + (int64_t)m * a.img_stride : a.W1img;
    if constexpr (BYS) w1img += (int64_t)bys_m * a.img_stride;
    float* mixed = MODELS ? a.mixed + (int64_t)m * C * a.stride : a.mixed;
    const fu32x4_t* wimg = reinterpret_cast<const fu32x4_t*>(w1img) + (size_t)wave * (a.D / 32) * 3 * 64 + lane;
    auto load_w = [&](int c, fu32x4_t (&wv)[WPC]) {
#pragma unroll
        for (int q = 0; q < WPC; ++q) wv[q] = wimg[((size_t)c * WPC + q) * 64];
    };
    f32x4_t acc[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) acc[r] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    f32x4_t tot[ST == 2 ? 8 : 1] = {};                     // fp32 bags: running sum of the column quarters (meta_forward_kernel)
    const int qchunks = nchunk / 4;                        // chunks per quarter (D a multiple of 256)
    const unsigned lds0 = (unsigned)(uintptr_t)smem + lane * 16;
    // fp32: lane l's A fragment (columns 8 (l >> 4) .. +7 of the chunk's 32) is pieces 2 ((l >> 4) & 1), +1 of fp32 k-step l >> 5
    const unsigned lds0f = (unsigned)(uintptr_t)smem + (lane >> 5) * 1024 + ((((lane >> 4) & 1) * 32) + (lane & 15)) * 16;
    auto body = [&](int c, const fu32x4_t (&cur)[WPC], fu32x4_t (&nxt)[WPC]) {
        if (c + 1 < nchunk) {                              // chunk c + 1: image fragments and rows, all waited for at the barrier
            if (!(diag & 2u)) load_w(c + 1, nxt);
            if (!(diag & 4u)) issue_x(c + 1, (c + 1) & 1);
        }
        if constexpr (ST == 2) {
            // row tile rt: its two fp32 pieces (two ds_read_b128), split, six MFMAs -- no read-ahead: the registers of a
            // second pair would spill at three workgroups per CU, and the other workgroups' MFMAs cover the LDS latency
            const unsigned buf = lds0f + (c & 1) * F128_BUF;
#pragma unroll
            for (int rt = 0; rt < 8; ++rt) {
                fu32x4_t P[2];
                fwd_lds16<0>(P[0], buf + rt * F128_KC * 1024);
                fwd_lds16<256>(P[1], buf + rt * F128_KC * 1024);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                asm volatile("" : "+v"(P[0]), "+v"(P[1]));
                if (!(diag & 1u)) {
                    uint4 xa[3];
                    fwd_split8(__builtin_bit_cast(uint4, P[0]), __builtin_bit_cast(uint4, P[1]), xa);
                    acc[rt] = fwd_mfma6(xa, cur[0], cur[1], cur[2], acc[rt]);
                }
            }
            if ((c + 1) % qchunks == 0) {                  // ((p0 + p1) + p2) + p3 over the quarters of the columns
                const bool first = c + 1 == qchunks;
#pragma unroll
                for (int r = 0; r < 8; ++r) fwd_fold_quarter(tot[r], acc[r], first);
            }
            __syncthreads();                               // chunk c + 1 has landed for everybody; this buffer is free
            return;
        }
        const unsigned buf = lds0 + (c & 1) * F128_BUF;
        // batches of two A fragments (row tiles 2 g, 2 g + 1 at k-step kl), one batch ahead of the six MFMAs that use them
        fu32x4_t A0[2], A1[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) fwd_lds16<0>(A0[r], buf + (r * F128_KC + 0) * 1024);
#pragma unroll
        for (int st = 0; st < F128_KC * 4; ++st) {         // step = (k-step kl, batch g)
            const int kl = st >> 2, g = st & 3;
            fu32x4_t (&Ac)[2] = (st & 1) ? A1 : A0;
            fu32x4_t (&An)[2] = (st & 1) ? A0 : A1;
            if (st + 1 < F128_KC * 4) {
                const int kl_n = (st + 1) >> 2, g_n = (st + 1) & 3;
#pragma unroll
                for (int r = 0; r < 2; ++r) fwd_lds16<0>(An[r], buf + ((g_n * 2 + r) * F128_KC + kl_n) * 1024);
                asm volatile("s_waitcnt lgkmcnt(2)" ::: "memory");
            } else {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
            asm volatile("" : "+v"(Ac[0]), "+v"(Ac[1]));
            if (!(diag & 1u)) {
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int t = 0; t < 3; ++t) acc[g * 2 + r] = moc_mfma_half<F16>(Ac[r], cur[kl * 3 + t], acc[g * 2 + r]);
            }
        }
        __syncthreads();                                   // chunk c + 1 has landed for everybody; this buffer is free
    };
    fu32x4_t wA[WPC], wB[WPC];
    load_w(0, wA);
    issue_x(0, 0);
    __syncthreads();
    for (int c = 0; c < nchunk; c += 2) {                  // (two chunks per trip: the fragment sets swap roles without copies)
        body(c, wA, wB);
        if (c + 1 < nchunk) body(c + 1, wB, wA);
    }
    {   // acc[r][i] = pre-activation of row r*16 + (lane>>4)*4 + i, hidden unit wave*16 + (lane&15)
        const int hcol = wave * 16 + (lane & 15);
        if constexpr (ST == 2) {
#pragma unroll
            for (int r = 0; r < 8; ++r) acc[r] = tot[r];
        }
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float pre = F16 ? acc[r][i] * (1.f / MOC_F16_W1_SCALE) : acc[r][i];     // exact power-of-two scaling
                Hs[r * 16 + (lane >> 4) * 4 + i][hcol] = fmaxf(moc_fadd(pre, bias), 0.f);
            }
        W2s[threadIdx.x] = w2_pre;
    }
    __syncthreads();
    if (!ENS && a.H1) {                  // needed by the backward pass only: evaluation passes NULL
        for (int e = threadIdx.x; e < F128_ROWS * H; e += 256) {
            const int r = e >> 6, h = e & 63;
            if (row0 + r < S) a.H1[(base + row0 + r) * H + h] = Hs[r][h];
        }
    }
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        const int r = (threadIdx.x >> 2) + rr * 64, i = threadIdx.x & 3;
        float z = 0.f;
        for (int h = 0; h < H; ++h) z = fmaf(Hs[r][h], W2s[i * H + h], z);
        z += b2_pre;
        const float g = 1.f / (1.f + expf(-z));
        Gs[r][i] = g;
        if constexpr (ENS) {                               // the running sum over the models; the mean at the last one
            float* gts = a.gates;
            asm volatile("" : "+s"(gts));                  // (not hoisted out of the model loop)
            if (gts && row0 + r < S) {
                float* gp = gts + (base + row0 + r) * 4 + i;
                const float sg = m > 0 ? *gp + g : g;
                *gp = m + 1 == a.n_runs ? sg / (float)a.n_runs : sg;
            }
        } else {
            if (a.gates && row0 + r < S) a.gates[(base + row0 + r) * 4 + i] = g;
        }
    }
    __syncthreads();
    float* Ms = reinterpret_cast<float*>(smem);            // ENS: [128][C] mixed scores of this model (over the row tile)
    if (erow_ok && !(diag & 8u)) {
        const float g0 = Gs[er][0], g1 = Gs[er][1], g2 = Gs[er][2], g3 = Gs[er][3];
        for (int cb = 0; cb < C; cb += 16) {
            // beyond the 16 classes requested at the start (MODELS: the model before left the last 16 there)
            if (cb > 0 || (MODELS && m > 0 && C > 16)) {
#pragma unroll
                for (int it = 0; it < 8; ++it) {
                    const int c = cb + ec0 + 2 * it;
                    if (c < C) es0[it] = ecd[(int64_t)c * cstride];
                }
            }
            float es1[8];
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int c = cb + ec0 + 2 * it;
                es1[it] = 0.f;
                if (c < C) es1[it] = a.cand_mode == 2 ? moc_softmax_from(es0[it], em1, erd) : ecd[(int64_t)(C + c) * cstride];
            }
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int c = cb + ec0 + 2 * it;
                if (c >= C) continue;
                const float s1 = es1[it];
                float v = 0.f;   // 0 + x == x exactly, so this is the reference's running sum in both modes
                if (a.use_bits & 1u) v = moc_fadd(v, moc_fmul(g0, es0[it]));
                if (a.use_bits & 2u) v = moc_fadd(v, moc_fmul(g1, s1));
                if (a.use_bits & 4u) v = moc_fadd(v, moc_fmul(g2, es2));
                if (a.use_bits & 8u) v = moc_fadd(v, moc_fmul(g3, es3));
                if constexpr (ENS) Ms[er * C + c] = v;
                else mixed[(int64_t)c * cstride + base + row0 + er] = v;
            }
        }
    }
    if constexpr (ENS) {
        __syncthreads();                                   // the tile's mixed scores are in Ms
        if (erow_ok) {
            // softmax(scale * mixed) of row er: both threads of the row form max and sum over all C classes in the same
            // order (the same bits), then each updates its own classes' Welford state in the output slots
            const float* mr = Ms + er * C;
            const float scale = a.ens_scale;
            float mx = -INFINITY, se = 0.f;
            for (int c = 0; c < C; ++c) mx = fmaxf(mx, scale * mr[c]);
            for (int c = 0; c < C; ++c) se += expf(scale * mr[c] - mx);
            float* __restrict__ pmean = a.mixed + base + row0 + er;
            float* __restrict__ pm2 = a.H1 ? a.H1 + base + row0 + er : nullptr;
            const bool last = m + 1 == a.n_runs;
            const float kf = (float)(m + 1);
            for (int cb = 0; cb < C; cb += 16) {
                float mu[8], m2[8];                        // the state of classes cb + ec0 + 2 it, requested together
#pragma unroll
                for (int it = 0; it < 8; ++it) {
                    const int c = cb + ec0 + 2 * it;
                    mu[it] = 0.f;
                    m2[it] = 0.f;
                    if (m > 0 && c < C) {
                        mu[it] = pmean[(int64_t)c * cstride];
                        if (pm2) m2[it] = pm2[(int64_t)c * cstride];
                    }
                }
#pragma unroll
                for (int it = 0; it < 8; ++it) {
                    const int c = cb + ec0 + 2 * it;
                    if (c >= C) continue;
                    const float p = expf(scale * mr[c] - mx) / se;
                    const float d = p - mu[it];
                    const float mu1 = m > 0 ? mu[it] + d / kf : p;      // Welford: model 0 sets, M2 stays 0
                    const float m21 = m > 0 ? m2[it] + d * (p - mu1) : 0.f;
                    pmean[(int64_t)c * cstride] = mu1;
                    if (pm2) pm2[(int64_t)c * cstride] = last ? sqrtf(m21 / (float)a.n_runs) : m21;
                }
            }
        }
        __syncthreads();                                   // Ms read by all: the next model's rows may land over it
    }
    if constexpr (MODELS) {
        if (++m < a.n_runs) goto next_model;
    }
}

// ablation mixes (main_moc.py:538-553): grid (ceil(S_bound/256), n), thread -> selected row
__global__ __launch_bounds__(256) void fixed_mix_kernel(FwdArgs a, int mode) {
    const int b = a.slide0 + blockIdx.y;
    const int64_t base = a.row_off[b];
    const int S = a.n_sel[b], C = a.C;
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    const float* cd = a.cand + base + s;
    const float s2 = cd[(int64_t)(2 * C) * a.stride], s3 = cd[(int64_t)(2 * C + 1) * a.stride];
    for (int c = 0; c < C; ++c) {
        const float s0 = cd[(int64_t)c * a.stride], s1 = cd[(int64_t)(C + c) * a.stride];
        float v;
        if (mode == 0) v = moc_fadd(moc_fadd(moc_fadd(moc_fmul(0.25f, s0), moc_fmul(0.25f, s1)), moc_fmul(0.25f, s2)), moc_fmul(0.25f, s3));
        else if (mode == 1) v = moc_fadd(moc_fadd(moc_fadd(s0, s1), s2), s3);
        else v = fmaxf(fmaxf(s0, s1), fmaxf(s2, s3));
        a.mixed[(int64_t)c * a.stride + base + s] = v;
    }
}

}  // namespace

// ------------------------------------------------------------------ host side
namespace moc_meta_internal {

int check_meta(const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws, const char* who,
               bool need_adam, bool need_grad, bool need_h1) {
    MOC_REQUIRE(M && ws, "%s: null meta/ws", who);
    MOC_REQUIRE(M->H == H, "%s: hidden width %d unsupported (must be %d)", who, M->H, H);
    MOC_REQUIRE(M->D == B->D, "%s: meta D=%d != batch D=%d", who, M->D, B->D);
    MOC_REQUIRE(M->W1 && M->b1 && M->W2 && M->b2, "%s: null parameter", who);
    MOC_REQUIRE((!need_h1 || (ws->H1 && ws->gates)) && ws->mixed && ws->pooled && ws->topk_idx && ws->topk_cnt && ws->loss && ws->pred,
                "%s: null work array", who);
    MOC_REQUIRE(B->sel_row && B->n_sel && B->cand, "%s: batch has no phase-A outputs", who);
    MOC_REQUIRE(!(B->flags & MOC_CAND_FROM_STATS) || !(need_adam || need_grad),
                "%s: a MOC_CAND_FROM_STATS batch has no materialised candidate scores (evaluation only)", who);
    MOC_REQUIRE(B->topk <= 256 && B->C <= 256, "%s: topk/C too large for the fused step (<= 256)", who);
    if (need_adam)
        MOC_REQUIRE(M->m_W1 && M->m_b1 && M->m_W2 && M->m_b2 && M->v_W1 && M->v_b1 && M->v_W2 && M->v_b2,
                    "%s: null Adam state", who);
    if (need_grad) MOC_REQUIRE(M->g_W1 && M->g_b1 && M->g_W2 && M->g_b2, "%s: null gradient output", who);
    if (need_adam || need_grad) MOC_REQUIRE(ws->pair_dh && ws->pair_row && ws->n_pair, "%s: null backward scratch", who);
    return MOC_OK;
}

int launch_w1_images(const moc_batch_t* B, const moc_meta_t* M, const moc_runs_t* R, hipStream_t s) {
    MOC_REQUIRE(M->W1_image, "meta: W1_image buffer is null (moc_w1_image_bytes)");
    w1_image_kernel<<<dim3(H * B->D / 256, R ? R->n_runs : 1), 256, 0, s>>>(M->W1, B->D, (unsigned char*)M->W1_image, B->dtype,
                                                                            R ? R->par_stride : 0, R ? R->image_stride : 0);
    MOC_CHECK_LAUNCH(R ? "moc_w1_image(runs)" : "moc_w1_image");
    return MOC_OK;
}

int s_bound(const moc_batch_t* B) {
    const int64_t by_sel = (int64_t)B->topj * (2 * B->C + 2);
    return (int)(by_sel < B->max_rows ? by_sel : B->max_rows);
}

}  // namespace moc_meta_internal

namespace {

constexpr int F64_SINGLE_ROWS = 16384;   // one slide: the 64-row forward from this many selectable rows on (16-bit bags)

// What every forward launch passes: the batch's arrays, the meta-learner, the first slide, and the candidate source the
// batch's flags name.  The rest is zero (base_host / S_host: -1, not known to the host); a launcher adds its outputs and
// the fields of its mode.
FwdArgs fwd_args(const moc_batch_t* B, const moc_meta_t* M, int slide0, uint32_t use_bits) {
    FwdArgs a = {};
    a.X = (const unsigned char*)B->X; a.row_off = B->row_off; a.sel_row = B->sel_row; a.n_sel = B->n_sel;
    a.cand = B->cand; a.W1 = M->W1; a.b1 = M->b1; a.W2 = M->W2; a.b2 = M->b2;
    a.W1img = (const unsigned char*)M->W1_image;
    a.stride = B->total_rows;
    a.D = B->D; a.C = B->C; a.slide0 = slide0; a.use_bits = use_bits;
    a.base_host = -1;
    a.S_host = -1;
    if (B->flags & MOC_CAND_FROM_STATS) {
        a.cand_mode = (B->flags & MOC_STATS_COMPACT) ? 2 : 1;
        a.stats = B->stats; a.sel_idx = B->sel_idx;
    }
    return a;
}

// The 128-row kernel in one mode (MODE: the F128_* flags, without the storage) for the batch's storage.  The only place
// that names an instantiation of it: a mode's three kernels get their LDS attribute on its first launch.
template <int MODE, bool DENSE>
int launch_f128(const FwdArgs& a, dim3 grid, int dtype, hipStream_t s, const char* who) {
    static std::once_flag attr;                               // (the batched runs launch from pool threads)
    std::call_once(attr, [] {
        (void)hipFuncSetAttribute((const void*)meta_forward128_kernel<MODE + 0, DENSE>, hipFuncAttributeMaxDynamicSharedMemorySize, f128_lds(f128_kc(0)));
        (void)hipFuncSetAttribute((const void*)meta_forward128_kernel<MODE + 1, DENSE>, hipFuncAttributeMaxDynamicSharedMemorySize, f128_lds(f128_kc(1)));
        (void)hipFuncSetAttribute((const void*)meta_forward128_kernel<MODE + 2, DENSE>, hipFuncAttributeMaxDynamicSharedMemorySize, f128_lds(f128_kc(2)));
    });
    if (dtype == MOC_F16) meta_forward128_kernel<MODE + 1, DENSE><<<grid, 256, f128_lds(f128_kc(1)), s>>>(a);
    else if (dtype == MOC_BF16) meta_forward128_kernel<MODE + 0, DENSE><<<grid, 256, f128_lds(f128_kc(0)), s>>>(a);
    else meta_forward128_kernel<MODE + 2, DENSE><<<grid, 256, f128_lds(f128_kc(2)), s>>>(a);
    MOC_CHECK_LAUNCH(who);
    return MOC_OK;
}

// The column-split kernel (fp32 bags, D <= 1024) for the batch's D and candidate source.  The only place that names an
// instantiation of it.  (The runs forward never has cand_mode != 0: check_meta refuses MOC_CAND_FROM_STATS to a training entry.)
int launch_ksplit(const FwdArgs& a, dim3 grid, hipStream_t s, const char* who) {
    static std::once_flag attr;
    std::call_once(attr, [] {
#define MOC_KS_ATTR(DQ)                                                                                                                                  \
    (void)hipFuncSetAttribute((const void*)meta_forward_ksplit_kernel<DQ, false>, hipFuncAttributeMaxDynamicSharedMemorySize, fks_lds_bytes(DQ * 256)); \
    (void)hipFuncSetAttribute((const void*)meta_forward_ksplit_kernel<DQ, true>, hipFuncAttributeMaxDynamicSharedMemorySize, fks_lds_bytes(DQ * 256))
        MOC_KS_ATTR(2); MOC_KS_ATTR(3); MOC_KS_ATTR(4);
#undef MOC_KS_ATTR
    });
    const int lds = fks_lds_bytes(a.D);
#define MOC_KS_LAUNCH(DQ)                                                                        \
    do {                                                                                         \
        if (a.cand_mode) meta_forward_ksplit_kernel<DQ, true><<<grid, 1024, lds, s>>>(a);         \
        else meta_forward_ksplit_kernel<DQ, false><<<grid, 1024, lds, s>>>(a);                    \
    } while (0)
    switch (a.D / 256) {
        case 1: MOC_KS_LAUNCH(1); break;
        case 2: MOC_KS_LAUNCH(2); break;
        case 3: MOC_KS_LAUNCH(3); break;
        default: MOC_KS_LAUNCH(4); break;
    }
#undef MOC_KS_LAUNCH
    MOC_CHECK_LAUNCH(who);
    return MOC_OK;
}

// the dense forwards' grid: the most rows of any slide in [slide0, slide0 + n) -- exact from the host copy of row_off when
// there is one, else the batch's bound
int64_t dense_rows(const moc_batch_t* B, int slide0, int n) {
    if (!B->row_off_host) return B->max_rows;
    int64_t rows = 0;
    for (int q = slide0; q < slide0 + n; ++q) {
        const int64_t nq = B->row_off_host[q + 1] - B->row_off_host[q];
        rows = nq > rows ? nq : rows;
    }
    return rows;
}

}  // namespace

int moc_meta_internal::launch_forward(const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws, int slide0, int n,
                                      uint32_t use_bits, hipStream_t s, bool emit_tiles, const moc_runs_t* runs, int64_t w2_stride,
                                      int S_host) {
    MOC_REQUIRE(!(B->flags & MOC_CAND_FROM_STATS) || (B->stats && B->sel_idx),
                "moc_meta_forward: MOC_CAND_FROM_STATS needs the batch's stats and sel_idx");
    FwdArgs a = fwd_args(B, M, slide0, use_bits);
#ifdef MOC_FWD_DIAG
    if (const char* dg = getenv("MOC_FWD_DIAG")) a.use_bits |= (uint32_t)atoi(dg) << 8;
#endif
    a.H1 = ws->H1; a.gates = ws->gates; a.mixed = ws->mixed;
    if (n == 1 && B->row_off_host) a.base_host = B->row_off_host[slide0];
    if (emit_tiles) {                                      // the caller's plan says the tile-record step follows
        MOC_REQUIRE(n == 1 && B->row_off_host && ws->tile_ws, "moc_meta_forward: tile records need one slide, row_off_host and ws->tile_ws");
        a.tile_on = 1;
        a.tile = tile_carve(ws->tile_ws, tile_slots(B->total_rows, B->n_slides, B->C));
        a.tile_cap = moc_cdiv(B->row_off_host[slide0 + 1] - a.base_host, 16);
        a.tile_slot0 = ((a.base_host >> 4) + slide0) * (int64_t)B->C * TILE_R;
    }
    dim3 grid(moc_cdiv(s_bound(B), 16), n);
    // one slide (a training step) whose S the host knows: S as an argument, and exactly the workgroups that have rows
    // (S_host: the train step's host_n_sel, which its step kernel gets too; callers that do not ask: n_sel_host)
    const bool s_known = n == 1 && B->n_sel_host != nullptr;
    if (S_host < 0 && s_known) S_host = B->n_sel_host[slide0];
    if (n == 1 && !runs && (S_host >= 0 || s_known)) {
        a.S_host = S_host;
        MOC_REQUIRE(a.S_host >= 0 && a.S_host <= s_bound(B), "moc_meta_forward: the host's count of slide %d, %d, is not a row count of this batch (bound %d)",
                    slide0, a.S_host, s_bound(B));
        grid.x = a.S_host > 0 ? moc_cdiv(a.S_host, 16) : 1;
    }
    if (runs) {                                            // one training slide per run, grid.y = run
        MOC_REQUIRE(n == 1 && a.tile_on, "moc_train_steps_runs: the batched forward needs the tile-record step");
        a.n_runs = runs->n_runs; a.slide_stride = runs->slide_stride;
        a.par_stride = runs->par_stride; a.img_stride = runs->image_stride; a.w2_stride = w2_stride;
        int s_max = 0;
        for (int r = 0; r < runs->n_runs; ++r) {
            const int sl = slide0 + r * runs->slide_stride;
            a.base_r[r] = B->row_off_host[sl];
            a.tile_cap_r[r] = moc_cdiv(B->row_off_host[sl + 1] - B->row_off_host[sl], 16);
            a.tile_slot0_r[r] = ((B->row_off_host[sl] >> 4) + sl) * (int64_t)B->C * TILE_R;
            if (s_known) {
                a.S_r[r] = B->n_sel_host[sl];
                MOC_REQUIRE(a.S_r[r] >= 0 && a.S_r[r] <= s_bound(B), "moc_train_steps_runs: n_sel_host[%d] = %d is not a row count of this batch", sl, a.S_r[r]);
                s_max = a.S_r[r] > s_max ? a.S_r[r] : s_max;
            }
        }
        if (s_known) { a.S_host = 0; grid.x = s_max > 0 ? moc_cdiv(s_max, 16) : 1; }
        grid.y = runs->n_runs;
        // fp32 bags: the sixteen-wave kernel is built for the latency of ONE tile per CU; with many runs there are more
        // tiles than the chip holds sixteen-wave workgroups (two per CU), and the four-wave kernel -- the same bits
        // (tests: MOC_FORWARD_FOUR_WAVES) -- packs seven to a CU and keeps the matrix cores fed
        static const int fwd4_env = getenv("MOC_RUNS_FWD4") ? atoi(getenv("MOC_RUNS_FWD4")) : -1;
        const bool four = fwd4_env >= 0 ? fwd4_env != 0 : (int64_t)grid.x * grid.y > 512;
        if (B->dtype == MOC_F32 && four && B->C <= 16) {
            meta_forward_kernel<false, false, true><<<grid, 256, 0, s>>>(a);
            MOC_CHECK_LAUNCH("moc_meta_forward(runs, four waves)");
            return MOC_OK;
        }
        if (B->dtype == MOC_F32) {
            MOC_REQUIRE(B->D <= 1024 && B->C <= 64, "moc_train_steps_runs: fp32 bags need D <= 1024, C <= 64");
            return launch_ksplit(a, grid, s, "moc_meta_forward(runs)");
        }
        if (B->dtype == MOC_F16) meta_forward_kernel<true, true, true><<<grid, 256, 0, s>>>(a);
        else meta_forward_kernel<true, false, true><<<grid, 256, 0, s>>>(a);
        MOC_CHECK_LAUNCH("moc_meta_forward(runs)");
        return MOC_OK;
    }
    static const int fwd_variant = getenv("MOC_FORWARD_EVAL") ? atoi(getenv("MOC_FORWARD_EVAL")) : 128;   // diagnostic: 64 = the 64-row kernel
    if (n >= 4 && (B->D * moc_elem_size(B->dtype)) % 512 == 0 && s_bound(B) >= 1024 && fwd_variant == 128 &&
        !(B->flags & MOC_FORWARD_ROWS64)) {
        // many slides of many selected rows (evaluation): 128 rows per workgroup, rows by LDS-DMA, two workgroups per CU
        return launch_f128<0, false>(a, dim3(moc_cdiv(s_bound(B), F128_ROWS), n), B->dtype, s, "moc_meta_forward(128)");
    }
    // ... or ONE slide of F64_SINGLE_ROWS or more selectable rows (the training forward of the 64-way x 50 k shape: 25,000
    // rows were 1,580 sixteen-row workgroups, each reading the whole 390-KB W1 image: 42.7 us; 8.9 -> 10.1 k meta-steps/s.
    // EBRAINS-30's 7,000 rows are faster sixteen at a time, and the 128-row kernel loses on one slide at either size.)
    const bool one_big = n == 1 && s_bound(B) >= F64_SINGLE_ROWS && !a.tile_on && !(B->flags & MOC_FORWARD_ROWS16);
    if ((n >= 4 || one_big) && B->dtype != MOC_F32 && (B->D * 2) % 512 == 0) {       // many slides at once (evaluation)
        dim3 g64(moc_cdiv(s_bound(B), 64), n);
        if (B->dtype == MOC_F16) meta_forward64_kernel<true><<<g64, 256, 0, s>>>(a);
        else meta_forward64_kernel<false><<<g64, 256, 0, s>>>(a);
        MOC_CHECK_LAUNCH("moc_meta_forward(64)");
        return MOC_OK;
    }
    // fp32 bags: the columns split over four wave groups (same bits as the four-wave kernel)
    if (B->dtype == MOC_F32 && B->D <= 1024 && B->C <= 64 && !(B->flags & MOC_FORWARD_FOUR_WAVES))
        return launch_ksplit(a, grid, s, "moc_meta_forward(ksplit)");
    if (a.tile_on) {
        if (B->dtype == MOC_F16) meta_forward_kernel<true, true, true><<<grid, 256, 0, s>>>(a);
        else if (B->dtype == MOC_BF16) meta_forward_kernel<true, false, true><<<grid, 256, 0, s>>>(a);
        else meta_forward_kernel<false, false, true><<<grid, 256, 0, s>>>(a);
    } else if (B->dtype == MOC_F16) meta_forward_kernel<true, true><<<grid, 256, 0, s>>>(a);
    else if (B->dtype == MOC_BF16) meta_forward_kernel<true><<<grid, 256, 0, s>>>(a);
    else meta_forward_kernel<false><<<grid, 256, 0, s>>>(a);
    MOC_CHECK_LAUNCH("moc_meta_forward");
    return MOC_OK;
}

namespace {

// The four 128-row-only modes.  Each is fwd_args, the mode's fields, launch_f128<MODE, DENSE>; the dense ones take every row's
// candidate scores from the statistics whatever the batch's flag says, and launch nothing for slides without rows.

// moc_meta_forward_dense: every row of slides [slide0, slide0 + n) of an unmasked batch
int launch_forward_dense(const moc_batch_t* B, const moc_meta_t* M, float* gates, float* mixed, int slide0, int n,
                         uint32_t use_bits, hipStream_t s) {
    const int64_t rows = dense_rows(B, slide0, n);
    if (rows <= 0) return MOC_OK;
    FwdArgs a = fwd_args(B, M, slide0, use_bits & 15u);
    a.gates = gates; a.mixed = mixed;
    a.x_off = B->x_off;
    a.cand_mode = (B->flags & MOC_STATS_COMPACT) ? 2 : 1;
    a.stats = B->stats;
    return launch_f128<0, true>(a, dim3(moc_cdiv(rows, F128_ROWS), n), B->dtype, s, "moc_meta_forward_dense");
}

// moc_meta_forward_models: R->n_runs meta-learners over the union rows of slides [slide0, slide0 + n)
int launch_forward_models(const moc_batch_t* B, const moc_meta_t* M, const moc_runs_t* R, float* mixed, int slide0, int n,
                          uint32_t use_bits, hipStream_t s) {
    FwdArgs a = fwd_args(B, M, slide0, use_bits & 15u);
    a.mixed = mixed;
    a.n_runs = R->n_runs; a.par_stride = R->par_stride; a.img_stride = R->image_stride;
    return launch_f128<F128_MODELS, false>(a, dim3(moc_cdiv(s_bound(B), F128_ROWS), n), B->dtype, s, "moc_meta_forward_models");
}

// moc_meta_forward_by_slide: the union rows of slides [slide0, slide0 + n), every slide with the meta-learner model_of_slide
// names for it.  Always this kernel (launch_forward would take the 64-row, 16-row or column-split kernels for few slides or
// few selectable rows; they give the same bits, so only this one has the mode)
int launch_forward_by_slide(const moc_batch_t* B, const moc_meta_t* M, const moc_runs_t* R, const int32_t* model_of_slide,
                            const moc_meta_ws_t* ws, int slide0, int n, uint32_t use_bits, hipStream_t s) {
    FwdArgs a = fwd_args(B, M, slide0, use_bits & 15u);
    a.H1 = ws->H1; a.gates = ws->gates; a.mixed = ws->mixed;
    a.n_runs = R->n_runs; a.par_stride = R->par_stride; a.img_stride = R->image_stride;
    a.model_of_slide = model_of_slide;
    return launch_f128<F128_BY_SLIDE, false>(a, dim3(moc_cdiv(s_bound(B), F128_ROWS), n), B->dtype, s, "moc_meta_forward_by_slide");
}

// moc_meta_forward_dense_models: R->n_runs meta-learners over every row of slides [slide0, slide0 + n), the models reduced on
// chip into prob_mean / prob_std / gates_mean
int launch_forward_dense_models(const moc_batch_t* B, const moc_meta_t* M, const moc_runs_t* R, float scale, float* prob_mean,
                                float* prob_std, float* gates_mean, int slide0, int n, uint32_t use_bits, hipStream_t s) {
    const int64_t rows = dense_rows(B, slide0, n);
    if (rows <= 0) return MOC_OK;
    FwdArgs a = fwd_args(B, M, slide0, use_bits & 15u);
    a.H1 = prob_std; a.gates = gates_mean; a.mixed = prob_mean;
    a.x_off = B->x_off;
    a.cand_mode = (B->flags & MOC_STATS_COMPACT) ? 2 : 1;
    a.stats = B->stats;
    a.n_runs = R->n_runs; a.par_stride = R->par_stride; a.img_stride = R->image_stride;
    a.ens_scale = scale;
    return launch_f128<F128_MODELS + F128_ENSEMBLE, true>(a, dim3(moc_cdiv(rows, F128_ROWS), n), B->dtype, s,
                                                          "moc_meta_forward_dense_models");
}

// ---- argument checks of the entries below, in the order they are made: the meta-learner, [the entry's outputs,] the runs,
// [the entry's own,] the batch.  `who` = the entry, in every message.
int check_fwd_meta(const moc_batch_t* B, const moc_meta_t* M, const char* who, bool images) {
    MOC_REQUIRE(M, "%s: null meta", who);
    MOC_REQUIRE(M->H == H, "%s: hidden width %d unsupported (must be %d)", who, M->H, H);
    MOC_REQUIRE(M->D == B->D, "%s: meta D=%d != batch D=%d", who, M->D, B->D);
    MOC_REQUIRE(M->W1 && M->b1 && M->W2 && M->b2, "%s: null parameter", who);
    if (images) MOC_REQUIRE(M->W1_image, "%s: W1_image buffer is null (n_runs x image_stride bytes)", who);
    return MOC_OK;
}
// stride0_why: why this entry's models all start at slide0
int check_fwd_runs(const moc_batch_t* B, const moc_runs_t* R, const char* who, const char* stride0_why) {
    MOC_REQUIRE(R, "%s: null runs", who);
    MOC_REQUIRE(R->n_runs >= 1 && R->n_runs <= MOC_MAX_RUNS, "%s: n_runs=%d outside 1 .. %d", who, R->n_runs, MOC_MAX_RUNS);
    MOC_REQUIRE(R->slide_stride == 0, "%s: slide_stride=%d must be 0 (%s)", who, R->slide_stride, stride0_why);
    MOC_REQUIRE(R->par_stride >= n_params(B->D), "%s: par_stride=%lld smaller than one meta-learner", who,
                (long long)R->par_stride);
    MOC_REQUIRE(R->image_stride >= (int64_t)moc_w1_image_bytes(B->D, B->dtype), "%s: image_stride=%lld < moc_w1_image_bytes=%lld",
                who, (long long)R->image_stride, (long long)moc_w1_image_bytes(B->D, B->dtype));
    return MOC_OK;
}
// dense: every row (needs the statistics); else the selected rows (needs all of phase A)
int check_fwd_batch(const moc_batch_t* B, const char* who, bool dense, int slide0, int n) {
    if (dense) {
        MOC_REQUIRE(!B->mask, "%s: the batch is masked (slots are not rows); run it unmasked", who);
        MOC_REQUIRE(B->stats, "%s: the batch has no statistics (run the score pass first)", who);
    } else {
        MOC_REQUIRE(!B->mask, "%s: the batch is masked; run it unmasked (an evaluation pass)", who);
        MOC_REQUIRE(B->stats && B->sel_row && B->n_sel && B->sel_idx, "%s: the batch has no phase-A outputs (run moc_phase_a first)", who);
        MOC_REQUIRE((B->flags & MOC_CAND_FROM_STATS) || B->cand, "%s: the batch has no candidate scores", who);
    }
    MOC_REQUIRE(slide0 >= 0 && n >= 1 && slide0 + n <= B->n_slides, "%s: bad slide range", who);
    return MOC_OK;
}

}  // namespace

extern "C" int moc_meta_forward(const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws,
                                int slide0, int n, uint32_t use_bits, moc_stream_t stream) {
    if (int rc = moc_check_batch(B, "moc_meta_forward")) return rc;
    if (int rc = check_meta(B, M, ws, "moc_meta_forward", false, false, false)) return rc;
    MOC_REQUIRE(slide0 >= 0 && n >= 1 && slide0 + n <= B->n_slides, "moc_meta_forward: bad slide range");
    // the parameters may have changed since the image was last written: rebuild it (H*D elements)
    if (int rc = launch_w1_images(B, M, nullptr, (hipStream_t)stream)) return rc;
    return launch_forward(B, M, ws, slide0, n, use_bits, (hipStream_t)stream);
}

extern "C" int moc_meta_forward_dense(const moc_batch_t* B, const moc_meta_t* M, float* gates, float* mixed,
                                      int slide0, int n, uint32_t use_bits, moc_stream_t stream) {
    const char* who = "moc_meta_forward_dense";
    if (int rc = moc_check_batch(B, who)) return rc;
    if (int rc = check_fwd_meta(B, M, who, false)) return rc;
    MOC_REQUIRE(mixed, "%s: null mixed", who);
    if (int rc = check_fwd_batch(B, who, true, slide0, n)) return rc;
    if (int rc = launch_w1_images(B, M, nullptr, (hipStream_t)stream)) return rc;
    return launch_forward_dense(B, M, gates, mixed, slide0, n, use_bits, (hipStream_t)stream);
}

extern "C" int moc_meta_forward_models(const moc_batch_t* B, const moc_meta_t* M, const moc_runs_t* R, float* mixed,
                                       int slide0, int n, uint32_t use_bits, moc_stream_t stream) {
    const char* who = "moc_meta_forward_models";
    if (int rc = moc_check_batch(B, who)) return rc;
    if (int rc = check_fwd_meta(B, M, who, true)) return rc;
    MOC_REQUIRE(mixed, "%s: null mixed", who);
    if (int rc = check_fwd_runs(B, R, who, "every model works on the same slides")) return rc;
    if (int rc = check_fwd_batch(B, who, false, slide0, n)) return rc;
    // every model's image, rebuilt from its parameters
    if (int rc = launch_w1_images(B, M, R, (hipStream_t)stream)) return rc;
    return launch_forward_models(B, M, R, mixed, slide0, n, use_bits, (hipStream_t)stream);
}

extern "C" int moc_meta_forward_by_slide(const moc_batch_t* B, const moc_meta_t* M, const moc_runs_t* R,
                                         const int32_t* model_of_slide, const moc_meta_ws_t* ws, int slide0, int n,
                                         uint32_t use_bits, moc_stream_t stream) {
    const char* who = "moc_meta_forward_by_slide";
    if (int rc = moc_check_batch(B, who)) return rc;
    if (int rc = check_fwd_meta(B, M, who, true)) return rc;
    MOC_REQUIRE(model_of_slide, "%s: null model_of_slide", who);
    MOC_REQUIRE(ws && ws->mixed, "%s: null work arrays / mixed", who);
    if (int rc = check_fwd_runs(B, R, who, "model_of_slide says which slide is whose")) return rc;
    if (int rc = check_fwd_batch(B, who, false, slide0, n)) return rc;
    if (int rc = launch_w1_images(B, M, R, (hipStream_t)stream)) return rc;
    return launch_forward_by_slide(B, M, R, model_of_slide, ws, slide0, n, use_bits, (hipStream_t)stream);
}

extern "C" int moc_meta_forward_dense_models(const moc_batch_t* B, const moc_meta_t* M, const moc_runs_t* R, float scale,
                                             float* prob_mean, float* prob_std, float* gates_mean, int slide0, int n,
                                             uint32_t use_bits, moc_stream_t stream) {
    const char* who = "moc_meta_forward_dense_models";
    if (int rc = moc_check_batch(B, who)) return rc;
    if (int rc = check_fwd_meta(B, M, who, true)) return rc;
    MOC_REQUIRE(prob_mean, "%s: null prob_mean", who);
    if (int rc = check_fwd_runs(B, R, who, "every model works on the same slides")) return rc;
    MOC_REQUIRE(B->C <= F128_ENS_MAX_C, "%s: C=%d > %d (a tile's mixed scores are reduced in LDS)", who, B->C, F128_ENS_MAX_C);
    MOC_REQUIRE(std::isfinite(scale), "%s: scale=%g is not finite", who, (double)scale);
    if (int rc = check_fwd_batch(B, who, true, slide0, n)) return rc;
    if (int rc = launch_w1_images(B, M, R, (hipStream_t)stream)) return rc;
    return launch_forward_dense_models(B, M, R, scale, prob_mean, prob_std, gates_mean, slide0, n, use_bits, (hipStream_t)stream);
}

extern "C" int moc_mix_fixed(const moc_batch_t* B, const moc_meta_ws_t* ws, int slide0, int n, int mode,
                             moc_stream_t stream) {
    if (int rc = moc_check_batch(B, "moc_mix_fixed")) return rc;
    MOC_REQUIRE(ws && ws->mixed && B->n_sel && B->cand, "moc_mix_fixed: null work array");
    MOC_REQUIRE(!(B->flags & MOC_CAND_FROM_STATS), "moc_mix_fixed: a MOC_CAND_FROM_STATS batch has no materialised candidate scores");
    MOC_REQUIRE(slide0 >= 0 && n >= 1 && slide0 + n <= B->n_slides, "moc_mix_fixed: bad slide range");
    MOC_REQUIRE(mode >= 0 && mode <= 2, "moc_mix_fixed: mode %d not in {0 avg, 1 sum, 2 max}", mode);
    // no meta-learner here: the ablation mixes read the batch's candidate columns only
    FwdArgs a = {};
    a.base_host = -1;
    a.row_off = B->row_off; a.n_sel = B->n_sel; a.cand = B->cand; a.mixed = ws->mixed;
    a.stride = B->total_rows; a.C = B->C; a.slide0 = slide0;
    fixed_mix_kernel<<<dim3(moc_cdiv(s_bound(B), 256), n), 256, 0, (hipStream_t)stream>>>(a, mode);
    MOC_CHECK_LAUNCH("moc_mix_fixed");
    return MOC_OK;
}

extern "C" size_t moc_w1_image_bytes(int D, int dtype) {
    if (D <= 0) return 0;
    (void)dtype;
    return (size_t)D * H * 3 * 2;                            // three bf16 (fp16) terms per weight, every storage
}
