// The landmark pseudo-inverse of the Nystrom layer (moc_amd/nystrom.py: moore_penrose_iter_pinv) as
// a chain of HIP products.  One shape: 8 heads, 256 landmarks, fp32.  X = attn2 [8, 256, 256]:
//
//   col = sum_j |X[h, i, j]|, row = sum_i |X[h, i, j]|;  c = max over ALL heads of col, r = likewise of row
//   Z0 = X^T / (c r)
//   iters times:  XZ = X Z;  P2 = XZ (7 I - XZ);  P3 = XZ (15 I - P2);  Z <- 0.25 Z (13 I - P3)
//
// Init, two launches, no atomics.  pinv_sums_kernel: workgroup (h, b) owns rows 32 b .. 32 b + 31 of head h whole (their
// sums over j) and columns 32 b .. 32 b + 31 whole (their sums over i) and leaves the maximum of each in the workspace:
// 64 pairs.  pinv_init_kernel: every workgroup takes the maximum of the 64 pairs itself (a maximum has no order to keep),
// forms c r as ONE fp32 product and writes a 64 x 64 tile of Z0 transposed through LDS, ONE fp32 division per element --
// what torch's `x.transpose(-1, -2) / (col.max() * row.max())` holds.
//
// One product kernel, four launches per iteration: Out[h] = alpha L[h] (beta I - R[h]), beta = 0 meaning plain R.  The
// right operand is formed as R is read: 0 - r off the diagonal, beta - r on it, the values of torch's `13 * eye - M`.
// alpha (1 or 0.25, exact) multiplies the finished accumulators.  A product needs whole rows of L and whole columns of R,
// so the dependency between products is all-to-all: stream order between launches carries it (no grid barrier, no
// cooperative launch, no flag another workgroup waits on).
//
// Tiling: a workgroup is one head x 32 rows x 64 columns -- 256 workgroups, head = block % 8 so that consecutive
// workgroups (which the dispatcher deals out across the eight XCDs) keep one head's operands in one L2.  Four waves: wave
// w has rows 16 (w & 1) and columns 32 (w >> 1), as TWO 16 x 16 accumulators (v_mfma_f32_16x16x4_f32: 32-cycle issue, 40
// dependent), 128 MFMAs per wave, one wave per SIMD.  Lane l = (c = l & 15, g = l >> 4) holds A[c][slot g] and
// B[slot g][c]; the four K slots of a step may stand for any four k as long as both operands agree: in step (J, t),
// J = 0..15, t = 0..3, slot g is k = 16 J + 4 g + t.  So
//   A: lane (c, g) reads ONE float4 L[row c][16 J + 4 g .. + 3] per J, component t feeding step t.  The L tile lies in LDS
//      in that order ([row block][J][lane], consecutive lanes consecutive 16 bytes), loaded from global in the same order.
//   B: lane (c, g) reads ONE float2 R'[k][2 c, 2 c + 1] per step, component e feeding accumulator e, whose column c is
//      column 2 c + e of the wave's 32: a lane ends with two adjacent columns and stores float2.  The R tile lies in LDS
//      row-major, 64 floats a row, the two 32-float halves of a row swapped where (k >> 2) & 1: the 32 lanes that one
//      ds_read_b64 pass serves (g, g + 1: rows four apart) then cover all 64 banks once.
// All 24 float4 a thread loads (8 of L, 16 of R) are requested up front; they are written to LDS and consumed in four k
// chunks of 64, one barrier each (every chunk has LDS of its own: 32 + 64 KiB), so the first products run while the later
// rows arrive.
//
// moc_nystrom_pinv_iterates is the same launches with every iterate kept: Z_t lands in Zs[t] instead of a ping-pong pair.
//
// The gradient (moc_nystrom_pinv_backward; DESIGN.md section 8c, "the pseudo-inverse's gradient").  From the iterates Z_t
// and dZ = d(Z_iters), for t = iters - 1 .. 0, with XZ, P2, P3 recomputed from Z_t:
//   dP3 = -0.25 Z_t^T dZ;  dP2 = -(XZ^T dP3);  dXZ = dP3 (15 I - P2)^T + dP2 (7 I - XZ)^T - XZ^T dP2
//   dX += dXZ Z_t^T;       dZ <- 0.25 dZ (13 I - P3)^T + X^T dXZ
// then through Z0 = X^T / den, den = c r:  dX += dZ^T / den;  dden = -sum(dZ o Z0) / den;  the rows whose sum is c share
// dden r evenly (torch's rule for a full max()), each element + share x sign(X); the columns whose sum is r share dden c.
//
// pinv_chain_kernel is the product kernel's sibling on the same tiling, lane conventions and LDS images:
//   Out = sum_i op(alpha_i L_i) op'(beta_i I - R_i) [+ C],  one to three terms into the SAME sums in term order,
// op / op' identity or transpose, each per term.  A transpose happens on the way into LDS: the thread still loads 16-byte
// row-contiguous pieces (of rows k of L, 32 floats each; of rows col of R, in 64-byte runs) and scatters their four
// components to where the plain load would have put them.  alpha (+-1, +-0.25: exact) scales L on that way too.  The
// terms reuse the four chunk images; the chunk barriers of one term already order its reads before the next term's
// writes (a wave that writes chunk q of term i + 1 has passed a barrier that every wave reaches after chunk q of term i).
// Summation: the forward's one fp32 chain of 256 products per output is not kept here.  attn2 is positive and close to
// uniform where a landmark holds few tokens; over such operands a sequential fp32 chain drifts, and the gradient --
// already 200 times the size of what is left of it after the softmax backward -- came out 16 times further from float64
// than torch's (7.5e-4 against 4.6e-5 on the layer's attn2 at 257 tokens; an op-by-op restatement of the chain on the CPU
// gives the same figure).  So an fp32 chain is 16 products here (one J), and the 16 x terms partial sums are added in
// double and rounded once: 1.3e-5 in the same restatement.  Sixteen v_add_f64 per J and lane beside 8 MFMAs.
// Independent products share a launch: the argument is a by-value group of up to two product descriptors, workgroup
// block / 256 takes descriptor block / 256.  The grouped schedule, per iteration (four dependent launches):
//   dP3 | XZ of iteration t - 1;   dP2 | P2 of t - 1;   dXZ (three terms) | P3 of t - 1;   dX += | dZ <- (two terms)
// after three launches for the last iteration's XZ, P2, P3: 3 + 4 iters product launches, 27 at six iterations, and four
// for the init (sums, the dden partials, their merge with the tie counts, the final dX +=): 31.  One product per launch
// (MOC_PINV_BWD_GROUPED=0, diagnostic) is 8 per iteration, 52 in all.  No atomics, no grid barrier, no flag: stream order.
#include "moc_common.h"

#include <cstdlib>

namespace {

constexpr int PV_HEADS = 8, PV_M = 256, PV_MAX_ITERS = 64;
constexpr size_t PV_MAT = (size_t)PV_HEADS * PV_M * PV_M;           // floats per [8, 256, 256] matrix
constexpr int PV_SUM_ROWS = 32;                                      // rows (and columns) per workgroup of pinv_sums_kernel
constexpr int PV_PARTS = PV_HEADS * (PV_M / PV_SUM_ROWS);            // 64 (row-sum maximum, column-sum maximum) pairs
constexpr int PV_TR = 32, PV_TC = 64;                                // output tile of the product kernel
constexpr int PV_TILES = (PV_M / PV_TR) * (PV_M / PV_TC);            // 32 per head
constexpr int PV_KCH = 64, PV_NCH = PV_M / PV_KCH;                   // k chunk, chunks
constexpr int PV_PROD_SMEM = (PV_TR * PV_M + PV_M * PV_TC) * 4;      // 96 KiB
constexpr int PV_IT = 64;                                            // tile of the transposing init
// workspace, in floats: XZ | P2 | P3 | Z ping | Z pong | the 64 pairs
constexpr size_t PV_WS_BYTES = (5 * PV_MAT + 2 * PV_PARTS) * sizeof(float);
// the backward's, in floats: two sets of (XZ, P2, P3) | dP3 | dP2 | dXZ | dZ ping | dZ pong | the 64 pairs | the 2 x 2,048
// row and column sums | the record of pinv_dden_merge_kernel (8 floats); then PV_DD_WGS doubles
constexpr int PV_BWD_MATS = 11, PV_NSUMS = PV_HEADS * PV_M, PV_REC = 8;
constexpr int PV_DD_WGS = 256;                                       // workgroups of the dden reduction, 2,048 elements each
constexpr size_t PV_BWD_FLOATS = PV_BWD_MATS * PV_MAT + 2 * PV_PARTS + 2 * PV_NSUMS + PV_REC;
constexpr size_t PV_BWD_WS_BYTES = PV_BWD_FLOATS * sizeof(float) + PV_DD_WGS * sizeof(double);
static_assert(PV_BWD_FLOATS * sizeof(float) % 16 == 0, "the doubles start aligned");
static_assert(PV_MAT == (size_t)PV_DD_WGS * 256 * 8, "two float4 per thread of the dden reduction");

__device__ __forceinline__ f32x4_t pv_mfma(float a, float b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float4 pv_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float pv_abs4(float4 v) { return (fabsf(v.x) + fabsf(v.y)) + (fabsf(v.z) + fabsf(v.w)); }

// grid (8 row / column blocks, 8 heads) x 256 threads.  KEEP (the backward): the sums themselves are left too, sums[h][i]
// over j and sums[2,048 + h][j] over i -- the values whose maxima the forward divides by, from the same instructions.
template <bool KEEP>
__global__ __launch_bounds__(256) void pinv_sums_kernel(const float* X, float* part, float* sums) {
    __shared__ float col_part[8][PV_SUM_ROWS];
    __shared__ float row_max[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.x, h = blockIdx.y;
    const float* Xh = X + (size_t)h * PV_M * PV_M;
    // sums over j of rows 32 b + 8 wave .. + 7: a lane takes four consecutive j, the wave adds up in a fixed tree
    float rmax = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float s = pv_abs4(pv_ld4(Xh + (size_t)(PV_SUM_ROWS * b + 8 * wave + i) * PV_M + 4 * lane));
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) s += __shfl_xor(s, off, 64);
        rmax = fmaxf(rmax, s);
        if constexpr (KEEP) {
            if (lane == 0) sums[h * PV_M + PV_SUM_ROWS * b + 8 * wave + i] = s;
        }
    }
    if (lane == 0) row_max[wave] = rmax;
    // sums over i of columns 32 b .. + 31: thread (column cc, group rg) walks rows rg, rg + 8, ...; groups in index order
    const int cc = threadIdx.x & 31, rg = threadIdx.x >> 5;
    float cs = 0.f;
#pragma unroll 8
    for (int i = rg; i < PV_M; i += 8) cs += fabsf(Xh[(size_t)i * PV_M + PV_SUM_ROWS * b + cc]);
    col_part[rg][cc] = cs;
    __syncthreads();
    if (threadIdx.x < 64) {
        float v = 0.f;
        if (threadIdx.x < PV_SUM_ROWS) {
#pragma unroll
            for (int k = 0; k < 8; ++k) v += col_part[k][threadIdx.x];
            if constexpr (KEEP) sums[PV_NSUMS + h * PV_M + PV_SUM_ROWS * b + threadIdx.x] = v;
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
        if (threadIdx.x == 0) {
            part[2 * (h * (PV_M / PV_SUM_ROWS) + b)] = fmaxf(fmaxf(row_max[0], row_max[1]), fmaxf(row_max[2], row_max[3]));
            part[2 * (h * (PV_M / PV_SUM_ROWS) + b) + 1] = v;
        }
    }
}

// grid (16 tiles of 64 x 64, 8 heads) x 256 threads: Z0[h][j][i] = X[h][i][j] / (c r)
__global__ __launch_bounds__(256) void pinv_init_kernel(const float* X, const float* part, float* Z0) {
    __shared__ float tile[PV_IT][PV_IT + 1];
    const int h = blockIdx.y, i0 = (blockIdx.x >> 2) * PV_IT, j0 = (blockIdx.x & 3) * PV_IT;
    float c = 0.f, r = 0.f;
    for (int k = 0; k < PV_PARTS; ++k) {
        c = fmaxf(c, part[2 * k]);
        r = fmaxf(r, part[2 * k + 1]);
    }
    const float den = moc_fmul(c, r);
    const float* Xh = X + (size_t)h * PV_M * PV_M;
    float* Zh = Z0 + (size_t)h * PV_M * PV_M;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int f = it * 256 + threadIdx.x, ii = f >> 4, j4 = (f & 15) * 4;
        const float4 v = pv_ld4(Xh + (size_t)(i0 + ii) * PV_M + j0 + j4);
        tile[ii][j4] = v.x; tile[ii][j4 + 1] = v.y; tile[ii][j4 + 2] = v.z; tile[ii][j4 + 3] = v.w;
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int f = it * 256 + threadIdx.x, jj = f >> 4, i4 = (f & 15) * 4;
        *reinterpret_cast<float4*>(Zh + (size_t)(j0 + jj) * PV_M + i0 + i4) =
            float4{moc_fdiv(tile[i4][jj], den), moc_fdiv(tile[i4 + 1][jj], den), moc_fdiv(tile[i4 + 2][jj], den),
                   moc_fdiv(tile[i4 + 3][jj], den)};
    }
}

// grid 256 (head = block % 8, tile = block / 8) x 256 threads, PV_PROD_SMEM bytes of dynamic LDS
__global__ __launch_bounds__(256) void pinv_product_kernel(const float* L, const float* R, float* Out, float alpha, float beta) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4* aimg = reinterpret_cast<float4*>(smem);                   // [row block 2][J 16][lane 64]
    float* bimg = reinterpret_cast<float*>(smem) + PV_TR * PV_M;      // [k 256][64], halves swapped where (k >> 2) & 1
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    const int h = blockIdx.x & (PV_HEADS - 1), tl = blockIdx.x >> 3;
    const int row0 = (tl >> 2) * PV_TR, col0 = (tl & 3) * PV_TC;
    const float* Lh = L + (size_t)h * PV_M * PV_M;
    const float* Rh = R + (size_t)h * PV_M * PV_M;

    float4 av[PV_NCH][2], bv[PV_NCH][4];
#pragma unroll
    for (int q = 0; q < PV_NCH; ++q) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {                                 // idx = 256 i + tid: row block i, J = 4 q + wave, this lane
            av[q][i] = pv_ld4(Lh + (size_t)(row0 + 16 * i + c) * PV_M + 16 * (4 * q + wave) + 4 * g);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {                                 // f = 256 i + tid: row 64 q + f / 16, four columns at 4 (f % 16)
            const int f = 256 * i + tid;
            bv[q][i] = pv_ld4(Rh + (size_t)(PV_KCH * q + (f >> 4)) * PV_M + col0 + 4 * (f & 15));
        }
    }
    const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4_t acc0 = zero4, acc1 = zero4;
    const int rb = wave & 1, cw = wave >> 1;
#pragma unroll
    for (int q = 0; q < PV_NCH; ++q) {
#pragma unroll
        for (int i = 0; i < 2; ++i) aimg[(i * 16 + 4 * q + wave) * 64 + lane] = av[q][i];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = 256 * i + tid, k = PV_KCH * q + (f >> 4), c4 = 4 * (f & 15);
            float4 v = bv[q][i];
            if (beta != 0.f) {                                        // beta I - R: 0 - r off the diagonal, beta - r on it
                const int d = k - (col0 + c4);                        // the diagonal's component, if 0..3
                v.x = moc_fsub(d == 0 ? beta : 0.f, v.x); v.y = moc_fsub(d == 1 ? beta : 0.f, v.y);
                v.z = moc_fsub(d == 2 ? beta : 0.f, v.z); v.w = moc_fsub(d == 3 ? beta : 0.f, v.w);
            }
            *reinterpret_cast<float4*>(bimg + k * PV_TC + (c4 ^ (((k >> 2) & 1) << 5))) = v;
        }
        __syncthreads();
#pragma unroll
        for (int J = 4 * q; J < 4 * q + 4; ++J) {
            const float4 a4 = aimg[(rb * 16 + J) * 64 + lane];
            const float a[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int k = 16 * J + 4 * g + t;                     // (k >> 2) & 1 == g & 1
                const float2 b2 = *reinterpret_cast<const float2*>(bimg + k * PV_TC + ((32 * cw + 2 * c) ^ ((g & 1) << 5)));
                acc0 = pv_mfma(a[t], b2.x, acc0);
                acc1 = pv_mfma(a[t], b2.y, acc1);
            }
        }
    }
    float* op = Out + (size_t)h * PV_M * PV_M + (size_t)(row0 + 16 * rb + 4 * g) * PV_M + col0 + 32 * cw + 2 * c;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        *reinterpret_cast<float2*>(op + (size_t)r * PV_M) = float2{moc_fmul(alpha, acc0[r]), moc_fmul(alpha, acc1[r])};
}

// ---- the backward's products: Out = sum_i op(alpha_i L_i) op'(beta_i I - R_i) [+ C]
struct PvTerm {
    const float* L;
    const float* R;
    float alpha, beta;     // alpha scales L (exact for the powers of two in use); beta = 0: plain R
    int lt, rt;            // 1: the operand is read transposed
};
struct PvProd {
    PvTerm t[3];
    const float* C;        // null, or an additive [8, 256, 256] (may be Out itself: a thread reads what it alone writes)
    float* Out;
    int nterms, pad_;
};
struct PvGroup { PvProd p[2]; };

// grid 256 x (1 or 2 products) x 256 threads, PV_PROD_SMEM bytes of dynamic LDS; pinv_product_kernel's tiling and images
__global__ __launch_bounds__(256) void pinv_chain_kernel(const PvGroup G) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4* aimg = reinterpret_cast<float4*>(smem);                   // [row block 2][J 16][lane 64]
    float* afl = reinterpret_cast<float*>(smem);
    float* bimg = reinterpret_cast<float*>(smem) + PV_TR * PV_M;      // [k 256][64], halves swapped where (k >> 2) & 1
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    const PvProd& P = G.p[blockIdx.x >> 8];
    const int blk = blockIdx.x & 255, h = blk & (PV_HEADS - 1), tl = blk >> 3;
    const int row0 = (tl >> 2) * PV_TR, col0 = (tl & 3) * PV_TC;
    const size_t hoff = (size_t)h * PV_M * PV_M;
    const int rb = wave & 1, cw = wave >> 1;
    const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
    // no fp32 chain longer than 16 products: every J starts fresh accumulators, which are added to these in double (see the
    // header: a 256-product fp32 chain over operands of one sign costs the gradient a digit)
    double sum0[4] = {0.0, 0.0, 0.0, 0.0}, sum1[4] = {0.0, 0.0, 0.0, 0.0};
    const int nterms = P.nterms;
    for (int n = 0; n < nterms; ++n) {
        const float* Lh = P.t[n].L + hoff;
        const float* Rh = P.t[n].R + hoff;
        const float alpha = P.t[n].alpha, beta = P.t[n].beta;
        const bool lt = P.t[n].lt != 0, rt = P.t[n].rt != 0;
        float4 av[PV_NCH][2], bv[PV_NCH][4];
#pragma unroll
        for (int q = 0; q < PV_NCH; ++q) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int f = 256 * i + tid;
                // plain: row block i, J = 4 q + wave, this lane.  transposed: row k = 64 q + f / 8 of L, its floats row0 + 4 (f % 8) ..
                av[q][i] = lt ? pv_ld4(Lh + (size_t)(PV_KCH * q + (f >> 3)) * PV_M + row0 + 4 * (f & 7))
                              : pv_ld4(Lh + (size_t)(row0 + 16 * i + c) * PV_M + 16 * (4 * q + wave) + 4 * g);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int f = 256 * i + tid;
                // plain: row 64 q + f / 16, four columns at 4 (f % 16).  transposed: row col0 + j of R, j = 16 (u & 3) + f % 16,
                // u = f / 64; its floats k4 .., k4 = 64 q + 16 (u >> 2) + 4 ((f / 16) % 4): sixteen 64-byte runs per wave
                const int u = f >> 6;
                bv[q][i] = rt ? pv_ld4(Rh + (size_t)(col0 + 16 * (u & 3) + (f & 15)) * PV_M + PV_KCH * q + 16 * (u >> 2) + 4 * ((f >> 4) & 3))
                              : pv_ld4(Rh + (size_t)(PV_KCH * q + (f >> 4)) * PV_M + col0 + 4 * (f & 15));
            }
        }
#pragma unroll
        for (int q = 0; q < PV_NCH; ++q) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float4 v = av[q][i];
                v.x = moc_fmul(alpha, v.x); v.y = moc_fmul(alpha, v.y); v.z = moc_fmul(alpha, v.z); v.w = moc_fmul(alpha, v.w);
                if (lt) {                                             // component e is L'[row 4 p + e][k]
                    const int f = 256 * i + tid, k = PV_KCH * q + (f >> 3), p = f & 7;
                    float* dst = afl + ((((p >> 2) * 16 + (k >> 4)) * 64 + ((k >> 2) & 3) * 16 + 4 * (p & 3)) * 4 + (k & 3));
                    dst[0] = v.x; dst[4] = v.y; dst[8] = v.z; dst[12] = v.w;
                } else {
                    aimg[(i * 16 + 4 * q + wave) * 64 + lane] = v;
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int f = 256 * i + tid, u = f >> 6;
                float4 v = bv[q][i];
                if (rt) {                                             // component e is R'[k4 + e][col0 + j]
                    const int j = 16 * (u & 3) + (f & 15), k4 = PV_KCH * q + 16 * (u >> 2) + 4 * ((f >> 4) & 3);
                    if (beta != 0.f) {
                        const int d = col0 + j - k4;
                        v.x = moc_fsub(d == 0 ? beta : 0.f, v.x); v.y = moc_fsub(d == 1 ? beta : 0.f, v.y);
                        v.z = moc_fsub(d == 2 ? beta : 0.f, v.z); v.w = moc_fsub(d == 3 ? beta : 0.f, v.w);
                    }
                    float* dst = bimg + k4 * PV_TC + (j ^ (((k4 >> 2) & 1) << 5));
                    dst[0] = v.x; dst[PV_TC] = v.y; dst[2 * PV_TC] = v.z; dst[3 * PV_TC] = v.w;
                } else {
                    const int k = PV_KCH * q + (f >> 4), c4 = 4 * (f & 15);
                    if (beta != 0.f) {
                        const int d = k - (col0 + c4);
                        v.x = moc_fsub(d == 0 ? beta : 0.f, v.x); v.y = moc_fsub(d == 1 ? beta : 0.f, v.y);
                        v.z = moc_fsub(d == 2 ? beta : 0.f, v.z); v.w = moc_fsub(d == 3 ? beta : 0.f, v.w);
                    }
                    *reinterpret_cast<float4*>(bimg + k * PV_TC + (c4 ^ (((k >> 2) & 1) << 5))) = v;
                }
            }
            __syncthreads();
#pragma unroll
            for (int J = 4 * q; J < 4 * q + 4; ++J) {
                const float4 a4 = aimg[(rb * 16 + J) * 64 + lane];
                const float a[4] = {a4.x, a4.y, a4.z, a4.w};
                f32x4_t acc0 = zero4, acc1 = zero4;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int k = 16 * J + 4 * g + t;
                    const float2 b2 = *reinterpret_cast<const float2*>(bimg + k * PV_TC + ((32 * cw + 2 * c) ^ ((g & 1) << 5)));
                    acc0 = pv_mfma(a[t], b2.x, acc0);
                    acc1 = pv_mfma(a[t], b2.y, acc1);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    sum0[r] += (double)acc0[r];
                    sum1[r] += (double)acc1[r];
                }
            }
        }
    }
    const size_t ooff = hoff + (size_t)(row0 + 16 * rb + 4 * g) * PV_M + col0 + 32 * cw + 2 * c;
    const float* cp = P.C;
    float* op = P.Out + ooff;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float2 o = float2{(float)sum0[r], (float)sum1[r]};
        if (cp) {
            const float2 cc = *reinterpret_cast<const float2*>(cp + ooff + (size_t)r * PV_M);
            o.x = moc_fadd(cc.x, o.x); o.y = moc_fadd(cc.y, o.y);
        }
        *reinterpret_cast<float2*>(op + (size_t)r * PV_M) = o;
    }
}

// ---- the backward through Z0 = X^T / (c r)
// grid PV_DD_WGS x 256 threads: part[w] = sum over the workgroup's 2,048 elements of dZ0 o Z0, in double: a thread's eight
// products in index order, then a fixed tree over the threads
__global__ __launch_bounds__(256) void pinv_dden_partial_kernel(const float* dZ0, const float* Z0, double* part) {
    __shared__ double tree[256];
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const size_t at = ((size_t)blockIdx.x * 512 + 256 * i + threadIdx.x) * 4;
        const float4 a = pv_ld4(dZ0 + at), b = pv_ld4(Z0 + at);
        s += (double)a.x * (double)b.x;
        s += (double)a.y * (double)b.y;
        s += (double)a.z * (double)b.z;
        s += (double)a.w * (double)b.w;
    }
    tree[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) tree[threadIdx.x] += tree[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = tree[0];
}

// one workgroup x 256 threads: c, r and den as pinv_init_kernel forms them, the number of rows whose sum IS c and of
// columns whose sum IS r over all heads, the PV_DD_WGS partials added in a fixed tree, and the record the last kernel
// reads: rec = {den, dden r / row ties, dden c / column ties, c, r} with dden = -sum / den (formed in double, rounded once)
__global__ __launch_bounds__(256) void pinv_dden_merge_kernel(const float* part, const float* sums, const double* dpart, float* rec) {
    __shared__ double tree[256];
    __shared__ int ties[2][256];
    float c = 0.f, r = 0.f;
    for (int k = 0; k < PV_PARTS; ++k) {
        c = fmaxf(c, part[2 * k]);
        r = fmaxf(r, part[2 * k + 1]);
    }
    int tc = 0, tr = 0;
    for (int k = threadIdx.x; k < PV_NSUMS; k += 256) {
        tc += sums[k] == c;
        tr += sums[PV_NSUMS + k] == r;
    }
    static_assert(PV_DD_WGS == 256, "one partial per thread");
    tree[threadIdx.x] = dpart[threadIdx.x];
    ties[0][threadIdx.x] = tc;
    ties[1][threadIdx.x] = tr;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            tree[threadIdx.x] += tree[threadIdx.x + off];
            ties[0][threadIdx.x] += ties[0][threadIdx.x + off];
            ties[1][threadIdx.x] += ties[1][threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float den = moc_fmul(c, r);
        const double dden = -tree[0] / (double)den;
        rec[0] = den;
        rec[1] = (float)(dden * (double)r / (double)ties[0][0]);
        rec[2] = (float)(dden * (double)c / (double)ties[1][0]);
        rec[3] = c;
        rec[4] = r;
    }
}

// grid (16 tiles of 64 x 64, 8 heads) x 256 threads:
//   dX[h][i][j] (+)= dZ0[h][j][i] / den + sign(X) ([sum_j |X[h][i]| == c] rec[1]) + sign(X) ([sum_i |X[h][.][j]| == r] rec[2])
__global__ __launch_bounds__(256) void pinv_init_backward_kernel(const float* X, const float* dZ0, const float* sums, const float* rec,
                                                                  float* dX, int accumulate) {
    __shared__ float tile[PV_IT][PV_IT + 1];
    const int h = blockIdx.y, i0 = (blockIdx.x >> 2) * PV_IT, j0 = (blockIdx.x & 3) * PV_IT;
    const float den = rec[0], share_c = rec[1], share_r = rec[2], c = rec[3], r = rec[4];
    const size_t hoff = (size_t)h * PV_M * PV_M;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int f = it * 256 + threadIdx.x, jj = f >> 4, i4 = (f & 15) * 4;
        const float4 v = pv_ld4(dZ0 + hoff + (size_t)(j0 + jj) * PV_M + i0 + i4);
        tile[jj][i4] = v.x; tile[jj][i4 + 1] = v.y; tile[jj][i4 + 2] = v.z; tile[jj][i4 + 3] = v.w;
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int f = it * 256 + threadIdx.x, ii = f >> 4, j4 = (f & 15) * 4;
        const size_t at = hoff + (size_t)(i0 + ii) * PV_M + j0 + j4;
        const float4 x = pv_ld4(X + at);
        const float4 cs = pv_ld4(sums + PV_NSUMS + h * PV_M + j0 + j4);
        const float tc = sums[h * PV_M + i0 + ii] == c ? share_c : 0.f;
        const float xs[4] = {x.x, x.y, x.z, x.w}, cv[4] = {cs.x, cs.y, cs.z, cs.w};
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float sg = xs[e] > 0.f ? 1.f : (xs[e] < 0.f ? -1.f : 0.f);
            float v = moc_fdiv(tile[j4 + e][ii], den);
            v = moc_fadd(v, moc_fmul(sg, tc));
            v = moc_fadd(v, moc_fmul(sg, cv[e] == r ? share_r : 0.f));
            o[e] = v;
        }
        if (accumulate) {
            const float4 old = pv_ld4(dX + at);
            o[0] = moc_fadd(old.x, o[0]); o[1] = moc_fadd(old.y, o[1]); o[2] = moc_fadd(old.z, o[2]); o[3] = moc_fadd(old.w, o[3]);
        }
        *reinterpret_cast<float4*>(dX + at) = float4{o[0], o[1], o[2], o[3]};
    }
}

bool pv_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool pv_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

int pv_product(const float* L, const float* R, float* Out, float alpha, float beta, hipStream_t s) {
    pinv_product_kernel<<<PV_HEADS * PV_TILES, 256, PV_PROD_SMEM, s>>>(L, R, Out, alpha, beta);
    MOC_CHECK_LAUNCH("moc_nystrom_pinv(product)");
    return MOC_OK;
}

// The forward's launches.  Z_t lands in Zs[t] where Zs is given (moc_nystrom_pinv_iterates), else in the workspace's
// ping-pong pair and the last one in Z (moc_nystrom_pinv).
int pv_forward(const float* A, int iters, float* Zs, float* Z, float* ws, hipStream_t s) {
    float* XZ = ws;
    float *P2 = XZ + PV_MAT, *P3 = P2 + PV_MAT, *Za = P3 + PV_MAT, *Zb = Za + PV_MAT, *part = Zb + PV_MAT;
    auto at = [&](int t) { return Zs ? Zs + (size_t)t * PV_MAT : (t == iters ? Z : (t & 1 ? Zb : Za)); };
    // (set on every call: cheap, and there is no once-only flag for two threads to race on)
    const hipError_t ea = hipFuncSetAttribute((const void*)pinv_product_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, PV_PROD_SMEM);
    if (ea != hipSuccess) MOC_FAIL(MOC_ELAUNCH, "moc_nystrom_pinv: %s", hipGetErrorString(ea));
    pinv_sums_kernel<false><<<dim3(PV_M / PV_SUM_ROWS, PV_HEADS), 256, 0, s>>>(A, part, nullptr);
    MOC_CHECK_LAUNCH("moc_nystrom_pinv(sums)");
    pinv_init_kernel<<<dim3((PV_M / PV_IT) * (PV_M / PV_IT), PV_HEADS), 256, 0, s>>>(A, part, at(0));
    MOC_CHECK_LAUNCH("moc_nystrom_pinv(init)");
    for (int it = 0; it < iters; ++it) {
        const float* zin = at(it);
        if (const int rc = pv_product(A, zin, XZ, 1.f, 0.f, s)) return rc;
        if (const int rc = pv_product(XZ, XZ, P2, 1.f, 7.f, s)) return rc;
        if (const int rc = pv_product(XZ, P2, P3, 1.f, 15.f, s)) return rc;
        if (const int rc = pv_product(zin, P3, at(it + 1), 0.25f, 13.f, s)) return rc;
    }
    return MOC_OK;
}

PvTerm pv_term(const float* L, bool lt, const float* R, bool rt, float alpha, float beta) {
    return PvTerm{L, R, alpha, beta, lt ? 1 : 0, rt ? 1 : 0};
}
PvProd pv_prod(float* Out, const float* C, PvTerm a) { return PvProd{{a, PvTerm{}, PvTerm{}}, C, Out, 1, 0}; }
PvProd pv_prod(float* Out, const float* C, PvTerm a, PvTerm b) { return PvProd{{a, b, PvTerm{}}, C, Out, 2, 0}; }
PvProd pv_prod(float* Out, const float* C, PvTerm a, PvTerm b, PvTerm c) { return PvProd{{a, b, c}, C, Out, 3, 0}; }

// one launch of one product, or of two independent ones side by side
int pv_chain(const PvProd& a, const PvProd* b, hipStream_t s) {
    PvGroup G{};
    G.p[0] = a;
    if (b) G.p[1] = *b;
    pinv_chain_kernel<<<PV_HEADS * PV_TILES * (b ? 2 : 1), 256, PV_PROD_SMEM, s>>>(G);
    MOC_CHECK_LAUNCH("moc_nystrom_pinv_backward(product)");
    return MOC_OK;
}

}  // namespace

extern "C" size_t moc_nystrom_pinv_workspace(int heads, int landmarks) {
    return heads == PV_HEADS && landmarks == PV_M ? PV_WS_BYTES : 0;
}

extern "C" int moc_nystrom_pinv(const float* A, int heads, int landmarks, int iters, float* Z, void* ws, size_t ws_bytes,
                                moc_stream_t stream) {
    MOC_REQUIRE(A, "moc_nystrom_pinv: A is null");
    MOC_REQUIRE(Z, "moc_nystrom_pinv: Z is null");
    MOC_REQUIRE(ws, "moc_nystrom_pinv: ws is null");
    if (heads != PV_HEADS || landmarks != PV_M)
        MOC_FAIL(MOC_EUNSUPPORTED, "moc_nystrom_pinv: heads=%d landmarks=%d, only 8 heads with 256 landmarks is built", heads, landmarks);
    MOC_REQUIRE(iters >= 0 && iters <= PV_MAX_ITERS, "moc_nystrom_pinv: iters=%d must be in 0..%d", iters, PV_MAX_ITERS);
    MOC_REQUIRE(pv_aligned(A) && pv_aligned(Z) && pv_aligned(ws), "moc_nystrom_pinv: A, Z and ws must be 16-byte aligned");
    MOC_REQUIRE(ws_bytes >= PV_WS_BYTES, "moc_nystrom_pinv: ws_bytes=%zu, need %zu", ws_bytes, PV_WS_BYTES);
    const size_t mat = PV_MAT * sizeof(float);
    MOC_REQUIRE(!pv_overlap(A, mat, Z, mat), "moc_nystrom_pinv: A and Z overlap");
    MOC_REQUIRE(!pv_overlap(ws, PV_WS_BYTES, A, mat) && !pv_overlap(ws, PV_WS_BYTES, Z, mat), "moc_nystrom_pinv: ws overlaps A or Z");
    return pv_forward(A, iters, nullptr, Z, (float*)ws, (hipStream_t)stream);
}

extern "C" int moc_nystrom_pinv_iterates(const float* A, int heads, int landmarks, int iters, float* Zs, void* ws, size_t ws_bytes,
                                         moc_stream_t stream) {
    MOC_REQUIRE(A, "moc_nystrom_pinv_iterates: A is null");
    MOC_REQUIRE(Zs, "moc_nystrom_pinv_iterates: Zs is null");
    MOC_REQUIRE(ws, "moc_nystrom_pinv_iterates: ws is null");
    if (heads != PV_HEADS || landmarks != PV_M)
        MOC_FAIL(MOC_EUNSUPPORTED, "moc_nystrom_pinv_iterates: heads=%d landmarks=%d, only 8 heads with 256 landmarks is built", heads,
                 landmarks);
    MOC_REQUIRE(iters >= 0 && iters <= PV_MAX_ITERS, "moc_nystrom_pinv_iterates: iters=%d must be in 0..%d", iters, PV_MAX_ITERS);
    MOC_REQUIRE(pv_aligned(A) && pv_aligned(Zs) && pv_aligned(ws), "moc_nystrom_pinv_iterates: A, Zs and ws must be 16-byte aligned");
    const size_t mat = PV_MAT * sizeof(float), all = (size_t)(iters + 1) * mat;
    MOC_REQUIRE(!pv_overlap(A, mat, Zs, all), "moc_nystrom_pinv_iterates: A and Zs overlap");
    MOC_REQUIRE(!pv_overlap(ws, PV_WS_BYTES, A, mat) && !pv_overlap(ws, PV_WS_BYTES, Zs, all),
                "moc_nystrom_pinv_iterates: ws overlaps A or Zs");
    MOC_REQUIRE(ws_bytes >= PV_WS_BYTES, "moc_nystrom_pinv_iterates: ws_bytes=%zu, need %zu", ws_bytes, PV_WS_BYTES);
    return pv_forward(A, iters, Zs, nullptr, (float*)ws, (hipStream_t)stream);
}

extern "C" size_t moc_nystrom_pinv_backward_workspace(int heads, int landmarks) {
    return heads == PV_HEADS && landmarks == PV_M ? PV_BWD_WS_BYTES : 0;
}

extern "C" int moc_nystrom_pinv_backward(const float* A, int heads, int landmarks, int iters, const float* Zs, const float* dZ,
                                         float* dA, void* ws, size_t ws_bytes, moc_stream_t stream) {
    MOC_REQUIRE(A, "moc_nystrom_pinv_backward: A is null");
    MOC_REQUIRE(Zs, "moc_nystrom_pinv_backward: Zs is null");
    MOC_REQUIRE(dZ, "moc_nystrom_pinv_backward: dZ is null");
    MOC_REQUIRE(dA, "moc_nystrom_pinv_backward: dA is null");
    MOC_REQUIRE(ws, "moc_nystrom_pinv_backward: ws is null");
    if (heads != PV_HEADS || landmarks != PV_M)
        MOC_FAIL(MOC_EUNSUPPORTED, "moc_nystrom_pinv_backward: heads=%d landmarks=%d, only 8 heads with 256 landmarks is built", heads,
                 landmarks);
    MOC_REQUIRE(iters >= 0 && iters <= PV_MAX_ITERS, "moc_nystrom_pinv_backward: iters=%d must be in 0..%d", iters, PV_MAX_ITERS);
    MOC_REQUIRE(pv_aligned(A) && pv_aligned(Zs) && pv_aligned(dZ) && pv_aligned(dA) && pv_aligned(ws),
                "moc_nystrom_pinv_backward: A, Zs, dZ, dA and ws must be 16-byte aligned");
    const size_t mat = PV_MAT * sizeof(float);
    const struct { const void* p; size_t n; const char* name; } buf[5] = {
        {A, mat, "A"}, {Zs, (size_t)(iters + 1) * mat, "Zs"}, {dZ, mat, "dZ"}, {dA, mat, "dA"}, {ws, PV_BWD_WS_BYTES, "ws"}};
    for (int i = 0; i < 5; ++i)
        for (int j = i + 1; j < 5; ++j)
            MOC_REQUIRE(!pv_overlap(buf[i].p, buf[i].n, buf[j].p, buf[j].n), "moc_nystrom_pinv_backward: %s and %s overlap", buf[i].name,
                        buf[j].name);
    MOC_REQUIRE(ws_bytes >= PV_BWD_WS_BYTES, "moc_nystrom_pinv_backward: ws_bytes=%zu, need %zu", ws_bytes, PV_BWD_WS_BYTES);
    hipStream_t s = (hipStream_t)stream;
    float* F[2][3];                                                   // two sets of XZ, P2, P3
    float* w = (float*)ws;
    for (int k = 0; k < 6; ++k) F[k / 3][k % 3] = w + (size_t)k * PV_MAT;
    float *dP3 = w + 6 * PV_MAT, *dP2 = dP3 + PV_MAT, *dXZ = dP2 + PV_MAT, *dZp[2] = {dXZ + PV_MAT, dXZ + 2 * PV_MAT};
    float *part = w + PV_BWD_MATS * PV_MAT, *sums = part + 2 * PV_PARTS, *rec = sums + 2 * PV_NSUMS;
    double* dpart = (double*)(w + PV_BWD_FLOATS);
    const char* env = getenv("MOC_PINV_BWD_GROUPED");                 // diagnostic: 0 = one product per launch
    const bool grouped = !(env && atoi(env) == 0);
    const hipError_t ea = hipFuncSetAttribute((const void*)pinv_chain_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, PV_PROD_SMEM);
    if (ea != hipSuccess) MOC_FAIL(MOC_ELAUNCH, "moc_nystrom_pinv_backward: %s", hipGetErrorString(ea));

    // XZ, P2, P3 of iterate Zt into set f: step 0, 1, 2
    auto fwd = [&](int f, const float* Zt, int step) {
        float *XZ = F[f][0], *P2 = F[f][1], *P3 = F[f][2];
        return step == 0   ? pv_prod(XZ, nullptr, pv_term(A, false, Zt, false, 1.f, 0.f))
               : step == 1 ? pv_prod(P2, nullptr, pv_term(XZ, false, XZ, false, 1.f, 7.f))
                           : pv_prod(P3, nullptr, pv_term(XZ, false, P2, false, 1.f, 15.f));
    };
    const float* dZin = dZ;
    int cur = 0;
    if (grouped && iters > 0)
        for (int step = 0; step < 3; ++step) {
            const PvProd p = fwd(cur, Zs + (size_t)(iters - 1) * PV_MAT, step);
            if (const int rc = pv_chain(p, nullptr, s)) return rc;
        }
    for (int t = iters - 1; t >= 0; --t) {
        const float* Zt = Zs + (size_t)t * PV_MAT;
        const float *XZ = F[cur][0], *P2 = F[cur][1], *P3 = F[cur][2];
        float* dZout = dZp[(iters - 1 - t) & 1];
        if (!grouped)
            for (int step = 0; step < 3; ++step) {
                const PvProd p = fwd(cur, Zt, step);
                if (const int rc = pv_chain(p, nullptr, s)) return rc;
            }
        const PvProd back[3] = {
            pv_prod(dP3, nullptr, pv_term(Zt, true, dZin, false, -0.25f, 0.f)),
            pv_prod(dP2, nullptr, pv_term(XZ, true, dP3, false, -1.f, 0.f)),
            pv_prod(dXZ, nullptr, pv_term(dP3, false, P2, true, 1.f, 15.f), pv_term(dP2, false, XZ, true, 1.f, 7.f),
                    pv_term(XZ, true, dP2, false, -1.f, 0.f))};
        const bool beside = grouped && t > 0;                         // the next (earlier) iteration's XZ, P2, P3 ride along
        for (int step = 0; step < 3; ++step) {
            const PvProd side = beside ? fwd(cur ^ 1, Zt - PV_MAT, step) : PvProd{};
            if (const int rc = pv_chain(back[step], beside ? &side : nullptr, s)) return rc;
        }
        const PvProd pdX = pv_prod(dA, t == iters - 1 ? nullptr : dA, pv_term(dXZ, false, Zt, true, 1.f, 0.f));
        const PvProd pdZ = pv_prod(dZout, nullptr, pv_term(dZin, false, P3, true, 0.25f, 13.f), pv_term(A, true, dXZ, false, 1.f, 0.f));
        if (grouped) {
            if (const int rc = pv_chain(pdX, &pdZ, s)) return rc;
        } else {
            if (const int rc = pv_chain(pdX, nullptr, s)) return rc;
            if (const int rc = pv_chain(pdZ, nullptr, s)) return rc;
        }
        dZin = dZout;
        if (grouped) cur ^= 1;
    }
    // through Z0 = A^T / (c r): dZin is d(Z0) now
    pinv_sums_kernel<true><<<dim3(PV_M / PV_SUM_ROWS, PV_HEADS), 256, 0, s>>>(A, part, sums);
    MOC_CHECK_LAUNCH("moc_nystrom_pinv_backward(sums)");
    pinv_dden_partial_kernel<<<PV_DD_WGS, 256, 0, s>>>(dZin, Zs, dpart);
    MOC_CHECK_LAUNCH("moc_nystrom_pinv_backward(dden partials)");
    pinv_dden_merge_kernel<<<1, 256, 0, s>>>(part, sums, dpart, rec);
    MOC_CHECK_LAUNCH("moc_nystrom_pinv_backward(dden merge)");
    pinv_init_backward_kernel<<<dim3((PV_M / PV_IT) * (PV_M / PV_IT), PV_HEADS), 256, 0, s>>>(A, dZin, sums, rec, dA, iters > 0 ? 1 : 0);
    MOC_CHECK_LAUNCH("moc_nystrom_pinv_backward(init)");
    return MOC_OK;
}
