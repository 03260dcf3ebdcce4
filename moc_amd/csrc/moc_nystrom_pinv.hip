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
#include "moc_common.h"

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

__device__ __forceinline__ f32x4_t pv_mfma(float a, float b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float4 pv_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float pv_abs4(float4 v) { return (fabsf(v.x) + fabsf(v.y)) + (fabsf(v.z) + fabsf(v.w)); }

// grid (8 row / column blocks, 8 heads) x 256 threads
__global__ __launch_bounds__(256) void pinv_sums_kernel(const float* X, float* part) {
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
    hipStream_t s = (hipStream_t)stream;
    float* XZ = (float*)ws;
    float *P2 = XZ + PV_MAT, *P3 = P2 + PV_MAT, *Za = P3 + PV_MAT, *Zb = Za + PV_MAT, *part = Zb + PV_MAT;
    // (set on every call: cheap, and there is no once-only flag for two threads to race on)
    const hipError_t ea = hipFuncSetAttribute((const void*)pinv_product_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, PV_PROD_SMEM);
    if (ea != hipSuccess) MOC_FAIL(MOC_ELAUNCH, "moc_nystrom_pinv: %s", hipGetErrorString(ea));
    pinv_sums_kernel<<<dim3(PV_M / PV_SUM_ROWS, PV_HEADS), 256, 0, s>>>(A, part);
    MOC_CHECK_LAUNCH("moc_nystrom_pinv(sums)");
    pinv_init_kernel<<<dim3((PV_M / PV_IT) * (PV_M / PV_IT), PV_HEADS), 256, 0, s>>>(A, part, iters == 0 ? Z : Za);
    MOC_CHECK_LAUNCH("moc_nystrom_pinv(init)");
    for (int it = 0; it < iters; ++it) {
        const float* zin = it & 1 ? Zb : Za;
        float* zout = it == iters - 1 ? Z : (it & 1 ? Za : Zb);
        if (const int rc = pv_product(A, zin, XZ, 1.f, 0.f, s)) return rc;
        if (const int rc = pv_product(XZ, XZ, P2, 1.f, 7.f, s)) return rc;
        if (const int rc = pv_product(XZ, P2, P3, 1.f, 15.f, s)) return rc;
        if (const int rc = pv_product(zin, P3, zout, 0.25f, 13.f, s)) return rc;
    }
    return MOC_OK;
}
