// TransMIL's PPEG (moc_amd/model_mil.py: PPEG; DESIGN.md section 8c, "PPEG"): the depth-wise 7 x 7, 5 x 5 and 3 x 3
// convolutions over the H x W token square, the identity and the three biases as ONE 49-tap pass, and its gradients.
// x, out, dout, dx are [1 + H W, 512], row 0 the class token, token 1 + y W + x_ position (y, x_): channels-last, a
// position's 512 channels are 2 KB.  With zero padding outside the square:
//       out[0]        = x[0]
//       out[1 + p, c] = x[1 + p, c] + ((b7[c] + b5[c]) + b3[c]) + sum_{dy, dx in -3..3} w[c, dy, dx] x[1 + p + (dy, dx), c]
//                       w = (w7 + pad(w5)) + pad(w3): the 5 x 5 and the 3 x 3 sit in the centre of the 7 x 7
//       dx[0]         = dout[0]
//       dx[1 + p, c]  = dout[1 + p, c] + sum_{dy, dx} w[c, dy, dx] dout[1 + p - (dy, dx), c]
//       G[c, dy, dx]  = sum_p dout[1 + p, c] x[1 + p + (dy, dx), c]
//       dw7 = G;  dw5, dw3 = G's central 5 x 5 and 3 x 3;  db7 = db5 = db3 = sum_p dout[1 + p, c]
//
// No operand is shared between channels, so this is a VALU kernel: a lane owns one channel (a wave reads 256 contiguous
// bytes of a position), holds the 49 merged taps of its channel in registers, and works on tiles of 4 x 4 positions.
// For a tile it requests the 10 x 10 positions around it (and, in the backward, the tile's 16 values of x) before it waits
// for any of them; a loaded value then feeds up to 49 FMAs.  A position outside the square is not read: the coordinates
// are clamped to the square, and the value is replaced by zero.
//   forward: one workgroup (one wave) per tile and 64 channels; the one for tile 0 also copies the class-token row.
//   backward: dx is the forward's loop over dout with the table read backwards.  G is summed the other way round,
//       G[d] = sum_q x[q] dout[q - d], so that it needs the SAME 10 x 10 values of dout and only the tile's own 16 of x.
//       A workgroup is two waves that share a run of consecutive tiles (row-major tile order), the tiles in turn.  An
//       entry of G is one fp32 chain of a tile's 16 products, then a double: a lane adds it to one of 50 doubles of its
//       own in LDS (nothing is summed in fp32 across tiles, so no fp32 sum lives in registers beside the 100 values of
//       dout).  At its end wave 0 adds the two waves' sums in index order and leaves 50 doubles per channel in the
//       workspace, [block][50][512]; a merge launch adds the blocks in index order, rounds to fp32 once and writes the six
//       gradient tensors.
// No atomics, no grid barrier: stream order only, the same bits on every call.
#include "moc_common.h"

namespace {

constexpr int PG_DIM = 512;                              // the one built width
constexpr int PG_LANES = 64;                             // channels per workgroup: one wave
constexpr int PG_CG = PG_DIM / PG_LANES;                 // channel groups
constexpr int PG_T = 4;                                  // a tile is PG_T x PG_T positions
constexpr int PG_R = PG_T + 6;                           // and reads PG_R x PG_R
constexpr int PG_SLOTS = 50;                             // 49 entries of G and the bias sum
constexpr int PG_BWD_WAVES = 2;                          // waves of a backward workgroup: they share a partial block
constexpr int PG_BWD_THREADS = PG_BWD_WAVES * PG_LANES;
constexpr int64_t PG_MAX_POS = (int64_t)1 << 22;
constexpr int64_t PG_POS_PER_BLOCK = 128;                // positions per partial block, at least

int64_t pg_tiles(int H, int W) { return (int64_t)((H + PG_T - 1) / PG_T) * ((W + PG_T - 1) / PG_T); }
// tiles per partial block: H W / 128 blocks at the most (and one at the least), so that the workspace stays below
// 1,600 bytes per position -- and below 2 MiB while H W < 1,024
int64_t pg_tiles_per_block(int H, int W) {
    const int64_t tiles = pg_tiles(H, W), pos = (int64_t)H * W;
    const int64_t most = pos / PG_POS_PER_BLOCK > 1 ? pos / PG_POS_PER_BLOCK : 1;
    return (tiles + most - 1) / most;
}
int64_t pg_blocks(int H, int W) {
    const int64_t tpb = pg_tiles_per_block(H, W);
    return (pg_tiles(H, W) + tpb - 1) / tpb;
}
size_t pg_ws_bytes(int H, int W) { return (size_t)pg_blocks(H, W) * PG_SLOTS * PG_DIM * sizeof(double); }
bool pg_shape_ok(int H, int W, int dim) { return dim == PG_DIM && H >= 1 && W >= 1 && (int64_t)H * W <= PG_MAX_POS; }

// the merged table of channel c; REVERSED: read backwards, w[6 - i][6 - j] at [i][j]
template <bool REVERSED>
__device__ __forceinline__ void pg_table(const float* w7, const float* w5, const float* w3, int c, float (&w)[49]) {
    float a7[49], a5[25], a3[9];
#pragma unroll
    for (int t = 0; t < 49; ++t) a7[t] = w7[c * 49 + t];
#pragma unroll
    for (int t = 0; t < 25; ++t) a5[t] = w5[c * 25 + t];
#pragma unroll
    for (int t = 0; t < 9; ++t) a3[t] = w3[c * 9 + t];
#pragma unroll
    for (int i = 0; i < 7; ++i)
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            float v = a7[i * 7 + j];
            if (i >= 1 && i <= 5 && j >= 1 && j <= 5) v = v + a5[(i - 1) * 5 + (j - 1)];
            if (i >= 2 && i <= 4 && j >= 2 && j <= 4) v = v + a3[(i - 2) * 3 + (j - 2)];
            w[REVERSED ? 48 - (i * 7 + j) : i * 7 + j] = v;
        }
}

// A tile's values are requested in one batch and made zero outside the square afterwards, with the caller's scheduling
// barrier between the two: otherwise the compiler, to save registers, waits for each value in turn.
// pg_request_halo: the 10 x 10 values of `src` around the tile at (y0, x0), channel c: [i][j] is position (y0 - 3 + i,
// x0 - 3 + j).  src points at token 1's row.  Every load is of a position inside: the coordinates are clamped to the square
// (min and max, no branch: the tile's own first position is inside).
__device__ __forceinline__ void pg_request_halo(const float* src, int H, int W, int y0, int x0, unsigned c, float (&v)[PG_R][PG_R]) {
#pragma unroll
    for (int i = 0; i < PG_R; ++i) {
        const int64_t row0 = (int64_t)min(max(y0 - 3 + i, 0), H - 1) * W;
#pragma unroll
        for (int j = 0; j < PG_R; ++j) {
            const float* row = src + (row0 + min(max(x0 - 3 + j, 0), W - 1)) * PG_DIM;   // (the same for every lane)
            v[i][j] = row[c];
        }
    }
}
// all ones if `in`, else zero, in a scalar register the optimiser cannot see through: were the zeroing a select on a
// condition it knows to be the same for every lane, it would move the load itself behind a branch on that condition, and the
// loads of a tile would no longer be one batch
__device__ __forceinline__ unsigned pg_mask(bool in) {
    unsigned m = __builtin_amdgcn_readfirstlane(in ? 0xffffffffu : 0u);
    asm("" : "+s"(m));
    return m;
}
__device__ __forceinline__ void pg_zero_halo(int H, int W, int y0, int x0, float (&v)[PG_R][PG_R]) {
    unsigned rm[PG_R], cm[PG_R];
#pragma unroll
    for (int i = 0; i < PG_R; ++i) {
        rm[i] = pg_mask(y0 - 3 + i >= 0 && y0 - 3 + i < H);
        cm[i] = pg_mask(x0 - 3 + i >= 0 && x0 - 3 + i < W);
    }
#pragma unroll
    for (int i = 0; i < PG_R; ++i)
#pragma unroll
        for (int j = 0; j < PG_R; ++j) v[i][j] = __uint_as_float(__float_as_uint(v[i][j]) & (rm[i] & cm[j]));
}

// the same for the tile's own PG_T x PG_T values
__device__ __forceinline__ void pg_request_tile(const float* src, int H, int W, int y0, int x0, unsigned c, float (&v)[PG_T][PG_T]) {
#pragma unroll
    for (int i = 0; i < PG_T; ++i) {
        const int64_t row0 = (int64_t)min(y0 + i, H - 1) * W;
#pragma unroll
        for (int j = 0; j < PG_T; ++j) {
            const float* row = src + (row0 + min(x0 + j, W - 1)) * PG_DIM;
            v[i][j] = row[c];
        }
    }
}
__device__ __forceinline__ void pg_zero_tile(int H, int W, int y0, int x0, float (&v)[PG_T][PG_T]) {
    unsigned rm[PG_T], cm[PG_T];
#pragma unroll
    for (int i = 0; i < PG_T; ++i) {
        rm[i] = pg_mask(y0 + i < H);
        cm[i] = pg_mask(x0 + i < W);
    }
#pragma unroll
    for (int i = 0; i < PG_T; ++i)
#pragma unroll
        for (int j = 0; j < PG_T; ++j) v[i][j] = __uint_as_float(__float_as_uint(v[i][j]) & (rm[i] & cm[j]));
}

// dst[p] = (centre + add) + sum_{i, j} w[i][j] v[p + (i, j)] for the tile's positions inside the square: one fp32 chain of
// 49 products per output
__device__ __forceinline__ void pg_conv_store(const float (&v)[PG_R][PG_R], const float (&w)[49], float add, float* dst, int H,
                                              int W, int y0, int x0, int c) {
#pragma unroll
    for (int oy = 0; oy < PG_T; ++oy)
#pragma unroll
        for (int ox = 0; ox < PG_T; ++ox) {
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < 7; ++i)
#pragma unroll
                for (int j = 0; j < 7; ++j) s = __builtin_fmaf(w[i * 7 + j], v[oy + i][ox + j], s);
            if (y0 + oy < H && x0 + ox < W)
                dst[((int64_t)(y0 + oy) * W + x0 + ox) * PG_DIM + c] = (v[oy + 3][ox + 3] + add) + s;
        }
}

// (two waves per SIMD: left alone the compiler keeps all 183 requested values apart and takes more than 256 registers)
__global__ __launch_bounds__(PG_LANES) __attribute__((amdgpu_waves_per_eu(2))) void ppeg_forward_kernel(
    const float* x, int H, int W, const float* w7, const float* b7, const float* w5, const float* b5, const float* w3,
    const float* b3, float* out) {
    const int c = (int)(blockIdx.x % PG_CG) * PG_LANES + threadIdx.x;      // channel groups fastest: the eight that read
    const int64_t tile = blockIdx.x / PG_CG;                               // adjacent 256 bytes of the same rows side by side
    const int tw = (W + PG_T - 1) / PG_T;
    const int y0 = __builtin_amdgcn_readfirstlane((int)(tile / tw) * PG_T);     // (the same for every lane: scalar registers)
    const int x0 = __builtin_amdgcn_readfirstlane((int)(tile % tw) * PG_T);
    float v[PG_R][PG_R], w[49];
    pg_request_halo(x + PG_DIM, H, W, y0, x0, c, v);
    pg_table<false>(w7, w5, w3, c, w);
    const float bias = (b7[c] + b5[c]) + b3[c];
    __builtin_amdgcn_sched_barrier(0);
    pg_zero_halo(H, W, y0, x0, v);
    if (tile == 0) out[c] = x[c];
    pg_conv_store(v, w, bias, out + PG_DIM, H, W, y0, x0, c);
}

struct PpegBwdArgs {
    const float* x;
    const float* w7;
    const float* w5;
    const float* w3;
    const float* dout;
    float* dx;
    double* part;          // [blocks][50][512]
    int H, W;
    int64_t tiles, tiles_per_block;
};

__global__ __launch_bounds__(PG_BWD_THREADS) __attribute__((amdgpu_waves_per_eu(2))) void ppeg_backward_kernel(PpegBwdArgs a) {
    __shared__ double sums[PG_BWD_WAVES][PG_SLOTS][PG_LANES];              // a lane adds to its own column of its wave's sums
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = (int)(blockIdx.x % PG_CG) * PG_LANES + lane;
    const int64_t block = blockIdx.x / PG_CG;
    const int H = a.H, W = a.W, tw = (W + PG_T - 1) / PG_T;
    const int64_t t0 = block * a.tiles_per_block;
    const int64_t t1 = t0 + a.tiles_per_block < a.tiles ? t0 + a.tiles_per_block : a.tiles;
    float w[49];
    pg_table<true>(a.w7, a.w5, a.w3, c, w);
    if (block == 0 && wave == 0) a.dx[c] = a.dout[c];
#pragma unroll
    for (int s = 0; s < PG_SLOTS; ++s) sums[wave][s][lane] = 0.0;
    for (int64_t tile = t0 + wave; tile < t1; tile += PG_BWD_WAVES) {      // the block's tiles in turn among the waves
        const int y0 = __builtin_amdgcn_readfirstlane((int)(tile / tw) * PG_T);
        const int x0 = __builtin_amdgcn_readfirstlane((int)(tile % tw) * PG_T);
        float d[PG_R][PG_R], xv[PG_T][PG_T];
        pg_request_halo(a.dout + PG_DIM, H, W, y0, x0, c, d);
        pg_request_tile(a.x + PG_DIM, H, W, y0, x0, c, xv);
        __builtin_amdgcn_sched_barrier(0);
        pg_zero_halo(H, W, y0, x0, d);
        pg_zero_tile(H, W, y0, x0, xv);
        pg_conv_store(d, w, 0.f, a.dx + PG_DIM, H, W, y0, x0, c);
        // G[i][j] += sum_q x[q] dout[q - (i - 3, j - 3)]: q = (qy, qx) of the tile is d[qy + 3][qx + 3].  One fp32 chain
        // of 16 products, then double; one entry at a time, so that no fp32 sum lives across tiles
#pragma unroll
        for (int i = 0; i < 7; ++i)
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                float s = 0.f;
#pragma unroll
                for (int qy = 0; qy < PG_T; ++qy)
#pragma unroll
                    for (int qx = 0; qx < PG_T; ++qx) s = __builtin_fmaf(xv[qy][qx], d[qy + 6 - i][qx + 6 - j], s);
                sums[wave][i * 7 + j][lane] += (double)s;
            }
        float gb = 0.f;
#pragma unroll
        for (int qy = 0; qy < PG_T; ++qy)
#pragma unroll
            for (int qx = 0; qx < PG_T; ++qx) gb = gb + d[qy + 3][qx + 3];
        sums[wave][49][lane] += (double)gb;
    }
    __syncthreads();
    if (wave == 0) {                                                       // the waves' sums in index order
        double* p = a.part + block * (PG_SLOTS * PG_DIM) + c;
#pragma unroll
        for (int s = 0; s < PG_SLOTS; ++s) {
            double v = sums[0][s][lane];
#pragma unroll
            for (int k = 1; k < PG_BWD_WAVES; ++k) v += sums[k][s][lane];
            p[s * PG_DIM] = v;
        }
    }
}

// one thread per (slot, channel): the blocks' partial sums in index order, sixteen loads at a time (past the last block the
// last one is read again and counts as zero), rounded to fp32 once; slot 7 i + j is G[i][j], slot 49 the bias sum
__global__ __launch_bounds__(256) void ppeg_backward_merge_kernel(const double* part, int64_t blocks, float* dw7, float* db7,
                                                                  float* dw5, float* db5, float* dw3, float* db3) {
    const int slot = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    const double* p = part + slot * PG_DIM + c;
    double s = 0.0;
    for (int64_t k = 0; k < blocks; k += 16) {
        double x[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) x[j] = p[(k + j < blocks ? k + j : blocks - 1) * (PG_SLOTS * PG_DIM)];
#pragma unroll
        for (int j = 0; j < 16; ++j) s += k + j < blocks ? x[j] : 0.0;
    }
    const float r = (float)s;
    if (slot == 49) {
        db7[c] = r; db5[c] = r; db3[c] = r;
        return;
    }
    const int i = slot / 7, j = slot % 7;
    dw7[c * 49 + slot] = r;
    if (i >= 1 && i <= 5 && j >= 1 && j <= 5) dw5[c * 25 + (i - 1) * 5 + (j - 1)] = r;
    if (i >= 2 && i <= 4 && j >= 2 && j <= 4) dw3[c * 9 + (i - 2) * 3 + (j - 2)] = r;
}

bool pg_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool pg_overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bytes && y < x + bytes;
}

int pg_check_shape(const char* fn, int H, int W, int dim) {
    if (dim != PG_DIM) MOC_FAIL(MOC_EUNSUPPORTED, "%s: dim=%d, only 512 is built", fn, dim);
    MOC_REQUIRE(H >= 1 && W >= 1, "%s: H=%d W=%d must be at least 1", fn, H, W);
    MOC_REQUIRE((int64_t)H * W <= PG_MAX_POS, "%s: H=%d W=%d, H W above %lld", fn, H, W, (long long)PG_MAX_POS);
    return MOC_OK;
}

}  // namespace

extern "C" int moc_ppeg_forward(const float* x, int H, int W, int dim, const float* w7, const float* b7, const float* w5,
                                const float* b5, const float* w3, const float* b3, float* out, moc_stream_t stream) {
    const char* fn = "moc_ppeg_forward";
    MOC_REQUIRE(x && w7 && b7 && w5 && b5 && w3 && b3, "%s: a null input (x, w7, b7, w5, b5, w3, b3)", fn);
    MOC_REQUIRE(out, "%s: out is null", fn);
    if (const int rc = pg_check_shape(fn, H, W, dim)) return rc;
    MOC_REQUIRE(pg_aligned(x) && pg_aligned(w7) && pg_aligned(b7) && pg_aligned(w5) && pg_aligned(b5) && pg_aligned(w3) &&
                    pg_aligned(b3) && pg_aligned(out),
                "%s: every pointer must be 16-byte aligned", fn);
    const size_t bytes = ((size_t)H * W + 1) * PG_DIM * sizeof(float);
    MOC_REQUIRE(!pg_overlap(x, out, bytes), "%s: out overlaps x (the halo is read after neighbours are written)", fn);
    const int64_t tiles = pg_tiles(H, W);                                  // at most 2^22 (H = 1): 2^25 workgroups
    ppeg_forward_kernel<<<(unsigned)(tiles * PG_CG), PG_LANES, 0, (hipStream_t)stream>>>(x, H, W, w7, b7, w5, b5, w3, b3, out);
    MOC_CHECK_LAUNCH(fn);
    return MOC_OK;
}

extern "C" size_t moc_ppeg_backward_workspace(int H, int W, int dim) { return pg_shape_ok(H, W, dim) ? pg_ws_bytes(H, W) : 0; }

extern "C" int moc_ppeg_backward(const float* x, int H, int W, int dim, const float* w7, const float* w5, const float* w3,
                                 const float* dout, float* dx, float* dw7, float* db7, float* dw5, float* db5, float* dw3,
                                 float* db3, void* ws, size_t ws_bytes, moc_stream_t stream) {
    const char* fn = "moc_ppeg_backward";
    MOC_REQUIRE(x && w7 && w5 && w3 && dout, "%s: a null input (x, w7, w5, w3, dout)", fn);
    MOC_REQUIRE(dx && dw7 && db7 && dw5 && db5 && dw3 && db3, "%s: a null output (dx, dw7, db7, dw5, db5, dw3, db3)", fn);
    MOC_REQUIRE(ws, "%s: ws is null", fn);
    if (const int rc = pg_check_shape(fn, H, W, dim)) return rc;
    MOC_REQUIRE(pg_aligned(x) && pg_aligned(w7) && pg_aligned(w5) && pg_aligned(w3) && pg_aligned(dout) && pg_aligned(dx) &&
                    pg_aligned(dw7) && pg_aligned(db7) && pg_aligned(dw5) && pg_aligned(db5) && pg_aligned(dw3) &&
                    pg_aligned(db3) && pg_aligned(ws),
                "%s: every pointer must be 16-byte aligned", fn);
    const size_t bytes = ((size_t)H * W + 1) * PG_DIM * sizeof(float);
    MOC_REQUIRE(!pg_overlap(dout, dx, bytes) && !pg_overlap(x, dx, bytes),
                "%s: dx overlaps dout or x (the halo is read after neighbours are written)", fn);
    MOC_REQUIRE(ws_bytes >= pg_ws_bytes(H, W), "%s: ws_bytes=%zu, need %zu", fn, ws_bytes, pg_ws_bytes(H, W));
    hipStream_t s = (hipStream_t)stream;
    PpegBwdArgs a;
    a.x = x; a.w7 = w7; a.w5 = w5; a.w3 = w3; a.dout = dout; a.dx = dx; a.part = (double*)ws; a.H = H; a.W = W;
    a.tiles = pg_tiles(H, W); a.tiles_per_block = pg_tiles_per_block(H, W);
    const int64_t blocks = pg_blocks(H, W);                                // at most 2^22 / 128 = 32,768
    ppeg_backward_kernel<<<(unsigned)(blocks * PG_CG), PG_BWD_THREADS, 0, s>>>(a);
    MOC_CHECK_LAUNCH(fn);
    ppeg_backward_merge_kernel<<<dim3(PG_DIM / 256, PG_SLOTS), 256, 0, s>>>(a.part, blocks, dw7, db7, dw5, db5, dw3, db3);
    MOC_CHECK_LAUNCH(fn);
    return MOC_OK;
}
