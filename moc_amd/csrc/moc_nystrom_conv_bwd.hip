// Backward of kernel B's residual convolution (moc_nystrom.hip: nystrom_token_kernel; moc_amd/nystrom.py:
// TokenValuesResidual; DESIGN.md section 8c, "the residual convolution's gradients").  With the forward
//       out[i, 64 h + d] += sum_t w[h, t] v[i + t - taps / 2, h, d]            (rows outside [0, n_pad) count as zero)
// and dout [n_pad, 512]:
//       dv[j, h, d] = sum_t w[h, t] dout[j - t + taps / 2, h, d]
//       dw[h, t]    = sum_i sum_d dout[i, h, d] v[i + t - taps / 2, h, d]
//
// One kernel forms both.  A workgroup is one head x 128 tokens, four waves, a wave per 16-token tile, two tiles each, on
// the forward's lane conventions (moc_nystrom.hip's header: v_mfma_f32_16x16x4_f32, lane l = (g = l >> 4, c = l & 15) holds
// A[c][g] and B[g][c], the result has column c and rows 4 g + r in register r).
//   dv: kernel B's 12 steps over the 48 rows around the tile, applied to dout instead of v, against the banded matrix
//       T'[i', j] = w[j - i' + taps / 2]: the forward's table read backwards.  Step st, slot g = row tok0 - 16 + 4 st + g: a
//       lane loads float4 4 c of that row (four whole 256-byte rows per instruction); output tile dt holds feature
//       16 g + 4 r + dt of token c, so a lane stores four float4 into the v columns of dqkv.
//   dw: G[i', i] = sum_d v[i', d] dout[i, d] for the 48 rows i' and the 16 tokens i, three 16 x 16 blocks of 16 steps each
//       (slot g of step s = feature 16 g + s: one fp32 chain over the 64 features per entry); the tap gradients are the
//       33 diagonals i' - i = -16 .. 16 of G.  Both operands want a lane to hold 16 features of ITS row, which from memory
//       would be 16-byte pieces of 16 rows per instruction, so they come through LDS: the workgroup first lays the 160 rows
//       of v around its tokens out row-major with rows of 68 floats (moc_nystrom_bwd.hip's image; rows outside the sequence
//       as zeros), and a wave passes its tile's own 16 rows of dout, which it holds for the dv steps 4 .. 7, through a
//       16-row image of its own.  Nothing longer than the 64-product chain is summed in fp32: each lane adds its 12 entries
//       of G into 12 doubles across its tiles, the workgroup adds the four waves' sums and then the 16 entries of each
//       diagonal through LDS, in double and in a fixed order, and leaves 33 doubles per head and 128-token block in the
//       workspace.  A merge launch adds the blocks in index order and rounds to fp32 once.
// A thread requests all it reads from memory (24 float4 of dout, 10 of v) before it waits for any of it: with two
// workgroups to a compute unit (61 KB of LDS each) there is little else to hide the latency behind.
// No atomics: two calls give the same bits.  Every load is of a row inside [0, n_pad): a halo row outside reads a row of
// the workgroup's own tokens instead and is replaced by zeros.
#include "moc_nystrom_shared.h"

namespace {

constexpr int NYC_THREADS = 256;                         // four waves
constexpr int NYC_WAVES = NYC_THREADS / 64;
constexpr int NYC_TOK = 128;                             // tokens per workgroup: two 16-token tiles per wave
constexpr int NYC_ROWS = 48;                             // the rows tok0 - 16 .. tok0 + 31 around a 16-token tile
constexpr int NYC_SLOTS = 33;                            // tap offsets i' - i = -16 .. 16, whatever `taps` is
constexpr int NYC_LDW = NY_D + 4;                        // floats per row of an LDS image
constexpr int NYC_VROWS = NYC_TOK + 32;                  // the workgroup's tokens and 16 halo rows on either side
constexpr int NYC_VIMG = NYC_VROWS * NYC_LDW;            // floats: the v image, later the waves' double sums
constexpr int NYC_DIMG = 16 * NYC_LDW;                   // floats: one wave's dout image
constexpr int NYC_TPW = NYC_TOK / 16 / NYC_WAVES;        // tiles per wave
constexpr int NYC_VSHARE = NYC_VROWS * (NY_D / 4) / NYC_THREADS;   // float4 of the v image per thread
static_assert(NYC_VSHARE * NYC_THREADS == NYC_VROWS * (NY_D / 4), "the v image divides among the threads");
static_assert(NYC_WAVES * NYC_ROWS * 16 * sizeof(double) <= NYC_VIMG * sizeof(float), "the sums reuse the v image");
static_assert(NY_B_TOK % NYC_TOK == 0 && (NYC_TOK / 16) % NYC_WAVES == 0, "whole workgroups, the same trips for every wave");

int64_t nyc_blocks(int64_t n_pad) { return n_pad / NYC_TOK; }
size_t nyc_ws_bytes(int64_t n_pad) { return (size_t)NY_HEADS * (size_t)nyc_blocks(n_pad) * NYC_SLOTS * sizeof(double); }

struct NyConvArgs {
    const float* qkv;      // [n_pad, 1536]
    const float* conv_w;   // [8, taps]
    const float* dout;     // [n_pad, 512]
    float* dqkv;           // [n_pad, 1536]: the v columns are written
    double* part;          // [8, n_pad / 128, 33]
    int64_t n_pad;
    int taps;
};

__device__ __forceinline__ void nyc_ld16(const float* p, float* o) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 v = ny_ld4(p + 4 * j);
        o[4 * j] = v.x; o[4 * j + 1] = v.y; o[4 * j + 2] = v.z; o[4 * j + 3] = v.w;
    }
}

__global__ __launch_bounds__(NYC_THREADS) void nystrom_conv_bwd_kernel(NyConvArgs a) {
    __shared__ __attribute__((aligned(16))) float smem[NYC_VIMG + NYC_WAVES * NYC_DIMG + 64];
    float* vimg = smem;                                              // [160][68]: row tok_base - 16 + row of v
    float* wt = smem + NYC_VIMG + NYC_WAVES * NYC_DIMG;              // wt[32 + i' - j] = w[j - i' + taps / 2], or 0
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    float* dimg = smem + NYC_VIMG + wave * NYC_DIMG;                 // [16][68]: this wave's tile of dout
    const int h = blockIdx.x;                                        // heads fastest: a token block's eight heads, which read
    const int64_t tok_base = (int64_t)blockIdx.y * NYC_TOK;          // adjacent 256 bytes of the same rows, run side by side
    // everything this thread reads from memory is requested before anything is waited for: the 48 rows of dout around each
    // of its wave's tiles, and its share of the 160 rows of v
    float4 dreg[NYC_TPW][12], vreg[NYC_VSHARE];
#pragma unroll
    for (int k = 0; k < NYC_TPW; ++k)
#pragma unroll
        for (int st = 0; st < 12; ++st) {                            // step st, slot g = row tok0 - 16 + 4 st + g
            const int64_t tok0 = tok_base + (wave + k * NYC_WAVES) * 16, tp = tok0 - 16 + 4 * st + g;
            const bool in = tp >= 0 && tp < a.n_pad;
            dreg[k][st] = ny_ld4(a.dout + (in ? tp : tok0) * NY_OUT + 64 * h + 4 * c);
            if (!in) dreg[k][st] = float4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
    for (int k = 0; k < NYC_VSHARE; ++k) {
        const int idx = threadIdx.x + k * NYC_THREADS, row = idx >> 4, c4 = idx & 15;
        const int64_t tp = tok_base - 16 + row;
        const bool in = tp >= 0 && tp < a.n_pad;
        vreg[k] = ny_ld4(a.qkv + (in ? tp : tok_base) * NY_ROW + 1024 + 64 * h + 4 * c4);
        if (!in) vreg[k] = float4{0.f, 0.f, 0.f, 0.f};
    }
    if (threadIdx.x < 64) {
        const int tap = a.taps / 2 - ((int)threadIdx.x - 32);
        wt[threadIdx.x] = tap >= 0 && tap < a.taps ? a.conv_w[h * a.taps + tap] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < NYC_VSHARE; ++k) {
        const int idx = threadIdx.x + k * NYC_THREADS, row = idx >> 4, c4 = idx & 15;
        *reinterpret_cast<float4*>(vimg + row * NYC_LDW + 4 * c4) = vreg[k];
    }
    const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
    double gsum[3][4];                                               // G[16 b + 4 g + r][c], summed over this wave's tiles
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) gsum[b][r] = 0.0;
#pragma unroll
    for (int k = 0; k < NYC_TPW; ++k) {                              // (every wave makes the same trips: the barriers match)
        const int tile = wave + k * NYC_WAVES;
        const int64_t tok0 = tok_base + tile * 16;
#pragma unroll
        for (int st = 4; st < 8; ++st)                               // the tile's own rows tok0 + 4 (st - 4) + g
            *reinterpret_cast<float4*>(dimg + (4 * (st - 4) + g) * NYC_LDW + 4 * c) = dreg[k][st];
        __syncthreads();                                             // the tap table, the v image, this tile's dout image
        // dv^T = dout^T T'
        f32x4_t o[4] = {zero4, zero4, zero4, zero4};
#pragma unroll
        for (int st = 0; st < 12; ++st) {
            const float4 d4 = dreg[k][st];
            const float b = wt[32 + (4 * st + g - 16) - c];
            o[0] = ny_mfma(d4.x, b, o[0]); o[1] = ny_mfma(d4.y, b, o[1]);
            o[2] = ny_mfma(d4.z, b, o[2]); o[3] = ny_mfma(d4.w, b, o[3]);
        }
        float* op = a.dqkv + (tok0 + c) * NY_ROW + 1024 + 64 * h + 16 * g;
#pragma unroll
        for (int r = 0; r < 4; ++r) *reinterpret_cast<float4*>(op + 4 * r) = float4{o[0][r], o[1][r], o[2][r], o[3][r]};
        // G = v dout^T, block by block: A = v[row tok0 - 16 + 16 b + c][16 g + s], B = dout[token c][16 g + s]
        float db[16];
        nyc_ld16(dimg + c * NYC_LDW + 16 * g, db);
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            float vb[16];
            nyc_ld16(vimg + (tile * 16 + 16 * b + c) * NYC_LDW + 16 * g, vb);
            f32x4_t G = zero4;
#pragma unroll
            for (int s = 0; s < 16; ++s) G = ny_mfma(vb[s], db[s], G);
#pragma unroll
            for (int r = 0; r < 4; ++r) gsum[b][r] += (double)G[r];
        }
        __syncthreads();                                             // both images are read before either is written again
    }
    // the four waves' sums entry by entry, then each diagonal's 16 entries, both in index order; the v image is done with
    double* gd = reinterpret_cast<double*>(smem);                    // [wave][48][16]
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) gd[(wave * NYC_ROWS + 16 * b + 4 * g + r) * 16 + c] = gsum[b][r];
    __syncthreads();
    for (int e = threadIdx.x; e < NYC_ROWS * 16; e += NYC_THREADS) {
        double s = gd[e];
        for (int w = 1; w < NYC_WAVES; ++w) s += gd[w * NYC_ROWS * 16 + e];
        gd[e] = s;
    }
    __syncthreads();
    if (threadIdx.x < NYC_SLOTS) {                                   // offset i' - i = threadIdx.x - 16: row i + threadIdx.x
        double s = 0.0;
        for (int i = 0; i < 16; ++i) s += gd[(i + threadIdx.x) * 16 + i];
        a.part[((int64_t)h * gridDim.y + blockIdx.y) * NYC_SLOTS + threadIdx.x] = s;
    }
}

// one thread per (head, tap): the blocks' partial sums in index order, sixteen loads at a time (past the last block the
// last one is read again and counts as zero), rounded to fp32 once
__global__ __launch_bounds__(64) void nystrom_conv_bwd_merge_kernel(const double* part, int blocks, int taps, float* dconv_w) {
    const int h = blockIdx.x, t = threadIdx.x;
    if (t >= taps) return;
    const double* p = part + (int64_t)h * blocks * NYC_SLOTS + (t - taps / 2 + 16);
    double s = 0.0;
    for (int k = 0; k < blocks; k += 16) {
        double x[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) x[j] = p[(int64_t)(k + j < blocks ? k + j : blocks - 1) * NYC_SLOTS];
#pragma unroll
        for (int j = 0; j < 16; ++j) s += k + j < blocks ? x[j] : 0.0;
    }
    dconv_w[h * taps + t] = (float)s;
}

bool nyc_taps_ok(int taps) { return taps >= 1 && (taps & 1) && taps <= NY_MAX_TAPS; }

}  // namespace

extern "C" size_t moc_nystrom_conv_backward_workspace(int64_t n_pad, int heads, int dim_head, int landmarks, int taps) {
    return ny_shape_ok(n_pad, heads, dim_head, landmarks) && nyc_taps_ok(taps) ? nyc_ws_bytes(n_pad) : 0;
}

extern "C" int moc_nystrom_conv_backward(const float* qkv, int64_t n_pad, int heads, int dim_head, int landmarks,
                                         const float* conv_w, int taps, const float* dout, float* dqkv, float* dconv_w,
                                         void* ws, size_t ws_bytes, moc_stream_t stream) {
    const char* fn = "moc_nystrom_conv_backward";
    MOC_REQUIRE(qkv && conv_w && dout, "%s: a null input (qkv, conv_w, dout)", fn);
    MOC_REQUIRE(dqkv && dconv_w, "%s: a null output (dqkv, dconv_w)", fn);
    MOC_REQUIRE(ws, "%s: ws is null", fn);
    if (const int rc = ny_check_shape(fn, n_pad, heads, dim_head, landmarks)) return rc;
    MOC_REQUIRE(taps >= 1 && (taps & 1), "%s: taps=%d must be odd", fn, taps);
    if (taps > NY_MAX_TAPS) MOC_FAIL(MOC_EUNSUPPORTED, "%s: taps=%d above 33", fn, taps);
    MOC_REQUIRE(ny_aligned(qkv) && ny_aligned(conv_w) && ny_aligned(dout) && ny_aligned(dqkv) && ny_aligned(dconv_w) && ny_aligned(ws),
                "%s: every pointer must be 16-byte aligned", fn);
    MOC_REQUIRE(ws_bytes >= nyc_ws_bytes(n_pad), "%s: ws_bytes=%zu, need %zu", fn, ws_bytes, nyc_ws_bytes(n_pad));
    hipStream_t s = (hipStream_t)stream;
    NyConvArgs a;
    a.qkv = qkv; a.conv_w = conv_w; a.dout = dout; a.dqkv = dqkv; a.part = (double*)ws; a.n_pad = n_pad; a.taps = taps;
    const int blocks = (int)nyc_blocks(n_pad);
    nystrom_conv_bwd_kernel<<<dim3(NY_HEADS, (unsigned)blocks), NYC_THREADS, 0, s>>>(a);      // blocks <= 2^22 / 128 = 32,768
    MOC_CHECK_LAUNCH(fn);
    nystrom_conv_bwd_merge_kernel<<<NY_HEADS, 64, 0, s>>>(a.part, blocks, taps, dconv_w);
    MOC_CHECK_LAUNCH(fn);
    return MOC_OK;
}
