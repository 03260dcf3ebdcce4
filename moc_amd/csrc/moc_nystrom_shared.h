// What the Nystrom forward (moc_nystrom.hip) and backward (moc_nystrom_bwd.hip) share: the one built shape, the qkv
// layout, the f32 MFMA step and its per-column reductions, and the host-side shape refusals.
#pragma once
#include "moc_common.h"
#include <cmath>

namespace {

constexpr int NY_HEADS = 8, NY_D = 64, NY_M = 256, NY_MAX_TAPS = 33;
constexpr int NY_ROW = 3 * NY_HEADS * NY_D;              // 1536 floats per token of qkv
constexpr int NY_OUT = NY_HEADS * NY_D;                  // 512 floats per token of out
constexpr int NY_CHUNK = 512;                            // tokens per partial range of the landmark-parallel kernels
constexpr int NY_B_TOK = 256;                            // tokens per workgroup of the token-parallel kernels
constexpr int64_t NY_MAX_N = (int64_t)1 << 22;

int64_t ny_chunks(int64_t n_pad) { return (n_pad + NY_CHUNK - 1) / NY_CHUNK; }
bool ny_shape_ok(int64_t n_pad, int heads, int dim_head, int landmarks) {
    return heads == NY_HEADS && dim_head == NY_D && landmarks == NY_M && n_pad >= NY_M && n_pad % NY_M == 0 && n_pad <= NY_MAX_N;
}

__device__ __forceinline__ f32x4_t ny_mfma(float a, float b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float4 ny_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float ny_col_max(float v) {                 // over the four lanes that share a column
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float ny_col_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

int ny_check_shape(const char* fn, int64_t n_pad, int heads, int dim_head, int landmarks) {
    if (heads != NY_HEADS || dim_head != NY_D || landmarks != NY_M)
        MOC_FAIL(MOC_EUNSUPPORTED, "%s: heads=%d dim_head=%d landmarks=%d, only 8 x 64 with 256 landmarks is built", fn, heads,
                 dim_head, landmarks);
    MOC_REQUIRE(n_pad >= landmarks && n_pad % landmarks == 0, "%s: n_pad=%lld must be a positive multiple of landmarks=%d", fn,
                (long long)n_pad, landmarks);
    if (n_pad > NY_MAX_N) MOC_FAIL(MOC_EUNSUPPORTED, "%s: n_pad=%lld above %lld", fn, (long long)n_pad, (long long)NY_MAX_N);
    return MOC_OK;
}

bool ny_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
