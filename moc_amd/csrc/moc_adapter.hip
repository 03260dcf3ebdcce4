// Fused adapter forward (reference models/model_adapters.py:185-193 Conch_CLIP_Ada.forward,
// :330-405 Conch_MOE_CLIP_Ada.forward with the soft router): one pass over a bag X [N, 512] -> logits [N, C].
//
//   unit(v) = v / ||v||   (a division: a zero row gives NaN, as torch does)
//   E = 1 ("clip"):  a = relu(W2 relu(W1 x));  m = r a + (1 - r) x;  logits = unit(m) Wc
//   E >= 2 ("moe"):  f = unit(x);  w = softmax_E(G f);  a_e = relu(W2_e relu(W1_e f));  s = unit(sum_e w_e a_e);
//                    logits = unit(r s + (1 - r) f) Wc
//
// A wave owns 16 rows from the load of the bag to the store of the logits; nothing but the weights is shared and there is
// no barrier (LDS only parks each lane's own share of the rows).  Both GEMMs run TRANSPOSED on the bf16 matrix cores --
// out^T = W act^T: the weights are the A
// operand (16 output features x 32 of K), the activations the B operand (32 of K x 16 rows) -- with fp32-exact products as
// in moc_attn.hip: each operand is three bf16 terms (hi + mid + lo == the fp32 value) and the six products down to 2^-16 of
// the leading one are accumulated in fp32.  An MFMA result holds, in lane (row = lane & 15, q = lane >> 4), the four output
// features 16 t + 4 q + 0..3 of that row; the 32 K-slots of an MFMA may be assigned to K indices freely as long as both
// operands agree, so slot (q, j) of K-step s stands for index 32 s + 16 (j >> 2) + 4 q + (j & 3): the results of two adjacent
// output tiles ARE the B operand of the next GEMM's K-step, in registers.  The same assignment is used for the bag itself, so
// the value x[row][c] a lane loaded (two float4 per K-step) sits in the lane that later holds the adapter's output for
// (row, c): the mix, the norms (lane sums + two cross-lane steps), the router and the classifier product are lane-local.
// The [N, 128] hidden, the [N, 512] adapter outputs and the [N, 512, E] stack never exist outside registers.
//
// The weights come from an image a first launch builds on every call (no cache: an in-place write to a parameter must be
// seen): per expert [K-step 16][hidden tile 8][term 3][lane 64] x 16 B for W1, [output tile 32][K-step 4][term 3][lane 64]
// x 16 B for W2 (768 KiB), then the classifier transposed, [C][512] fp32.  Every wave reads each fragment once per expert,
// straight from the cache hierarchy (the four waves of a workgroup walk the image together).
//
// Bound: 4 N c h E 6 flops on the bf16 matrix pipe (N = 15,000: 9 us at E = 1, 47 us at E = 5) against 6 us of HBM time for
// the bag; one weight fragment feeds one MFMA row tile here, so the fragment stream (32 B / clock / wave) and not the matrix
// pipe is what a wave waits for.  Measured figures: DESIGN.md.
#include "moc_common.h"
#include <cmath>

namespace {

constexpr int AD_C = 512, AD_H = 128;
constexpr int AD_ROWS = 64;                      // rows per workgroup (16 per wave)
constexpr int AD_KS1 = AD_C / 32, AD_HT = AD_H / 16, AD_KS2 = AD_H / 32, AD_CT = AD_C / 16;
constexpr int AD_MAX_E = 8, AD_MAX_CLS = 64;
constexpr size_t AD_W1_FRAGS = (size_t)AD_KS1 * AD_HT * 3, AD_W2_FRAGS = (size_t)AD_CT * AD_KS2 * 3;    // 1 KiB each
constexpr size_t AD_EXPERT_BYTES = (AD_W1_FRAGS + AD_W2_FRAGS) * 1024;                                   // 768 KiB

size_t ad_ws_bytes(int E, int C) { return (size_t)E * AD_EXPERT_BYTES + (size_t)C * AD_C * sizeof(float); }

struct AdWeights { const float* W1[AD_MAX_E]; const float* W2[AD_MAX_E]; };

// K index of slot j (of eight) of lane group q in K-step s
__host__ __device__ constexpr int ad_kidx(int s, int q, int j) { return 32 * s + 16 * (j >> 2) + 4 * q + (j & 3); }

// One thread per (expert, matrix, fragment, lane): the three terms of eight weights.  Then the classifier, transposed.
__global__ __launch_bounds__(256) void adapter_image_kernel(AdWeights w, int E, const float* Wc, int C, uint4* img) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n_frag = (int64_t)E * 2 * 128 * 64;
    if (idx >= n_frag) {
        const int64_t t = idx - n_frag;
        if (t < (int64_t)C * AD_C) {
            float* WcT = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(img) + (size_t)E * AD_EXPERT_BYTES);
            const int k = (int)(t / AD_C), c = (int)(t % AD_C);
            WcT[t] = Wc[(int64_t)c * C + k];
        }
        return;
    }
    const int lane = (int)(idx & 63), f = (int)((idx >> 6) & 127), second = (int)((idx >> 13) & 1), e = (int)(idx >> 14);
    const int m = lane & 15, q = lane >> 4;
    const float* src;
    size_t dst;                                                       // in uint4 units
    if (!second) {
        const int s = f / AD_HT, ht = f % AD_HT;
        src = w.W1[e] + (int64_t)(16 * ht + m) * AD_C + ad_kidx(s, q, 0);
        dst = (size_t)(s * AD_HT + ht) * 3 * 64;
    } else {
        const int ct = f / AD_KS2, u = f % AD_KS2;
        src = w.W2[e] + (int64_t)(16 * ct + m) * AD_H + ad_kidx(u, q, 0);
        dst = (AD_W1_FRAGS + (size_t)(ct * AD_KS2 + u) * 3) * 64;
    }
    const float4 v0 = *reinterpret_cast<const float4*>(src), v1 = *reinterpret_cast<const float4*>(src + 16);
    const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    uint16_t hi[8], mid[8], lo[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) moc_split3<false>(v[j], 1.f, hi[j], mid[j], lo[j]);
    auto pack = [](const uint16_t (&t)[8]) {
        return uint4{(uint32_t)t[0] | ((uint32_t)t[1] << 16), (uint32_t)t[2] | ((uint32_t)t[3] << 16),
                     (uint32_t)t[4] | ((uint32_t)t[5] << 16), (uint32_t)t[6] | ((uint32_t)t[7] << 16)};
    };
    uint4* out = img + (size_t)e * (AD_EXPERT_BYTES / 16) + dst + lane;
    out[0] = pack(hi);
    out[64] = pack(mid);
    out[128] = pack(lo);
}

typedef unsigned __attribute__((ext_vector_type(4))) au32x4_t;
struct AdTerms { au32x4_t t[3]; };

// three bf16 terms of eight fp32 values (truncating split: v == hi + mid + lo exactly), packed in MFMA operand order
// (v_perm_b32 selector 0x07060302: the upper halves of (odd, even) side by side)
__device__ __forceinline__ void ad_split(const float (&v)[8], AdTerms& o) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const unsigned e0 = __float_as_uint(v[2 * p]), e1 = __float_as_uint(v[2 * p + 1]);
        const float r0 = v[2 * p] - __uint_as_float(e0 & 0xFFFF0000u), r1 = v[2 * p + 1] - __uint_as_float(e1 & 0xFFFF0000u);
        const unsigned r0b = __float_as_uint(r0), r1b = __float_as_uint(r1);
        const float l0 = r0 - __uint_as_float(r0b & 0xFFFF0000u), l1 = r1 - __uint_as_float(r1b & 0xFFFF0000u);
        o.t[0][p] = __builtin_amdgcn_perm(e1, e0, 0x07060302u);
        o.t[1][p] = __builtin_amdgcn_perm(r1b, r0b, 0x07060302u);
        o.t[2][p] = __builtin_amdgcn_perm(__float_as_uint(l1), __float_as_uint(l0), 0x07060302u);
    }
}

__device__ __forceinline__ f32x4_t ad_mfma(const au32x4_t& w, const au32x4_t& x, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, w), __builtin_bit_cast(bf16x8_t, x), c, 0, 0, 0);
}
__device__ __forceinline__ au32x4_t ad_load(const uint4* p) {
    const uint4 v = *p;
    return au32x4_t{v.x, v.y, v.z, v.w};
}
// twelve consecutive fragments of the image: four (hidden tile | K-step) x three terms
__device__ __forceinline__ void ad_load12(const uint4* p, au32x4_t (&w)[12]) {
#pragma unroll
    for (int i = 0; i < 12; ++i) w[i] = ad_load(p + 64 * i);
}
// The six products of four (weight fragment, activation fragment) pairs: weights w[3 i + term], activations x[i * XS];
// small products into sm[i * AS], large ones into lg[i * AS], the four pairs in turn (independent accumulators).
template <int XS, int AS>
__device__ __forceinline__ void ad_six4(const au32x4_t (&w)[12], const AdTerms* x, f32x4_t* sm, f32x4_t* lg) {
#pragma unroll
    for (int i = 0; i < 4; ++i) sm[i * AS] = ad_mfma(w[3 * i + 2], x[i * XS].t[0], sm[i * AS]);
#pragma unroll
    for (int i = 0; i < 4; ++i) lg[i * AS] = ad_mfma(w[3 * i + 1], x[i * XS].t[0], lg[i * AS]);
#pragma unroll
    for (int i = 0; i < 4; ++i) sm[i * AS] = ad_mfma(w[3 * i], x[i * XS].t[2], sm[i * AS]);
#pragma unroll
    for (int i = 0; i < 4; ++i) lg[i * AS] = ad_mfma(w[3 * i], x[i * XS].t[1], lg[i * AS]);
#pragma unroll
    for (int i = 0; i < 4; ++i) sm[i * AS] = ad_mfma(w[3 * i + 1], x[i * XS].t[1], sm[i * AS]);
#pragma unroll
    for (int i = 0; i < 4; ++i) lg[i * AS] = ad_mfma(w[3 * i], x[i * XS].t[0], lg[i * AS]);
}
// relu that keeps NaN (torch.relu does)
__device__ __forceinline__ float ad_relu(float v) { return v < 0.f ? 0.f : v; }
// sum over the four lanes that share a row (lane & 15): the same bits in all four
__device__ __forceinline__ float ad_row_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
// sum_j v[s][j]^2 over a lane's 128 values, then over the row
__device__ __forceinline__ float ad_row_sumsq(const float (&v)[AD_KS1][8]) {
    float p[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < AD_KS1; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) p[j & 3] = fmaf(v[s][j], v[s][j], p[j & 3]);
    return ad_row_sum((p[0] + p[1]) + (p[2] + p[3]));
}
// sum_c v[c] w[c] over the row; w points at this lane group's first column (+ 4 q) of a 512-vector
__device__ __forceinline__ float ad_row_dot(const float (&v)[AD_KS1][8], const float* w) {
    float p[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < AD_KS1; ++s)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const float4 g = *reinterpret_cast<const float4*>(w + 32 * s + 16 * hf);
            p[0] = fmaf(v[s][4 * hf + 0], g.x, p[0]); p[1] = fmaf(v[s][4 * hf + 1], g.y, p[1]);
            p[2] = fmaf(v[s][4 * hf + 2], g.z, p[2]); p[3] = fmaf(v[s][4 * hf + 3], g.w, p[3]);
        }
    return ad_row_sum((p[0] + p[1]) + (p[2] + p[3]));
}

struct AdArgs {
    const float* X;         // [N, 512]
    const uint4* img;       // adapter_image_kernel
    const float* G;         // [E, 512] (moe)
    float* logits;          // [N, C]
    int64_t N;
    int E, C;
    float r, one_minus_r;
};

constexpr int AD_SMEM = 4 * 2 * AD_KS1 * 64 * 16;                     // the four waves' rows: 128 KiB

// Every [row, 512] quantity of this kernel is laid out as v[s][j] = value[row][ad_kidx(s, q, j)].  The rows themselves
// (x, or f = unit(x)) wait in LDS, each lane's 128 values in slots of its own -- xl[64 k], k = 2 s + (j >> 2), one float4
// each: no lane reads what another wrote -- so that the K loop of the first product stays a loop.
template <bool MOE>
__global__ __launch_bounds__(256) void adapter_kernel(AdArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4;
    const int64_t row = (int64_t)blockIdx.x * AD_ROWS + wave * 16 + (lane & 15);
    const float* xp = a.X + (row < a.N ? row : a.N - 1) * AD_C + 4 * q;      // clamp: loads stay in the bag
    float4* xl = reinterpret_cast<float4*>(smem) + wave * (2 * AD_KS1 * 64) + lane;
    {
        float p[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 2 * AD_KS1; ++k) {
            const float4 v = *reinterpret_cast<const float4*>(xp + 16 * k);
            xl[64 * k] = v;
            p[0] = fmaf(v.x, v.x, p[0]); p[1] = fmaf(v.y, v.y, p[1]); p[2] = fmaf(v.z, v.z, p[2]); p[3] = fmaf(v.w, v.w, p[3]);
        }
        if constexpr (MOE) {
            const float nrm = moc_fsqrt(ad_row_sum((p[0] + p[1]) + (p[2] + p[3])));
#pragma unroll 4
            for (int k = 0; k < 2 * AD_KS1; ++k) {
                float4 v = xl[64 * k];
                v.x = moc_fdiv(v.x, nrm); v.y = moc_fdiv(v.y, nrm); v.z = moc_fdiv(v.z, nrm); v.w = moc_fdiv(v.w, nrm);
                xl[64 * k] = v;
            }
        }
    }
    float wr[AD_MAX_E];                                               // router weights (moe)
    if constexpr (MOE) {
#pragma unroll
        for (int e = 0; e < AD_MAX_E; ++e) wr[e] = 0.f;
#pragma unroll 2
        for (int k = 0; k < 2 * AD_KS1; ++k) {
            const float4 v = xl[64 * k];
#pragma unroll
            for (int e = 0; e < AD_MAX_E; ++e)
                if (e < a.E) {
                    const float4 g = *reinterpret_cast<const float4*>(a.G + (int64_t)e * AD_C + 16 * k + 4 * q);
                    wr[e] = fmaf(v.x, g.x, wr[e]); wr[e] = fmaf(v.y, g.y, wr[e]);
                    wr[e] = fmaf(v.z, g.z, wr[e]); wr[e] = fmaf(v.w, g.w, wr[e]);
                }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int e = 0; e < AD_MAX_E; ++e) {
            wr[e] = ad_row_sum(wr[e]);
            mx = e < a.E && !(wr[e] <= mx) ? wr[e] : mx;              // a NaN score makes the whole softmax NaN, as torch's
        }
        float den = 0.f;
#pragma unroll
        for (int e = 0; e < AD_MAX_E; ++e) {
            wr[e] = e < a.E ? expf(wr[e] - mx) : 0.f;
            den += wr[e];
        }
#pragma unroll
        for (int e = 0; e < AD_MAX_E; ++e) wr[e] = moc_fdiv(wr[e], den);
    }

    float mix[AD_KS1][8];                                             // moe: sum_e w_e a_e; then m, then unit(m)
    if constexpr (MOE) {
#pragma unroll
        for (int s = 0; s < AD_KS1; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) mix[s][j] = 0.f;
    }
    const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
    const int n_exp = MOE ? a.E : 1;
    for (int e = 0; e < n_exp; ++e) {
        float we = 1.f;
        if constexpr (MOE) {
            we = wr[0];
#pragma unroll
            for (int k = 1; k < AD_MAX_E; ++k) we = e == k ? wr[k] : we;
        }
        const uint4* w1 = a.img + (size_t)e * (AD_EXPERT_BYTES / 16) + lane;
        const uint4* w2 = w1 + AD_W1_FRAGS * 64;
        // Two register sets of twelve fragments: one is loaded while the other feeds 24 MFMAs.  The scheduling fences keep
        // each load where it is written (left alone, hipcc hoists loads of many stages and spills).
        au32x4_t wa[12], wb[12];

        // ---- hidden^T = W1 act^T: 8 tiles of 16 hidden units x this wave's 16 rows, four tiles per stage
        f32x4_t hs[AD_HT], hl[AD_HT];
#pragma unroll
        for (int t = 0; t < AD_HT; ++t) { hs[t] = zero4; hl[t] = zero4; }
        ad_load12(w1, wa);
#pragma unroll 1
        for (int s = 0; s < AD_KS1; ++s) {
            const float4 v0 = xl[64 * (2 * s)], v1 = xl[64 * (2 * s + 1)];
            const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
            AdTerms xt;
            ad_split(v, xt);
            ad_load12(w1 + (size_t)(s * AD_HT + 4) * 3 * 64, wb);
            ad_six4<0, 1>(wa, &xt, hs, hl);
            __builtin_amdgcn_sched_barrier(0);
            const int sn = s + 1 < AD_KS1 ? s + 1 : AD_KS1 - 1;      // the last stage re-reads its own fragments: uniform
            ad_load12(w1 + (size_t)(sn * AD_HT) * 3 * 64, wa);
            ad_six4<0, 1>(wb, &xt, hs + 4, hl + 4);
            __builtin_amdgcn_sched_barrier(0);
        }
        // relu, and the terms of the hidden as the B operand of the second product: K-step u <- tiles 2 u, 2 u + 1
        AdTerms ht[AD_KS2];
#pragma unroll
        for (int u = 0; u < AD_KS2; ++u) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = ad_relu(hl[2 * u + (j >> 2)][j & 3] + hs[2 * u + (j >> 2)][j & 3]);
            ad_split(v, ht[u]);
        }
        // ---- a^T = relu(W2 hidden^T): output tile T = 2 s + half holds columns ad_kidx(s, q, 4 half + 0..3); its four
        // K-steps x three terms are twelve consecutive fragments; one accumulator pair per K-step
        ad_load12(w2, wa);
#pragma unroll
        for (int s = 0; s < AD_KS1; ++s) {
            f32x4_t os[2][4], ol[2][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { os[0][u] = zero4; ol[0][u] = zero4; os[1][u] = zero4; ol[1][u] = zero4; }
            ad_load12(w2 + (size_t)(2 * s + 1) * 12 * 64, wb);
            ad_six4<1, 1>(wa, ht, os[0], ol[0]);
            __builtin_amdgcn_sched_barrier(0);
            const int tn = 2 * s + 2 < AD_CT ? 2 * s + 2 : AD_CT - 1;
            ad_load12(w2 + (size_t)tn * 12 * 64, wa);
            ad_six4<1, 1>(wb, ht, os[1], ol[1]);
            float xf[8];
            if constexpr (!MOE) {
                const float4 v0 = xl[64 * (2 * s)], v1 = xl[64 * (2 * s + 1)];
                xf[0] = v0.x; xf[1] = v0.y; xf[2] = v0.z; xf[3] = v0.w; xf[4] = v1.x; xf[5] = v1.y; xf[6] = v1.z; xf[7] = v1.w;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int hf = j >> 2, i = j & 3;
                const float sm = (os[hf][0][i] + os[hf][1][i]) + (os[hf][2][i] + os[hf][3][i]);
                const float lg = (ol[hf][0][i] + ol[hf][1][i]) + (ol[hf][2][i] + ol[hf][3][i]);
                const float av = ad_relu(lg + sm);
                if constexpr (MOE) mix[s][j] = moc_fadd(mix[s][j], moc_fmul(av, we));
                else mix[s][j] = moc_fadd(moc_fmul(av, a.r), moc_fmul(xf[j], a.one_minus_r));
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if constexpr (MOE) {
        const float sn = moc_fsqrt(ad_row_sumsq(mix));
#pragma unroll
        for (int s = 0; s < AD_KS1; ++s) {
            const float4 v0 = xl[64 * (2 * s)], v1 = xl[64 * (2 * s + 1)];
            const float xf[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
            for (int j = 0; j < 8; ++j)
                mix[s][j] = moc_fadd(moc_fmul(moc_fdiv(mix[s][j], sn), a.r), moc_fmul(xf[j], a.one_minus_r));
        }
    }
    const float mn = moc_fsqrt(ad_row_sumsq(mix));
#pragma unroll
    for (int s = 0; s < AD_KS1; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) mix[s][j] = moc_fdiv(mix[s][j], mn);

    // ---- logits = unit(m) Wc: one class at a time against the transposed classifier
    const float* WcT = reinterpret_cast<const float*>(reinterpret_cast<const unsigned char*>(a.img) + (size_t)a.E * AD_EXPERT_BYTES);
    for (int k = 0; k < a.C; ++k) {
        const float v = ad_row_dot(mix, WcT + (int64_t)k * AD_C + 4 * q);
        if (q == (k & 3) && row < a.N) a.logits[row * a.C + k] = v;
    }
}

}  // namespace

extern "C" size_t moc_adapter_workspace(int64_t N, int c, int h, int E, int C) {
    if (N < 1 || c != AD_C || h != AD_H || E < 1 || E > AD_MAX_E || C < 1 || C > AD_MAX_CLS) return 0;
    return ad_ws_bytes(E, C);
}

extern "C" int moc_adapter_logits(const float* X, int64_t N, int c, const float* const* W1, const float* const* W2, int h,
                                  int E, const float* G, const float* Wc, int C, float ratio, float* logits,
                                  void* workspace, size_t workspace_bytes, moc_stream_t stream) {
    MOC_REQUIRE(X, "moc_adapter_logits: X is null");
    MOC_REQUIRE(W1 && W2, "moc_adapter_logits: the W1 / W2 pointer arrays are null");
    MOC_REQUIRE(Wc, "moc_adapter_logits: Wc is null");
    MOC_REQUIRE(logits, "moc_adapter_logits: logits is null");
    MOC_REQUIRE(workspace, "moc_adapter_logits: workspace is null");
    MOC_REQUIRE(N >= 1 && N < (1ll << 31), "moc_adapter_logits: bad N=%lld", (long long)N);
    MOC_REQUIRE(c == AD_C, "moc_adapter_logits: c=%d, only 512 is built", c);
    MOC_REQUIRE(h == AD_H, "moc_adapter_logits: h=%d, only 128 is built", h);
    MOC_REQUIRE(E >= 1 && E <= AD_MAX_E, "moc_adapter_logits: E=%d outside [1, 8]", E);
    MOC_REQUIRE(C >= 1 && C <= AD_MAX_CLS, "moc_adapter_logits: C=%d outside [1, 64]", C);
    MOC_REQUIRE((G == nullptr) == (E == 1), "moc_adapter_logits: G must be null when E == 1 and given when E >= 2 (E=%d)", E);
    MOC_REQUIRE(std::isfinite(ratio), "moc_adapter_logits: ratio is not finite");
    AdWeights w{};
    for (int e = 0; e < E; ++e) {
        MOC_REQUIRE(W1[e] && W2[e], "moc_adapter_logits: W1[%d] or W2[%d] is null", e, e);
        MOC_REQUIRE(((uintptr_t)W1[e] & 15) == 0 && ((uintptr_t)W2[e] & 15) == 0,
                    "moc_adapter_logits: W1[%d] and W2[%d] must be 16-byte aligned", e, e);
        w.W1[e] = W1[e];
        w.W2[e] = W2[e];
    }
    MOC_REQUIRE(((uintptr_t)X & 15) == 0, "moc_adapter_logits: X must be 16-byte aligned");
    MOC_REQUIRE(((uintptr_t)G & 15) == 0, "moc_adapter_logits: G must be 16-byte aligned");
    MOC_REQUIRE(((uintptr_t)workspace & 15) == 0, "moc_adapter_logits: workspace must be 16-byte aligned");
    MOC_REQUIRE(workspace_bytes >= ad_ws_bytes(E, C), "moc_adapter_logits: workspace_bytes=%zu, need %zu", workspace_bytes,
                ad_ws_bytes(E, C));
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_img = (int64_t)E * 2 * 128 * 64 + (int64_t)C * AD_C;
    adapter_image_kernel<<<moc_cdiv(n_img, 256), 256, 0, s>>>(w, E, Wc, C, (uint4*)workspace);
    MOC_CHECK_LAUNCH("moc_adapter_logits(image)");
    AdArgs a;
    a.X = X; a.img = (const uint4*)workspace; a.G = G; a.logits = logits; a.N = N; a.E = E; a.C = C;
    a.r = ratio; a.one_minus_r = (float)(1.0 - (double)ratio);
    const int grid = moc_cdiv(N, AD_ROWS);
    // (set on every call: cheap, and there is no once-only flag for two threads to race on)
    const void* fn = E == 1 ? (const void*)adapter_kernel<false> : (const void*)adapter_kernel<true>;
    const hipError_t ea = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, AD_SMEM);
    if (ea != hipSuccess) MOC_FAIL(MOC_ELAUNCH, "moc_adapter_logits: %s", hipGetErrorString(ea));
    if (E == 1) adapter_kernel<false><<<grid, 256, AD_SMEM, s>>>(a);
    else adapter_kernel<true><<<grid, 256, AD_SMEM, s>>>(a);
    MOC_CHECK_LAUNCH("moc_adapter_logits");
    return MOC_OK;
}
