// What more than one of the step's sources needs -- moc_step_pool.hip (the three-launch step), moc_step_fused.hip (the
// narrow and the wide one-launch step), moc_step_tiles.hip (the one-launch step over tile records) and moc_meta.hip (the
// training entries): Adam's update, the argument block every pooling kernel reads, the pooling of a slide by one
// workgroup.  Private to those sources.  The kernel-argument structs stay in an anonymous namespace, one type per source:
// every kernel keeps the (internal) name it has always had.  What crosses between the sources is in moc_meta_internal.h.
#pragma once
#include <cstdlib>
#include "moc_meta_internal.h"
#include "moc_p2p.h"
#include "moc_step_lds.h"   // the step kernels' dynamic LDS: one layout per kernel, for the launch and for the carve

using namespace moc_meta_internal;
namespace lds = moc_step_lds;
static_assert(lds::H == MOC_HIDDEN, "moc_step_lds.h carries the hidden width on its own");
using lds::FIN_CHUNK;
using lds::WD_PCH_MIN;

namespace {

// torch.optim.Adam (single-tensor path, coupled L2), operation by operation:
//   g = g + wd*p ; m.lerp_(g, 1-b1) ; v.mul_(b2).addcmul_(g, g, 1-b2)
//   denom = sqrt(v)/bc2_sqrt + eps ; p.addcdiv_(m, denom, -step_size)
__device__ __forceinline__ void adam_update(float& p, float& m, float& v, float g, const AdamCoef& k) {
    g = moc_fadd(g, moc_fmul(k.wd, p));
    m = moc_fadd(m, moc_fmul(k.one_minus_b1, moc_fsub(g, m)));
    v = moc_fadd(moc_fmul(v, k.beta2), moc_fmul(moc_fmul(k.one_minus_b2, g), g));
    const float denom = moc_fadd(moc_fdiv(moc_fsqrt(v), k.bc2_sqrt), k.eps);
    p = moc_fadd(p, moc_fdiv(moc_fmul(k.neg_step_size, m), denom));
}

// ------------------------------------------------------------------ loss (+ pair gradients)
struct FinishArgs {
    const int64_t* row_off;
    const int64_t* sel_row;
    const int32_t* n_sel;
    const float* cand;
    const float *H1, *gates, *pooled;
    const float* mixed_in;          // fused kernel: [C, stride] mixed scores
    const int32_t *topk_idx, *topk_cnt;
    const int64_t* labels;
    float* loss;
    int32_t* pred;
    // train only
    float *W2, *b2, *b1;
    float *m_W2, *m_b2, *m_b1, *v_W2, *v_b2, *v_b1;
    float *g_W2, *g_b2, *g_b1;
    float* pair_dh;
    const unsigned char* X;
    int64_t* pair_row;
    int32_t* n_pair;
    int64_t stride;
    int64_t base_host;              // >= 0: first slot of the (single) slide; seg_host its slot count
    int seg_host, D, xdt;     // xdt: storage code of X (MOC_F32 / MOC_BF16 / MOC_F16)
    int C, K, slide0, train, apply_adam;
    uint32_t use_bits;
    AdamCoef adam;
    // graph replay (moc_train_steps_graph): the step's coefficients are adam_tab[adam_ctr[0] + adam_pos] instead of
    // `adam` -- kernel arguments are frozen at capture, the Adam step count is not
    const AdamCoef* adam_tab;
    const int32_t* adam_ctr;
    int adam_pos;
};

// the step's Adam coefficients: the kernel argument, or (graph replay) the table entry of this position in the pass.
// Uniform addresses: two scalar loads, requested where this is called (kernel start), consumed at the very end.
__device__ __forceinline__ AdamCoef step_coef(const FinishArgs& a) {
    AdamCoef k = a.adam;
    if (a.adam_tab) k = a.adam_tab[a.adam_ctr[0] + a.adam_pos];
    return k;
}

// ------------------------------------------------------------------ fused pooling + loss (+ step)
// top-K mean for every class, cross entropy, argmax and (train) the pair gradients with the
// Adam step of b1/W2/b2 in ONE workgroup of 16 waves -- for K <= 16, C <= 16, S <= 4096.
//
// top-K without K block-wide reductions: element i lives on wave i%16.  The K-th largest of
// the 16 per-wave maxima is a lower bound T0 of the K-th largest element (K waves hold an
// element >= T0), so only elements >= T0 can be in the top-K: a few dozen out of thousands.
// They go to a short LDS list per class, and one wave per class extracts them in value order
// (K wave-wide max reductions over the short list, DPP row operations, no LDS round trips).
constexpr int PS_VPT = 4;       // values per thread per class  (S <= 4096)

__device__ __forceinline__ float key_to_float(unsigned u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

__device__ __forceinline__ unsigned long long ps_key(const float* col, int i, int S) {
    return i < S ? ((unsigned long long)moc_key_desc(col[i]) << 32) | (unsigned)(~(unsigned)i) : 0ull;
}

struct PoolLds {
    unsigned long long *list, *wmax;     // [C][cap] candidate keys, [C][16] per-wave maxima
    float *pooled_s, *dpool;             // [C] pooled logits, d loss / d pooled
    int *ncand, *topk_s;                 // [C] candidate counts, [C][K] pooled rows in value order
};
// the pooling block of a kernel's layout, as pointers
__device__ __forceinline__ PoolLds pool_lds(unsigned char* smem, const lds::PoolBlockLds& B) {
    return {reinterpret_cast<unsigned long long*>(smem + B.list), reinterpret_cast<unsigned long long*>(smem + B.wmax),
            reinterpret_cast<float*>(smem + B.pooled_s), reinterpret_cast<float*>(smem + B.dpool),
            reinterpret_cast<int*>(smem + B.ncand), reinterpret_cast<int*>(smem + B.topk_s)};
}

// cross entropy of the pooled logits, argmax and (train) d loss / d pooled: wave 0, one class per lane;
// CE_OFF = widest xor offset (8: C <= 16, 32: C <= 64)
template <int CE_OFF>
__device__ __forceinline__ void ce_wave0(const FinishArgs& a, int b, int C, int y, const float* pooled_s, float* dpool,
                                         bool write_out, int which_wave = 0) {
    const int lane = threadIdx.x & 63;
    if ((int)(threadIdx.x >> 6) != which_wave) return;
    const float xv = lane < C ? pooled_s[lane] : -INFINITY;
    float mx = xv;
    int arg = lane < C ? lane : 0x7fffffff;
    for (int off = CE_OFF; off > 0; off >>= 1) {
        const float om = __shfl_xor(mx, off, 64);
        const int oa = __shfl_xor(arg, off, 64);
        if (om > mx || (om == mx && oa < arg)) { mx = om; arg = oa; }
    }
    const float ex = lane < C ? expf(xv - mx) : 0.f;
    float se = ex;
    for (int off = CE_OFF; off > 0; off >>= 1) se += __shfl_xor(se, off, 64);
    const float lse = mx + logf(se);
    if (lane < C && a.train) dpool[lane] = expf(xv - lse) - (lane == y ? 1.f : 0.f);
    if (lane == 0 && write_out) {
        a.loss[b] = lse - pooled_s[y];
        a.pred[b] = arg;
    }
}

// Pooling + loss of slide b by ONE workgroup of 16 waves (all threads must call): leaves the pooled
// rows in L.topk_s, the pooled logits in L.pooled_s and (train) d loss/d pooled in L.dpool; returns
// k = rows pooled per class.  `write_out`: this workgroup also publishes pooled/topk/loss/pred.
// VPT = scores per thread per class (S <= 1024 * VPT); CE_OFF = widest xor offset of the cross-entropy
// reduction (8: C <= 16 on lanes 0..15; 32: C <= 64 on the whole wave).
// CG = classes handled per round (CG * VPT 64-bit keys live in registers).
// `after_first_loads()` is called once, right after the first group's score loads have been ISSUED: the place for the
// caller's own prefetches (parameters, moments) -- loads return in issue order, so whatever is requested before the
// scores delays the first thing this kernel waits for.
struct PoolNoHook { __device__ __forceinline__ void operator()() const {} };
template <int VPT = PS_VPT, int CE_OFF = 8, int CG = 4, typename Hook = PoolNoHook>
__device__ __forceinline__ int pool_phase(const FinishArgs& a, int b, const PoolLds& L, int PS_CAP, bool write_out,
                                          float* pooled_out, int32_t* topk_idx_out, int32_t* topk_cnt_out,
                                          int64_t* base_out, Hook after_first_loads = Hook()) {
    const int C = a.C, K = a.K;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long* list = L.list;
    unsigned long long* wmax = L.wmax;
    float* pooled_s = L.pooled_s;
    float* dpool = L.dpool;
    int* ncand = L.ncand;
    int* topk_s = L.topk_s;
    const int64_t base = a.base_host >= 0 ? a.base_host : a.row_off[b];
    const int seg = a.base_host >= 0 ? a.seg_host : (int)(a.row_off[b + 1] - base);   // reads below stay inside the slide's slots
    const int y = (int)a.labels[b];
    if (threadIdx.x < C) ncand[threadIdx.x] = 0;
    // ---- the mixed scores, once: element q*1024 + tid (contiguous per wave) of up to 4 classes at a
    // time.  The loads are issued before n_sel is known (clamped to the slide's slots), masked after.
    // With fewer than k non-empty waves (S < 64k) the threshold below is 0 and every element is a
    // candidate: S <= 64*15 then, which the list holds.
    const int S = a.n_sel[b];
    const int k = K < S ? K : S;
    for (int c0 = 0; c0 < C; c0 += CG) {
        unsigned long long key[CG][VPT];
        {   // the group's loads, ALL of them before the first wait: unconditional (an absent class re-reads the last one,
            // a slot past the slide its last slot), masked afterwards -- a branch per class made every class its own
            // memory round trip
            float v[CG][VPT];
#pragma unroll
            for (int cc = 0; cc < CG; ++cc) {
                const int cl = c0 + cc < C ? c0 + cc : C - 1;
                const float* col = a.mixed_in + (int64_t)cl * a.stride + base;
#pragma unroll
                for (int q = 0; q < VPT; ++q) {
                    const int i = q * 1024 + (int)threadIdx.x;
                    v[cc][q] = col[i < seg ? i : seg - 1];
                }
            }
            if (c0 == 0) {
                after_first_loads();
                __builtin_amdgcn_sched_barrier(0);                // (hipcc otherwise sinks the hook's requests past the barriers below)
            }
#pragma unroll
            for (int cc = 0; cc < CG; ++cc)
#pragma unroll
                for (int q = 0; q < VPT; ++q) {
                    const int i = q * 1024 + (int)threadIdx.x;
                    key[cc][q] = (c0 + cc < C && i < S) ? ((unsigned long long)moc_key_desc(v[cc][q]) << 32) | (unsigned)(~(unsigned)i) : 0ull;
                }
        }
#pragma unroll
        for (int cc = 0; cc < CG; ++cc) {
            if (c0 + cc < C) {
                unsigned long long m = 0;
#pragma unroll
                for (int q = 0; q < VPT; ++q) m = key[cc][q] > m ? key[cc][q] : m;
                m = wave_max_u64(m);
                if (lane == 0) wmax[(c0 + cc) * 16 + wave] = m;
            }
        }
        __syncthreads();
        MOC_STAMP(11);
        // threshold = K-th largest wave maximum (keys are unique; 0 = empty wave): wave cc finds class c0 + cc's and leaves
        // it in the class's first wmax slot -- ONE wave per class, side by side on different SIMDs, not all sixteen each
        // for every class (an instruction all sixteen waves execute costs the CU four times one wave's)
        if (wave < CG && c0 + wave < C) {
            const int c = c0 + wave;
            const unsigned long long mine = wmax[c * 16 + (lane & 15)];
            int rank = 0;
#pragma unroll
            for (int l = 0; l < 16; ++l) rank += wmax[c * 16 + l] > mine ? 1 : 0;
            const unsigned long long hit = __ballot(lane < 16 && rank == k - 1 && mine != 0ull);
            unsigned long long T0 = 0ull;
            if (hit != 0ull && k <= 16) {
                const int src = __ffsll((long long)hit) - 1;
                const unsigned lo = (unsigned)__shfl((int)(unsigned)mine, src, 64);
                const unsigned hi = (unsigned)__shfl((int)(unsigned)(mine >> 32), src, 64);
                T0 = ((unsigned long long)hi << 32) | lo;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // every lane's reads of the slots are done
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) wmax[c * 16] = T0;
        }
        __syncthreads();
#pragma unroll
        for (int cc = 0; cc < CG; ++cc) {
            const int c = c0 + cc;
            if (c >= C) break;
            const unsigned long long T0 = wmax[c * 16];
#pragma unroll
            for (int q = 0; q < VPT; ++q) {
                const unsigned long long v = key[cc][q];
                if (v != 0ull && v >= T0) {
                    const int pos = atomicAdd(&ncand[c], 1);
                    if (pos < PS_CAP) list[(size_t)c * PS_CAP + pos] = v;
                }
            }
        }
    }
    __syncthreads();
    MOC_STAMP(12);
    // ---- extraction: wave w takes classes w, w+16, ...  Short lists (<= 64 candidates, the normal
    // case) are ranked in one sweep: a candidate's rank is the number of larger ones, and rank r < k
    // IS its position in value order.  Longer lists fall back to k wave-wide maximum rounds.
    for (int c = wave; c < C; c += 16) {
        const int n = ncand[c];
        if (k > 0 && n <= 64) {
            const unsigned long long mine = lane < n ? list[(size_t)c * PS_CAP + lane] : 0ull;
            int rank = 0;
            for (int l = 0; l < n; ++l) rank += list[(size_t)c * PS_CAP + l] > mine ? 1 : 0;
            float* topv = reinterpret_cast<float*>(wmax + c * 16);       // wave maxima are spent: 16 x 8 B of scratch
            if (lane < n && rank < k) {
                topk_s[c * K + rank] = (int)(~(unsigned)mine);
                topv[rank] = key_to_float((unsigned)(mine >> 32));
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) {                                             // summed largest first
                float sum = 0.f;
                for (int r = 0; r < k; ++r) sum += topv[r];
                pooled_s[c] = sum / (float)k;
            }
        } else if (k > 0) {
            const bool overflow = n > PS_CAP;        // pathological ties: rank straight from global
            const float* col = a.mixed_in + (int64_t)c * a.stride + base;
            unsigned long long prev = ~0ull;
            float sum = 0.f;
            for (int r = 0; r < k; ++r) {
                unsigned long long best = 0ull;
                if (!overflow) {
                    for (int i = lane; i < n; i += 64) {
                        const unsigned long long v = list[(size_t)c * PS_CAP + i];
                        if (v < prev && v > best) best = v;
                    }
                } else {
                    for (int i = lane; i < S; i += 64) {
                        const unsigned long long v = ps_key(col, i, S);
                        if (v < prev && v > best) best = v;
                    }
                }
                best = wave_max_u64(best);
                prev = best;
                sum += key_to_float((unsigned)(best >> 32));
                if (lane == 0) topk_s[c * K + r] = (int)(~(unsigned)best);
            }
            if (lane == 0) pooled_s[c] = sum / (float)k;
        } else if (lane == 0) {
            pooled_s[c] = __uint_as_float(0x7FC00000u);     // mean over no rows = NaN, like torch
        }
        __builtin_amdgcn_wave_barrier();
        if (lane == 0 && write_out) {
            pooled_out[(int64_t)b * C + c] = pooled_s[c];
            if (topk_cnt_out) topk_cnt_out[(int64_t)b * C + c] = k;
        }
        if (topk_idx_out && write_out)
            for (int r = lane; r < K; r += 64)
                topk_idx_out[((int64_t)b * C + c) * K + r] = r < k ? topk_s[c * K + r] : -1;
    }
    __syncthreads();
    MOC_STAMP(13);
    // ---- cross entropy, argmax: wave 0, one class per lane
    ce_wave0<CE_OFF>(a, b, C, y, pooled_s, dpool, write_out);
    *base_out = base;
    return k;
}

// The argument block of the narrow and the wide one-launch step (moc_step_fused.hip).
struct FusedArgs {
    FinishArgs f;
    float *W1, *m_W1, *v_W1, *g_W1;
    unsigned char* W1img;
    float* W2out;
    int img_dt;
    P2pArgs x;              // world > 1: sum the gradient over the node's ranks before the update
};

// ------------------------------------------------------------------ host side
// the wide step's layout of a batch, at `pch` pairs per chunk
inline lds::WideStepLds wide_lds(const moc_batch_t* B, int pch) {
    return lds::wide_step_lds(B->C, B->topk, B->D, (int)moc_elem_size(B->dtype), pch, lds::wide_cap(B->C));
}

// what finish_kernel, pool_step_kernel and the one-launch steps all read; each launcher adds only its own fields
inline FinishArgs finish_args(const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws, const int64_t* labels, int slide0,
                              int train, int apply_adam, uint32_t use_bits, const AdamCoef& k) {
    FinishArgs a = {};
    a.row_off = B->row_off; a.sel_row = B->sel_row; a.n_sel = B->n_sel; a.cand = B->cand;
    a.H1 = ws->H1; a.gates = ws->gates; a.pooled = ws->pooled;
    a.labels = labels; a.loss = ws->loss; a.pred = ws->pred;
    a.W2 = M->W2; a.b2 = M->b2; a.b1 = M->b1;
    a.m_W2 = M->m_W2; a.m_b2 = M->m_b2; a.m_b1 = M->m_b1; a.v_W2 = M->v_W2; a.v_b2 = M->v_b2; a.v_b1 = M->v_b1;
    a.g_W2 = M->g_W2; a.g_b2 = M->g_b2; a.g_b1 = M->g_b1;
    a.stride = B->total_rows; a.C = B->C; a.K = B->topk; a.slide0 = slide0; a.train = train;
    a.apply_adam = apply_adam; a.use_bits = use_bits; a.adam = k;
    return a;
}
// ... and of the kernels that pool for themselves: the scores, the rows, and one slide's extent where the host knows it
inline void finish_rows(FinishArgs& a, const moc_batch_t* B, const moc_meta_ws_t* ws, int slide, bool one_slide) {
    a.mixed_in = ws->mixed;
    a.X = (const unsigned char*)B->X; a.D = B->D; a.xdt = B->dtype;   /* storage code: 0 f32, 1 bf16, 2 f16 */
    a.base_host = -1; a.seg_host = 0;
    if (one_slide && B->row_off_host) {
        a.base_host = B->row_off_host[slide];
        a.seg_host = (int)(B->row_off_host[slide + 1] - a.base_host);
    }
}

}  // namespace
