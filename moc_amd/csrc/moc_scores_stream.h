// Device pieces of the streaming score pass that more than one translation unit compiles: the kernel arguments, the
// row statistics of a 16-row tile (row_stats_emit) and the hand-issued loads with their counted waits.  moc_scores.hip
// (moc_scores) and moc_scores_banks.hip (moc_scores_banks) include it; the statements are the ones moc_scores.hip held.
// The host side of both entries comes with it: the launch plan (moc_scores_plan.h) and the argument filler.
#pragma once
#include "moc_common.h"
#include "moc_scores_plan.h"
#include <type_traits>

namespace {

// ------------------------------------------------------------------ score pass
struct ScoresArgs {
    const unsigned char* X;
    const unsigned char* bank;
    const int64_t* row_off;
    const int64_t* x_off;    // nullable
    const int32_t* kept;     // nullable
    const int32_t* n_kept;   // valid iff kept != nullptr
    float* stats;
    uint8_t* sel_flag;
    int64_t stride;          // total_rows
    int D, C, Ce, NT;
    int tpw;                 // 16-row tiles per wave (1 when NT > 1)
    float oscale;            // products -> logits: 1, or 2^-14 for the scaled fp16 image
    int compact;             // MOC_STATS_COMPACT: logits[C] | m1 | 1/den | gap | bg_sum | bg_max (no softmax columns)
    const uint32_t* cu_reserved;   // nullable: compute units the streaming form stays off (moc_batch_t.cu_reserved)
    int32_t* ticket;               // nullable: the streaming form's tile counter (moc_batch_t.tile_ticket), zero at launch
};

// The arguments of a pass over batch B against the image `bank` of NT n-tiles, for both entries: static walk over the
// whole chip (no ticket, no reserved set) and tpw = 0 until the caller's plan says otherwise.
inline ScoresArgs scores_args(const moc_batch_t* B, const void* bank, int NT) {
    ScoresArgs a;
    a.X = (const unsigned char*)B->X;
    a.bank = (const unsigned char*)bank;
    a.row_off = B->row_off;
    a.x_off = B->x_off;
    a.kept = B->mask ? B->kept : nullptr;
    a.n_kept = B->n_kept;
    a.stats = B->stats;
    a.sel_flag = B->sel_flag;
    a.stride = B->total_rows;
    a.D = B->D; a.C = B->C; a.Ce = B->Ce; a.NT = NT;
    a.tpw = 0;
    a.oscale = B->dtype == MOC_F16 ? 1.f / MOC_F16_BANK_SCALE : 1.f;
    a.compact = (B->flags & MOC_STATS_COMPACT) ? 1 : 0;
    a.cu_reserved = nullptr;
    a.ticket = nullptr;
    return a;
}

// The two partners of a lane under xor 16 / xor 32 without LDS (ds_bpermute) or its lgkmcnt: the gfx950 row swaps.
// permlane16_swap(x, x) leaves (x[row 0], x[row 1]) in BOTH rows 0 and 1 of the pair (rows 2, 3 alike), permlane32_swap
// the two halves: every lane of a pair then holds the same (lo, hi), so a commutative merge gives both the same bits.
template <int OFF>
__device__ __forceinline__ void xor_pair(float x, float& lo, float& hi) {
    static_assert(OFF == 16 || OFF == 32, "row swaps");
    const unsigned xi = __float_as_uint(x);
    if constexpr (OFF == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap(xi, xi, false, false);
        lo = __uint_as_float(r[0]); hi = __uint_as_float(r[1]);
    } else {
        const auto r = __builtin_amdgcn_permlane32_swap(xi, xi, false, false);
        lo = __uint_as_float(r[0]); hi = __uint_as_float(r[1]);
    }
}

// The statistics of one row from its Q*4 column values spread over the row's four lanes (lane = (part, row), part owning
// columns part, part + 4, ...): class columns q < qc, extension columns qc <= q < qe of this lane.  The wave spends more
// cycles here than in its MFMAs when it is alone on its SIMD (three n-tiles: 4,400 of 9,800 cycles per tile before this
// form, scripts/diag_score_phases.py), so the form is branch-free and short: masked values instead of predicated code,
// top-2 by min / max, the cross-lane merges by row swaps, exp as v_exp_f32 of (v - max) log2(e) -- exactly 1 at the
// maximum, relative error 2e-7 elsewhere, no denormal tail -- and ONE division per row (p = e * (1 / den)).
template <int Q>
__device__ __forceinline__ void row_stats_emit(const ScoresArgs& a, const float (&v)[Q], int64_t slot_base, int row0, int nk,
                                               const float* tile, int ldt) {
    const int lane = threadIdx.x & 63, row = lane & 15, part = lane >> 4;
    const int C = a.C, Ce = a.Ce;
    const int qc = (C - part + 3) >> 2, qe = (Ce - part + 3) >> 2;          // c = 4 q + part < C  <=>  q < qc
    float vm[Q];
    float m1 = -INFINITY, m2 = -INFINITY, bsum = 0.f, bmax = -INFINITY;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const bool cls = q < qc, ext = q >= qc && q < qe;
        vm[q] = cls ? v[q] : -INFINITY;
        m2 = fmaxf(m2, fminf(m1, vm[q]));                  // duplicates of the maximum count (gap 0), as topk(2)
        m1 = fmaxf(m1, vm[q]);
        bsum += ext ? v[q] : 0.f;
        bmax = fmaxf(bmax, ext ? v[q] : -INFINITY);
    }
    auto merge = [&](auto off) {
        constexpr int OFF = decltype(off)::value;
        float a1, b1, a2, b2, s0, s1, x0, x1;
        xor_pair<OFF>(m1, a1, b1); xor_pair<OFF>(m2, a2, b2); xor_pair<OFF>(bsum, s0, s1); xor_pair<OFF>(bmax, x0, x1);
        m2 = fmaxf(fminf(a1, b1), fmaxf(a2, b2));
        m1 = fmaxf(a1, b1);
        bsum = s0 + s1;
        bmax = fmaxf(x0, x1);
    };
    merge(std::integral_constant<int, 16>{});
    merge(std::integral_constant<int, 32>{});
    float e[Q], den = 0.f;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        e[q] = __builtin_amdgcn_exp2f((vm[q] - m1) * 1.44269504088896340736f);       // exp2(-inf) = 0: the masked columns
        den += e[q];
    }
    {
        float d0, d1;
        xor_pair<16>(den, d0, d1); den = d0 + d1;
        xor_pair<32>(den, d0, d1); den = d0 + d1;
    }
    const bool own_row = (unsigned)(row0 + row) < (unsigned)nk;  // else: beyond the slide (or, in a short first tile, before it)
    if (!own_row && !a.compact) return;                          // (the compact form's 16-byte stores use another lane mapping)
#ifdef MOC_STAMPS
    if (a.tpw == 7) {                                  // diagnostic (MOC_EPI_MODE=7): everything computed, nothing stored
#pragma unroll
        for (int q = 0; q < Q; ++q) { const float pq = e[q] / den; asm volatile("" ::"v"(pq), "v"(v[q])); }
        asm volatile("" ::"v"(m1), "v"(m2), "v"(bsum), "v"(bmax));
        return;
    }
#endif
    const float rden = 1.f / den;
    // column c of the statistics starts at stats + c * stride: a uniform base per q, one 32-bit lane offset for all
    const int64_t stride = a.stride;
    float* sv = a.stats + slot_base;
    float* sp = sv + (int64_t)C * stride;
    const unsigned off = (unsigned)((int64_t)part * stride + (row0 + row));
    if (a.compact) {
        // C + 5 columns: the logits, then m1 | 1/den | gap | bg_sum | bg_max.  The softmax columns are what the selector
        // and the candidate gather re-form from (v, m1, 1/den) with exactly the arithmetic above: e * rden.
        if (own_row) {
            float* st = a.stats + slot_base + (int64_t)C * stride + (row0 + row);
            if (part == 0) { st[0] = m1; st[2 * stride] = fabsf(m1 - m2); }
            else if (part == 1) { st[stride] = rden; st[3 * stride] = bsum; }
            else if (part == 2) st[4 * stride] = bmax;
            else a.sel_flag[slot_base + row0 + row] = 0;
        }
        // The logits leave as 16-byte stores: lane -> column 16 p + (lane >> 2), rows 4 (lane & 3) .. + 3 of the tile, read
        // back from the wave's LDS tile (where they are the v[] above).  One store instruction carries 16 columns x 64 B
        // instead of 4: the tile's C columns take ceil(C / 16) instructions, not ceil(C / 4) -- the wave was held by its
        // store issue (round 2: 2,000 of a tile's 8,000 cycles at thirty classes).  Tiles are cut at absolute multiples
        // of 16 slots, so a whole quad is 16-byte aligned; quads that straddle the slide's ends go row by row.
        const int rg = lane & 3, cq = lane >> 2;
        const int r_lo = row0 + rg * 4;
        const bool whole = r_lo >= 0 && r_lo + 3 < nk;
        for (int c0 = 0; c0 < C; c0 += 16) {
            const int c = c0 + cq;
            if (c >= C) continue;
            const float* tp = tile + (rg * 4) * ldt + c;
            const float x0 = tp[0], x1 = tp[ldt], x2 = tp[2 * ldt], x3 = tp[3 * ldt];
            float* dst = a.stats + slot_base + (int64_t)c * stride + r_lo;
            if (whole) {
                // (4-byte aligned in general -- a column starts at c * total_rows floats -- and 16-byte aligned whenever the
                // batch's total is a multiple of four: global_store_dwordx4 takes either)
                typedef float f32x4u_t __attribute__((ext_vector_type(4), aligned(4)));
                f32x4u_t pk = {x0, x1, x2, x3};
                *reinterpret_cast<f32x4u_t*>(dst) = pk;
            } else {
                if ((unsigned)(r_lo + 0) < (unsigned)nk) dst[0] = x0;
                if ((unsigned)(r_lo + 1) < (unsigned)nk) dst[1] = x1;
                if ((unsigned)(r_lo + 2) < (unsigned)nk) dst[2] = x2;
                if ((unsigned)(r_lo + 3) < (unsigned)nk) dst[3] = x3;
            }
        }
        return;
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        if (q < qc) {
            sv[off] = v[q];
            sp[off] = e[q] * rden;
        }
        sv += 4 * stride;
        sp += 4 * stride;
    }
    if (part < 3) {
        const float t = part == 0 ? fabsf(m1 - m2) : part == 1 ? bsum : bmax;
        a.stats[slot_base + (int64_t)(2 * C + part) * stride + row0 + row] = t;
    } else {
        a.sel_flag[slot_base + row0 + row] = 0;
    }
}

// ---- hand-counted vector loads for the streaming kernel --------------------------------
// LDS ordering inside one wave without touching vmcnt (the workgroup-scope fence used above
// emits s_waitcnt vmcnt(0) and would drain the loads in flight).  LDS executes a wave's
// operations in order; only the compiler must not reorder them.
__device__ __forceinline__ void wave_lds_order() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

typedef unsigned __attribute__((ext_vector_type(4))) u32x4_t;   // native vector: a legal "v" asm operand
template <int OFF>
__device__ __forceinline__ void asm_load16(u32x4_t& dst, const unsigned char* p) {
    asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=&v"(dst) : "v"(p), "n"(OFF) : "memory");
}
template <int F, int NF>
__device__ __forceinline__ void asm_issue(u32x4_t (&buf)[NF], const unsigned char* p) {
    if constexpr (F < NF) {
        asm_load16<F * 64>(buf[F], p);
        asm_issue<F + 1, NF>(buf, p);
    }
}
// wait until at most KEEP vector-memory operations are outstanding, then re-define every register
// of `buf` through an empty asm so that no use of it can be scheduled above the wait
template <int F, int NF>
__device__ __forceinline__ void asm_touch(u32x4_t (&buf)[NF]) {
    if constexpr (F < NF) {
        asm volatile("" : "+v"(buf[F]));
        asm_touch<F + 1, NF>(buf);
    }
}
template <int KEEP, int NF>
__device__ __forceinline__ void asm_wait_keep(u32x4_t (&buf)[NF]) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(KEEP) : "memory");
    asm_touch<0, NF>(buf);
}

// LDS reads of the B fragments, issued and awaited by hand for the same reason: left to hipcc, every
// ds_read_b128 sinks next to the MFMA that uses it (read, wait, MFMA, 144 times per tile at NT = 3) and
// with one workgroup per CU nothing hides that latency.  LDS returns in order, so after issuing batch
// n+1, "lgkmcnt(size of batch n+1)" means batch n has landed.  No scalar load is outstanding inside
// compute() (locate() consumes its own), so lgkmcnt counts only these reads.
template <int OFF>
__device__ __forceinline__ void asm_lds16(u32x4_t& dst, unsigned addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=&v"(dst) : "v"(addr), "n"(OFF) : "memory");
}
template <int KEEP, int NB>
__device__ __forceinline__ void asm_lds_wait_keep(u32x4_t (&buf)[NB]) {
    asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(KEEP) : "memory");
    asm_touch<0, NB>(buf);
}
// batch of B fragments for A fragment F: PER reads (terms) at F*PER*1024 + t*1024 from each of NT bases
template <int F, int PER, int NT, int I, int NB>
__device__ __forceinline__ void asm_lds_batch(u32x4_t (&Bv)[NB], const unsigned (&base)[NT]) {
    if constexpr (I < PER * NT) {
        constexpr int t = I / NT, nt = I % NT;
        asm_lds16<(F * PER + t) * 1024>(Bv[I], base[nt]);
        asm_lds_batch<F, PER, NT, I + 1, NB>(Bv, base);
    }
}

// two A fragments per step: issue the batch for F+1, wait for batch F, MFMAs of F; issue F+2, wait F+1, MFMAs
template <int F, int NF, int PER, int NT, int NB, typename Mac>
__device__ __forceinline__ void compute_pairs_impl(const u32x4_t (&buf)[NF], u32x4_t (&B0)[NB], u32x4_t (&B1)[NB],
                                                   const unsigned (&base)[NT], Mac& mac) {
    if constexpr (F < NF) {
        asm_lds_batch<F + 1, PER, NT, 0, NB>(B1, base);
        asm_lds_wait_keep<NB, NB>(B0);
        mac(B0, buf[F]);
        if constexpr (F + 2 < NF) {
            asm_lds_batch<F + 2, PER, NT, 0, NB>(B0, base);
            asm_lds_wait_keep<NB, NB>(B1);
        } else {
            asm_lds_wait_keep<0, NB>(B1);
        }
        mac(B1, buf[F + 1]);
        compute_pairs_impl<F + 2, NF, PER, NT, NB>(buf, B0, B1, base, mac);
    }
}

}  // namespace
