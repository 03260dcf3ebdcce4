// The score pass as an LDS-DMA ring (MOC_SCORES_RING, include/moc_hip.h), and the entries moc_scores / moc_scores_timed.
//
// scores_stream_kernel (moc_scores.hip) keeps a tile's A fragments in registers, two buffers of sixteen 16-byte loads
// per lane: 202 VGPRs at two workgroups per CU, and no forward or step workgroup fits on a CU that holds one of them --
// hence the reserved CUs and the ticketed walk of the look-ahead launch.  Here the rows never touch a register on their
// way in.  A persistent workgroup per CU has ONE loader wave, which moves every 16-row x 1 KiB unit of the workgroup's
// tiles into a ring of 16 KiB LDS slots with sixteen global_load_lds_dwordx4 (nt: the rows are read once), and THREE
// consumer waves, each of which takes every third tile of the workgroup, reads the unit's A fragments from its slot
// and the B fragments from the bank image in LDS, and issues the v_mfma_f32_16x16x4_f32 chain of the register kernel
// in the same order: the same statistics, bit for bit (tests/test_gpu_scores_ring.py).
//
// One DMA instruction writes 1 KiB of LDS, lane l at 16 l: with lane (part, row) = (l >> 4, l & 15) fetching bytes
// [64 F + 16 part, + 16) of its row, fragment F of a slot IS the register kernel's A fragment F in lane order.  The
// consumers read it back with one ds_read_b128 per lane at consecutive addresses: no two row starts share a bank.
//
// Synchronisation is inside the workgroup and in LDS only: per slot a FULL word (the loader writes the slot's
// generation once the fill has landed, behind a counted vmcnt that leaves the next fills in flight) and a FREE word
// (the consumer that read the slot writes the generation back).  Every use of a slot has exactly one consumer, and
// the uses of a slot are ordered by the protocol itself, so one FREE word per slot serves all three waves.  Tiles by a
// static stride over the flat tile list of scores_stream_kernel's static walk: no ticket, no counter, no flag in
// global memory, no wait on another workgroup.
//
// moc_scores.hip is compiled as part of this unit, unchanged (profiles/traffic.json is keyed by its hash): its two
// entries are the register path, under other names, and the entries below plan the batch first.
#include "moc_common.h"
#define moc_scores moc_scores_registers
#define moc_scores_timed moc_scores_registers_timed
#include "moc_scores.hip"
#undef moc_scores
#undef moc_scores_timed

namespace {

constexpr int RING_UNIT = (int)SCORE_RING_SLOT;           // bytes of a slot: 16 rows x 1 KiB, sixteen A fragments

// One LDS word read or written with the wave's own wait, invisible to the compiler's wait insertion: an ordinary LDS
// access in a wave with LDS-DMA in flight makes hipcc drain vmcnt first (the DMA writes LDS too).
__device__ __forceinline__ int ring_lds_read(unsigned addr) {
    int v;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(v) : "v"(addr) : "memory");
    return __builtin_amdgcn_readfirstlane(v);
}
__device__ __forceinline__ int64_t ring_lds_read64(unsigned addr) {
    unsigned long long v;
    asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(v) : "v"(addr) : "memory");
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (int64_t)(((unsigned long long)hi << 32) | lo);
}
// (every lane writes the same word: the wave's LDS operations execute in order, so whatever the wave read or wrote in
// LDS before this has happened when another wave sees the word)
__device__ __forceinline__ void ring_lds_write(unsigned addr, int v) {
    asm volatile("s_waitcnt lgkmcnt(0)\n\tds_write_b32 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
// -> false after RING_SPIN_MAX polls (about a tenth of a second; a wait of this protocol lasts microseconds): the wave then
// leaves the kernel, its slots unwritten, instead of holding the compute unit for ever
constexpr int RING_SPIN_MAX = 1 << 20;
__device__ __forceinline__ bool ring_wait_word(unsigned addr, int at_least) {
    for (int spin = 0; spin < RING_SPIN_MAX; ++spin) {
        if (ring_lds_read(addr) >= at_least) return true;
        __builtin_amdgcn_s_sleep(1);
    }
    return false;
}

// The consumer's sixteen k-steps of a unit: the A fragment (ring slot) and the B fragment (bank image) of step F + 1 are
// requested before the four MFMAs of step F, by hand (moc_scores_stream.h: left to hipcc, every read sinks next to its
// MFMA -- read, wait, MFMA, sixteen times over).  LDS returns a wave's reads in order: with the pair of F + 1 just issued,
// lgkmcnt(2) means the pair of F has landed.  The MFMAs and their order are scores_stream_kernel's (NT = 1).
template <int F>
__device__ __forceinline__ void ring_issue(u32x4_t (&P)[2], unsigned aa, unsigned ba) {
    asm_lds16<F * 1024>(P[0], aa);
    asm_lds16<F * 1024>(P[1], ba);
}
__device__ __forceinline__ void ring_mac(const u32x4_t (&P)[2], f32x4_t& acc) {
#pragma unroll
    for (int m = 0; m < 4; ++m)
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(P[0][m]), __uint_as_float(P[1][m]), acc, 0, 0, 0);
}
template <int F>
__device__ __forceinline__ void ring_pairs(u32x4_t (&P0)[2], u32x4_t (&P1)[2], unsigned aa, unsigned ba, f32x4_t& acc) {
    if constexpr (F < 16) {
        ring_issue<F + 1>(P1, aa, ba);
        asm_lds_wait_keep<2, 2>(P0);
        ring_mac(P0, acc);
        if constexpr (F + 2 < 16) {
            ring_issue<F + 2>(P0, aa, ba);
            asm_lds_wait_keep<2, 2>(P1);
        } else {
            asm_lds_wait_keep<0, 2>(P1);
        }
        ring_mac(P1, acc);
        ring_pairs<F + 2>(P0, P1, aa, ba, acc);
    }
}

// DEPTH: fills the loader leaves in flight behind the one it publishes (2 from four slots on, else 1)
template <int DEPTH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void scores_ring_kernel(ScoresArgs a, int n_slides, int nslot) {
    static_assert(DEPTH == 1 || DEPTH == 2, "vmcnt counts 16 DMA instructions per fill, 63 at the most");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int img_bytes = (a.D / 16) * 1024;
    const int U = a.D / 256;                                     // units per tile: 1 KiB of each row
    const int64_t row_bytes = (int64_t)a.D * 4;
    // the carve: RingLds (moc_scores_plan.h)
    uint4* lds_b = reinterpret_cast<uint4*>(smem);
    unsigned char* ring = smem + img_bytes;
    float* tiles = reinterpret_cast<float*>(ring + (size_t)nslot * RING_UNIT);
    int64_t* s_base = reinterpret_cast<int64_t*>(tiles + 3 * 16 * 17);
    int64_t* s_xbase = s_base + n_slides;
    int* prefix = reinterpret_cast<int*>(s_xbase + n_slides);
    int* s_nk = prefix + n_slides + 1;
    const unsigned meta_end = (unsigned)(uintptr_t)(s_nk + n_slides);
    const unsigned desc_a = (meta_end + 15u) & ~15u;             // per slot: first slot of the slide (8 B) | row0 | kept rows
    const unsigned full_a = desc_a + 16u * nslot, free_a = full_a + 4u * nslot;

    {   // bank image -> LDS, four 16-B loads in flight per thread
        const uint4* src = reinterpret_cast<const uint4*>(a.bank);
        const int nvec = img_bytes / 16;
        int i = threadIdx.x;
        for (; i + 3 * 256 < nvec; i += 4 * 256) {
            const uint4 t0 = src[i], t1 = src[i + 256], t2 = src[i + 512], t3 = src[i + 768];
            lds_b[i] = t0; lds_b[i + 256] = t1; lds_b[i + 512] = t2; lds_b[i + 768] = t3;
        }
        for (; i < nvec; i += 256) lds_b[i] = src[i];
    }
    for (int b = threadIdx.x; b < n_slides; b += 256) {
        const int64_t base = a.row_off[b];
        s_base[b] = base;
        s_xbase[b] = a.x_off ? a.x_off[b] : base;
        s_nk[b] = a.kept ? a.n_kept[b] : (int)(a.row_off[b + 1] - base);
    }
    if ((int)threadIdx.x < 2 * nslot) reinterpret_cast<int*>(smem + (full_a - (unsigned)(uintptr_t)smem))[threadIdx.x] = 0;
    __syncthreads();
    if (wave == 0) {   // prefix[b] = tiles of slides < b; tiles are cut at absolute multiples of 16 slots (scores_stream_kernel)
        int carry = 0;
        for (int c0 = 0; c0 < n_slides; c0 += 64) {
            const int b = c0 + lane;
            int v = 0;
            if (b < n_slides && s_nk[b] > 0) v = (s_nk[b] + (int)(s_base[b] & 15) + 15) >> 4;
            int inc = v;
            for (int off = 1; off < 64; off <<= 1) {
                const int o = __shfl_up(inc, off, 64);
                if (lane >= off) inc += o;
            }
            if (b < n_slides) prefix[b + 1] = carry + inc;
            carry += __shfl(inc, 63, 64);
        }
        if (lane == 0) prefix[0] = 0;
    }
    __syncthreads();
    const int total = __builtin_amdgcn_readfirstlane(prefix[n_slides]);
    const int G = gridDim.x;
    // this workgroup's tiles: blockIdx.x + j G, j < nj
    const int nj = (int)blockIdx.x < total ? (total - (int)blockIdx.x + G - 1) / G : 0;
    if (nj == 0) return;

    if (wave == 0) {
        // ---------------------------------------------------------------- loader
        typedef const __attribute__((address_space(1))) void* gptr_t;
        typedef __attribute__((address_space(3))) void* lptr_t;
        typedef const int32_t __attribute__((address_space(4))) * kept_sptr;
        kept_sptr kept_s = (kept_sptr)(uintptr_t)a.kept;
        const unsigned prefix_a = (unsigned)(uintptr_t)prefix, base_a = (unsigned)(uintptr_t)s_base;
        const unsigned xbase_a = (unsigned)(uintptr_t)s_xbase, nk_a = (unsigned)(uintptr_t)s_nk;
        int cb = 0;                                                // slide of the previous tile
        int slot = 0, gen = 1;                                     // of the unit being issued
        int pslot = 0, pgen = 1, pending = 0;                      // of the oldest unit not yet published
        auto publish = [&]() {
            ring_lds_write(full_a + 4u * pslot, pgen);
            if (++pslot == nslot) { pslot = 0; ++pgen; }
            --pending;
        };
        for (int j = 0; j < nj; ++j) {
            const int g = (int)blockIdx.x + j * G;
            // the slide of tile g: prefix[b] <= g < prefix[b + 1], from the previous tile's slide on -- gallop, then bisect
            // (the next tile of a workgroup is G tiles on: mostly the same slide or the next, far away only among tiny slides)
            int lo = cb, step = 1;
            while (lo + step < n_slides && ring_lds_read(prefix_a + 4u * (lo + step)) <= g) { lo += step; step <<= 1; }
            int hi = lo + step < n_slides ? lo + step : n_slides;
            while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (ring_lds_read(prefix_a + 4u * mid) <= g) lo = mid; else hi = mid; }
            const int b = cb = lo;
            const int64_t base = ring_lds_read64(base_a + 8u * b), xbase = ring_lds_read64(xbase_a + 8u * b);
            const int nk = ring_lds_read(nk_a + 4u * b);
            const int row0 = (g - ring_lds_read(prefix_a + 4u * b)) * 16 - (int)(base & 15);     // < 0 in a short first tile
            int sel = lane & 15;
            const int first_valid = row0 < 0 ? -row0 : 0, last_valid = nk - 1 - row0;              // the tile holds a row
            sel = sel > first_valid ? sel : first_valid;               // clamp: loads stay in the slide
            sel = sel < last_valid ? sel : last_valid;
            int r = row0 + sel;
            if (a.kept) {
                const int idx = __builtin_amdgcn_readfirstlane((int)base + row0);
                int k[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    k[i] = kept_s[idx + i];
                    asm volatile("" : "+s"(k[i]));     // pin to an SGPR: the kept rows come through the scalar cache (lgkmcnt)
                }
                r = k[0];
#pragma unroll
                for (int i = 1; i < 16; ++i) r = sel == i ? k[i] : r;
            }
            const unsigned char* p = a.X + (xbase + r) * row_bytes + (lane >> 4) * 16;
            for (int c = 0; c < U; ++c) {
                if (!ring_wait_word(free_a + 4u * slot, gen - 1)) return;     // the slot's previous use has been read
                const unsigned d = desc_a + 16u * slot;
                ring_lds_write(d, (int)(unsigned)base);
                ring_lds_write(d + 4, (int)(unsigned)((unsigned long long)base >> 32));
                ring_lds_write(d + 8, row0);
                ring_lds_write(d + 12, nk);
                unsigned char* dst = ring + (size_t)slot * RING_UNIT;
                const unsigned char* pc = p + (int64_t)c * 1024;
#pragma unroll
                for (int F = 0; F < 16; ++F)
                    __builtin_amdgcn_global_load_lds((gptr_t)(pc + F * 64), (lptr_t)(dst + F * 1024), 16, 0, 2);     // aux 2: nt
                if (++slot == nslot) { slot = 0; ++gen; }
                if (++pending > DEPTH) {                              // the oldest fill has landed when DEPTH younger ones remain
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(16 * DEPTH) : "memory");
                    publish();
                }
            }
        }
        if constexpr (DEPTH == 2) {
            if (pending == 2) {
                asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
                publish();
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (pending) publish();
        return;
    }

    // -------------------------------------------------------------------- consumers
    const int cw = wave - 1;
    float* tile = tiles + cw * 16 * 17;
    for (int j = cw; j < nj; j += 3) {
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
        int64_t base = 0;
        int row0 = 0, nk = 0;
        for (int c = 0; c < U; ++c) {
            const int u = j * U + c, slot = u % nslot, gen = u / nslot + 1;
            if (!ring_wait_word(full_a + 4u * slot, gen)) return;
            const unsigned aa = (unsigned)(uintptr_t)(reinterpret_cast<const uint4*>(ring + (size_t)slot * RING_UNIT) + lane);
            const unsigned ba = (unsigned)(uintptr_t)(lds_b + c * 16 * 64 + lane);
            u32x4_t P0[2], P1[2];
            ring_issue<0>(P0, aa, ba);
            ring_pairs<0>(P0, P1, aa, ba, acc);
            if (c == U - 1) {
                const unsigned d = desc_a + 16u * slot;
                base = ring_lds_read64(d);
                row0 = ring_lds_read(d + 8);
                nk = ring_lds_read(d + 12);
            }
            ring_lds_write(free_a + 4u * slot, gen);                  // (behind the wave's reads of the slot: LDS is in order)
        }
        wave_lds_order();
#pragma unroll
        for (int i = 0; i < 4; ++i) tile[((lane >> 4) * 4 + i) * 17 + (lane & 15)] = acc[i] * a.oscale;
        wave_lds_order();
        row_epilogue_wide<1>(a, tile, base, row0, nk);
    }
}

// the plan of a batch as moc_scores sees it (the register path re-plans without the ring bit: the same function)
ScoreShape scores_shape(const moc_batch_t* B) {
    ScoreShape q = {B->D, B->dtype, bank_nt(B->Ce), B->n_slides, B->total_rows, B->max_rows,
                    B->tile_ticket != nullptr, B->cu_reserved != nullptr, B->tile_ticket ? lookahead_cap() : 0, false};
    q.ring = (B->flags & MOC_SCORES_RING) != 0;
    return q;
}

int scores_entry(const moc_batch_t* B, const void* bank, moc_stream_t stream, hipEvent_t ev0, hipEvent_t ev1) {
    if (!B || !(B->flags & MOC_SCORES_RING)) return scores_impl(B, bank, stream, ev0, ev1);
    if (int rc = moc_check_batch(B, "moc_scores")) return rc;
    MOC_REQUIRE(bank && B->stats && B->sel_flag, "moc_scores: null bank/stats/sel_flag");
    const ScorePlan P = score_plan(scores_shape(B));
    MOC_REQUIRE(P.err != SCORE_PLAN_RING_TICKET, "moc_scores: MOC_SCORES_RING takes neither tile_ticket nor cu_reserved (the ring kernel "
                "walks the tiles statically, on every compute unit)");
    if (P.err || P.form != SCORE_RING) return scores_impl(B, bank, stream, ev0, ev1);
    const ScoresArgs a = scores_args(B, bank, 1);
    const ScoreLaunch l = {a, P, (hipStream_t)stream, ev0, ev1, false, false};
    if (P.unit >= 4) score_launch<scores_ring_kernel<2>>(l, B->n_slides, P.unit);
    else score_launch<scores_ring_kernel<1>>(l, B->n_slides, P.unit);
    MOC_CHECK_LAUNCH("moc_scores(ring)");
    return MOC_OK;
}

}  // namespace

extern "C" int moc_scores(const moc_batch_t* B, const void* bank, moc_stream_t stream) {
    return scores_entry(B, bank, stream, nullptr, nullptr);
}

extern "C" int moc_scores_timed(const moc_batch_t* B, const void* bank, moc_stream_t stream, void* start_event, void* stop_event) {
    MOC_REQUIRE(start_event && stop_event, "moc_scores_timed: null event");
    return scores_entry(B, bank, stream, (hipEvent_t)start_event, (hipEvent_t)stop_event);
}

extern "C" int moc_scores_form(const moc_batch_t* B) {
    if (moc_check_batch(B, "moc_scores_form")) return -1;
    const ScorePlan P = score_plan(scores_shape(B));
    if (P.err == SCORE_PLAN_RING_TICKET) {
        moc_set_error("moc_scores: MOC_SCORES_RING takes neither tile_ticket nor cu_reserved (the ring kernel walks the tiles "
                      "statically, on every compute unit)");
        return -1;
    }
    if (P.err) {
        moc_set_error("moc_scores: D=%d / n_slides=%d: no score kernel fits (plan error %d, %zu B of LDS)", B->D, B->n_slides, P.err, P.need);
        return -1;
    }
    return P.form;
}
