// The one-launch step over the forward's tile records (pool_w1_step_tiles_kernel): the step of the shapes with
// C * topk <= 64 whose caller has given the record arrays -- for one meta-learner or for the lockstep runs of moc_train_steps_runs{,_hp} (grid.z = run).  Its
// argument blocks (TileStepArgs*) do not leave this file: the training entries (moc_meta.hip) call launch_tile_step and
// launch_tile_runs.
#include <cstddef>
#include <type_traits>
#include "moc_step_shared.h"

namespace {

// ---- the one-launch step over the forward's tile records (round 4) ----------------------------------------------
// Same job as pool_w1_step_kernel -- pooling, loss, backward, the whole Adam step in one launch, every workgroup
// repeating the pooling for itself -- restructured around what the phase stamps of round 4 showed (profiles/NOTES.md):
// the step is a chain of dependent memory round trips and of dependent instructions; neither gets shorter by adding
// threads, only by taking round trips and instructions out of the chain.
//  * A workgroup is FOUR waves and owns 256 columns of ONE hidden unit of W1, or -- the last column block, the "tail"
//    workgroup of the hidden unit -- b1[h] and W2[:, h] (h = 0: b2 too) and no column (grid (D / 256 + 1) x H: 192
//    workgroups at D = 512).  Every sum over the pairs runs in the same order as in pool_w1_step_kernel: the same bits.
//  * The kernel's arguments are its own compact struct, ordered by first use, and every cache line of them is touched
//    at the top in ONE wait: the general step's 700 bytes of arguments were five scalar-cache misses one after the other
//    in front of the first load.
//  * The pooling of class c is ONE wave's business from the first load to the pooled rows, with no workgroup barrier in
//    between: it reads the class's tile records (above; VQ keys per lane), forms the sixteen group maxima in registers
//    (32-bit score keys: quad maxima, one ds_bpermute, fifteen row rotations for the ranks), lists the records >= T0
//    (places by ballot, no LDS counter), requests the candidates' row ids / gates / candidate scores -- one round trip
//    that the ranking loop hides -- and leaves the pooled rows' operands in LDS.  No second gather round for them.
//    The class wave's work ENDS with the winners: nothing behind the barrier that the other waves' requests wait at
//    needs the pooled mean.
//  * Then ONE more round trip: the pairs' 256-column row pieces (three waves); the fourth wave requests their hidden
//    activation of unit h, forms the C pooled means from the winners' values (lane c: class c, largest first), does the
//    cross entropy under that request (butterflies by DPP) and forms dz / dh of the pairs itself, so that ONE barrier
//    stands between the round trip and the gradient sums; the parameters this workgroup steps were requested at the
//    top.  The publishing workgroup's fourth wave stores the slide's outputs as the last thing it does.
// Falls back to the full scores inside the kernel when the records cannot prove exactness.
struct TileStepArgs {
    // ---- first cache line (64 bytes): what the first loads need -- they are issued before the other lines are touched
    const unsigned long long* tkey;
    const uint32_t* trho;
    int64_t slot0;
    int cap, ntile_bound, C, K, D, slide0;
    int n_runs, slide_stride;       // batched runs (n_runs > 0): see the end of the struct
    const int32_t* n_sel;
    // ---- what this thread steps
    const int64_t* labels;
    int PS_CAP, xdt;
    int tail_inside;                // != 0: no tail workgroups (grid.x = D / 256), column block 0 owns the hidden unit's small elements too
    int S_host;                     // the slide's selected-row count when the host knows it (one run's launch; -1: n_sel[b])
    float *W1, *m_W1, *v_W1;
    const float* W2;
    float *b1, *m_b1, *v_b1, *b2, *m_b2, *v_b2, *m_W2, *v_W2;
    int64_t base;
    AdamCoef adam;
    const AdamCoef* adam_tab;       // graph replay: coefficients adam_tab[adam_ctr[0] + adam_pos]
    const int32_t* adam_ctr;
    int adam_pos, apply_adam;
    uint32_t use_bits;
    int img_dt;
    // ---- the candidates' operands, round trip 2
    const int64_t* trid;
    const float4* tlam;
    const float4* tsc;
    const float* H1;
    const unsigned char* X;
    // ---- outputs
    float* pooled_out;
    int32_t* topk_idx_out;
    int32_t* topk_cnt_out;
    float* loss;
    int32_t* pred;
    int32_t* n_pair;
    unsigned char* W1img;
    float* W2out;
    float *g_W1, *g_b1, *g_W2, *g_b2;
    // ---- fall-back
    const float* mixed_in;
    const float* cand;
    const float* gates;
    const int64_t* sel_row;
    int64_t stride;
    // ---- batched runs (n_runs > 0): grid.z = run; run r steps the meta-learner whose tensors lie par_stride floats (W2 in:
    // w2_stride, W2 out: w2out_stride, operand image: img_stride bytes) behind run 0's, on slide slide0 + r * slide_stride
    int64_t par_stride, w2_stride, w2out_stride, img_stride;
    // ---- the slide the NEXT step works on (slide b + 1 of the same work arrays): its selected rows are pulled toward the
    // Infinity Cache by the waves that have no class to pool
    // (the slide's first slot is read from the device's row_off by the prefetching waves themselves: a per-run array of them
    // made the argument segment 984 bytes, and the two more lines of it cost every launch 0.25 us)
    const int64_t* row_off;
    int prefetch_next;              // != 0: slide b + 1 follows in the same work arrays
    int sink_off;                   // byte offset of 1 KiB of LDS nobody reads (the prefetch's LDS-DMA destination)
};
// The launch of batched runs carries the per-run scalars behind the common block; ONE run's launch does not: the argument
// segment lives in host memory and every 64-byte line of it that the kernel touches costs its start ~0.1 us (984 -> 864
// bytes: alone 16.70 -> 16.45 us per step; without the 384 bytes of per-run arrays: see profiles/NOTES.md).
struct TileStepArgsRuns {
    TileStepArgs s;
    int64_t base_r[MOC_MAX_RUNS], slot0_r[MOC_MAX_RUNS];
    int32_t cap_r[MOC_MAX_RUNS], ntb_r[MOC_MAX_RUNS];
};
static_assert(sizeof(TileStepArgsRuns) <= 1024, "a kernel-argument segment over 1 KiB takes a slow launch path (profiles/NOTES.md)");
// Batched runs with Adam coefficients PER RUN (moc_train_steps_runs_hp): run r's AdamCoef of this step travels by value
// behind the per-run scalars and the workgroup's run index -- wave-uniform -- selects its entry with one scalar load from
// the argument block: no device table, no upload, nothing to synchronise per step.  Sixteen entries of 32 bytes behind the
// 864 bytes above would pass the 1-KiB bound of the fast launch path, so a launch of this form serves at most
// MOC_HP_RUNS = 8 runs (the chain length moc_amd.runs uses: 480 + 8 x 24 + 8 x 32 = 928 bytes); the entry issues the step
// of more runs as two launches.  The launches of moc_train_steps_runs keep the block above, and their kernel.
struct TileStepArgsRunsHp {
    TileStepArgs s;
    int64_t base_r[MOC_HP_RUNS], slot0_r[MOC_HP_RUNS];
    int32_t cap_r[MOC_HP_RUNS], ntb_r[MOC_HP_RUNS];
    AdamCoef adam_r[MOC_HP_RUNS];
};
static_assert(sizeof(TileStepArgsRunsHp) <= 1024, "a kernel-argument segment over 1 KiB takes a slow launch path (profiles/NOTES.md)");
static_assert(offsetof(TileStepArgsRunsHp, adam_r) % sizeof(AdamCoef) == 0, "a run's coefficients: one aligned 32-byte scalar load");
__host__ __device__ __forceinline__ const TileStepArgs& tile_common(const TileStepArgs& x) { return x; }
__host__ __device__ __forceinline__ const TileStepArgs& tile_common(const TileStepArgsRuns& x) { return x.s; }
__host__ __device__ __forceinline__ const TileStepArgs& tile_common(const TileStepArgsRunsHp& x) { return x.s; }

// Lane l's value of x on lane l ^ OFF of its row of sixteen lanes (OFF = 8, 4, 2, 1), by DPP: what __shfl_xor gives for
// these partners, without its ds_bpermute round trip.  Every lane of the row must be active.
//   8: row_ror:8     4: row_half_mirror (l -> 7 - l of eight), then quad_perm [3,2,1,0]     2: quad_perm [2,3,0,1]     1: [1,0,3,2]
template <int OFF>
__device__ __forceinline__ int row16_xor(int x) {
    static_assert(OFF == 8 || OFF == 4 || OFF == 2 || OFF == 1, "partners within a row of sixteen");
    if constexpr (OFF == 8) return __builtin_amdgcn_update_dpp(0, x, 0x128, 0xf, 0xf, false);
    else if constexpr (OFF == 4)
        return __builtin_amdgcn_update_dpp(0, __builtin_amdgcn_update_dpp(0, x, 0x141, 0xf, 0xf, false), 0x1B, 0xf, 0xf, false);
    else if constexpr (OFF == 2) return __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xf, 0xf, false);
    else return __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xf, 0xf, false);
}
template <int OFF>
__device__ __forceinline__ float row16_xor(float x) { return __uint_as_float((unsigned)row16_xor<OFF>((int)__float_as_uint(x))); }

template <int VQ, typename ArgsT>
__global__ __launch_bounds__(256, 4) void pool_w1_step_tiles_kernel(ArgsT args) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool RUNS = !std::is_same<ArgsT, TileStepArgs>::value;
    constexpr bool RUN_HP = std::is_same<ArgsT, TileStepArgsRunsHp>::value;      // Adam coefficients per run
    const TileStepArgs& a = tile_common(args);
    static_assert(offsetof(TileStepArgs, n_sel) + 8 <= 64, "the first loads' arguments must share the first cache line");
    // batched runs: this workgroup's run -- its slide, its region of the records, the offsets of its tensors (the argument
    // block itself is not modified and its arrays are read through kernarg_at: either would send all of it to scratch)
    int b = a.slide0;
    int64_t base = 0, slot0 = a.slot0, po = 0, w2o = 0, w2outo = 0, imgo = 0;
    int cap = a.cap, ntile_bound = a.ntile_bound;
    [[maybe_unused]] constexpr bool runs = RUNS;     // (read by device code only)
    if constexpr (RUNS) {
        const int run = blockIdx.z;
        b += run * a.slide_stride;
        slot0 = kernarg_at<int64_t>(offsetof(ArgsT, slot0_r) + 8 * (size_t)run);
        cap = kernarg_at<int32_t>(offsetof(ArgsT, cap_r) + 4 * (size_t)run);
        ntile_bound = kernarg_at<int32_t>(offsetof(ArgsT, ntb_r) + 4 * (size_t)run);
    }
    const int C = a.C, K = a.K, D = a.D;
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int cb = blockIdx.x, h = blockIdx.y;
    // The last column block is the TAIL workgroup of its hidden unit: it owns b1[h] and W2[:, h] (h = 0: b2 too) and no
    // column of W1 -- on a W1 workgroup those few elements' sums and second Adam update ran after the wave's own W1 work
    // (Batched runs of four or more keep the small elements on column block 0 instead -- tail_inside: R x 128 workgroups of
    // which a CU holds four, so that eight runs are ONE round of workgroups and not two; a few threads' second sum and
    // second Adam update behind their W1 work cost a single run 0.6 us, a launch of eight runs wins 8 us.)
    const bool tail_wg = !a.tail_inside && cb == (D >> 8); // (grid.x = D / 256 + 1; not gridDim: that pulls 256 bytes of hidden arguments into the segment)
    const bool tail_role = a.tail_inside ? cb == 0 : tail_wg;
    const bool wg0 = cb == 0 && h == 0;                                              // (of its run: publishes the slide's outputs)
    constexpr int CL = lds::TILE_CL;                                                  // candidates per class
    MOC_STAMP(10);
    MOC_STAMP_MIN(33);
    MOC_STAMP_MAX(34);
    // ---- round trip 1, requested before anything else -- before the other argument lines are even touched: the keys of
    // this wave's first class (wave w: classes w, w + 4, ...)
    unsigned long long key[VQ];
    uint32_t rho[VQ / 4];
#define MOC_TILE_KEYS(c)                                                                                              \
    {                                                                                                                 \
        const int64_t s_c_ = slot0 + (int64_t)(c) * cap * TILE_R;                                                     \
        const int nrec_b_ = ntile_bound * TILE_R;                                                                     \
        _Pragma("unroll") for (int q = 0; q < VQ; ++q) {                                                              \
            const int j = q * 64 + lane;                                                                              \
            key[q] = a.tkey[s_c_ + (j < nrec_b_ ? j : nrec_b_ - 1)];                                                  \
        }                                                                                                             \
        _Pragma("unroll") for (int rq = 0; rq < VQ / 4; ++rq) {                                                       \
            const int x = rq * 64 + lane;                                                                             \
            rho[rq] = a.trho[slot0 / TILE_R + (int64_t)(c) * cap + (x < ntile_bound ? x : ntile_bound - 1)];          \
        }                                                                                                             \
    }
    if (wave < C) MOC_TILE_KEYS(wave)
    __builtin_amdgcn_sched_barrier(0);
    moc_kernarg_touch<sizeof(ArgsT)>();                  // every other line of the arguments, side by side, one wait
    const int PS_CAP = a.PS_CAP;
    base = a.base;
    if constexpr (RUNS) {
        const int run = blockIdx.z;
        base = kernarg_at<int64_t>(offsetof(ArgsT, base_r) + 8 * (size_t)run);
        po = (int64_t)run * a.par_stride; w2o = (int64_t)run * a.w2_stride; w2outo = (int64_t)run * a.w2out_stride;
        imgo = (int64_t)run * a.img_stride;
    }
    // ... then what this thread steps (independent of the pooling; it queues behind the keys).  The small tensors' owners
    // sit in different waves: their sums over the pairs run side by side, not one after the other in one wave
    const int d = cb * 256 + t;                                                      // this thread's column of W1[h]
    float pw = 0.f, pm = 0.f, pv = 0.f;
    float pT = 0.f, pTm = 0.f, pTv = 0.f;                                            // this thread's element of W2 / b1 / b2
    int tail = -1;                                                                   // flat index past W1: b1 | W2 | b2
    if (tail_role) {
        if (t < 4) tail = H + t * H + h;                                             // W2[i = t][h]: wave 0
        else if (t == 64) tail = h;                                                  // b1[h]: wave 1
        else if (h == 0 && t >= 128 && t < 132) tail = H + 4 * H + (t - 128);        // b2[i]: wave 2
    }
    float w2v = 0.f;
    if (t < 4) w2v = a.W2[w2o + t * H + h];
    if (a.apply_adam) {
        if (!tail_wg) {
            const int64_t e = po + h * D + d;
            pw = a.W1[e]; pm = a.m_W1[e]; pv = a.v_W1[e];
        }
        if (tail >= H + 4 * H) { const int64_t i = po + tail - 5 * H; pT = a.b2[i]; pTm = a.m_b2[i]; pTv = a.v_b2[i]; }
        else if (tail >= H) { const int64_t i = po + tail - H; pTm = a.m_W2[i]; pTv = a.v_W2[i]; }
        else if (tail >= 0) { pT = a.b1[po + tail]; pTm = a.m_b1[po + tail]; pTv = a.v_b1[po + tail]; }
    }
    MOC_STAMP(19);
    // ---- the next slide's selected rows, its row ids and its candidate columns: one dword of every 128-byte line, by the
    // waves with no class to pool (C < 4), results never used.  The forward of the next step then finds them in the
    // Infinity Cache: with 492 MB of score pass streaming through that cache every pass, nothing of a slide is left in it
    // from the pass before (a 1-GB copy between two passes of steps with nothing else on the GPU: 16.8 -> 18.5 us per
    // step, scripts/diag_mall.py).  Inline asm: the compiler's wait insertion does not see these loads, nobody waits for
    // them (s_endpgm does).
    if (wave >= C && a.prefetch_next) {
        const int64_t nb = a.row_off[b + 1];
        const int S2 = a.n_sel[b + 1];
        const int esz_p = a.xdt == MOC_F32 ? 4 : 2;
        const int lpr = D * esz_p / 128;                                            // lines per row
        const int iw = 4 - C;                                                       // waves of a workgroup that come here
        const int gx = (D >> 8) + (a.tail_inside ? 0 : 1);
        const int g0 = ((h * gx + cb) * iw + (wave - C)) * 64 + lane, G = gx * H * iw * 64;
        // (LDS-DMA into 256 sacrificial bytes per wave: a load into a register that nobody reads leaves the compiler free to
        // re-use that register while the load is still in flight -- the first form of this did, and faulted)
        typedef const __attribute__((address_space(1))) void* gptr_t;
        typedef __attribute__((address_space(3))) void* lptr_t;
        float* sinkw = reinterpret_cast<float*>(smem + a.sink_off) + (wave - C) * 64;
        for (int L = g0; L < S2 * lpr; L += G) {
            const int r = L / lpr;
            const unsigned char* pl = a.X + a.sel_row[nb + r] * (int64_t)D * esz_p + (int64_t)(L - r * lpr) * 128;
            __builtin_amdgcn_global_load_lds((gptr_t)pl, (lptr_t)sinkw, 4, 0, 0);
        }
        const int ncol = 2 * C + 2, lpc = (S2 + 31) >> 5;                           // candidate columns, lines per column
        for (int L = g0; L < ncol * lpc; L += G) {
            const int c = L / lpc;
            const float* pl = a.cand + (int64_t)c * a.stride + nb + (int64_t)(L - c * lpc) * 32;
            __builtin_amdgcn_global_load_lds((gptr_t)pl, (lptr_t)sinkw, 4, 0, 0);
        }
    }
    AdamCoef ak = a.adam;
    if (a.adam_tab) ak = a.adam_tab[a.adam_ctr[0] + a.adam_pos];
    // (every place below that applies Adam -- the W1 tile, b1, W2 / b2, on column block 0 or on a tail workgroup -- takes `ak`)
    if constexpr (RUN_HP) ak = kernarg_at<AdamCoef>(offsetof(ArgsT, adam_r) + sizeof(AdamCoef) * (size_t)blockIdx.z);
    const int S = (!RUNS && a.S_host >= 0) ? a.S_host : a.n_sel[b];
    const int y = (int)a.labels[b];
    const int k = K < S ? K : S;
    // LDS carve (the sink above is Y.sink: it reaches the kernel as a.sink_off, ahead of everything this needs)
    const lds::TileStepLds Y = lds::tile_step_lds(C, K, PS_CAP);
    float4* plam = reinterpret_cast<float4*>(smem + Y.plam);
    float4* psc = reinterpret_cast<float4*>(smem + Y.psc);
    float* xs = reinterpret_cast<float*>(smem + Y.xs);
    float* dhs = reinterpret_cast<float*>(smem + Y.dhs);
    float* dz = reinterpret_cast<float*>(smem + Y.dz);
    unsigned long long* list = reinterpret_cast<unsigned long long*>(smem + Y.list);
    unsigned long long* t0s = reinterpret_cast<unsigned long long*>(smem + Y.t0s);
    int64_t* prid = reinterpret_cast<int64_t*>(smem + Y.prid);
    int* lsrc = reinterpret_cast<int*>(smem + Y.lsrc);
    float* topv = reinterpret_cast<float*>(smem + Y.topv);
    float* pooled_s = reinterpret_cast<float*>(smem + Y.pooled_s);
    float* dpool = reinterpret_cast<float*>(smem + Y.dpool);
    int* ncand = reinterpret_cast<int*>(smem + Y.ncand);
    int* flagc = reinterpret_cast<int*>(smem + Y.flagc);
    int* topk_s = reinterpret_cast<int*>(smem + Y.topk_s);
    float* h1s = reinterpret_cast<float*>(smem + Y.h1s);
    float* w2s = reinterpret_cast<float*>(smem + Y.w2s);
    if (t < 4) { w2s[t] = w2v; if (tail >= H) pT = w2v; }
    const int ntile = (S + 15) >> 4;
    for (int c = wave; c < C; c += 4) {                                              // ---- class c: this wave's, start to end
        const int64_t s_c = slot0 + (int64_t)c * cap * TILE_R;                       // the class's first record
        if (c != wave) MOC_TILE_KEYS(c)
        // the score halves of the keys decide bound and candidates (32-bit maxima and compares); absent records: 0
        uint32_t hi[VQ];
        uint32_t m = 0u;
        const int nrec = ntile * TILE_R;
#pragma unroll
        for (int q = 0; q < VQ; ++q) {
            hi[q] = q * 64 + lane < nrec ? (uint32_t)(key[q] >> 32) : 0u;
            m = hi[q] > m ? hi[q] : m;
        }
        MOC_STAMP(20);
        // group g = the tiles g, g + 16, ...: record j sits on lane j & 63, its tile is j >> 2 -- the four lanes 4g .. 4g + 3
        // hold group g, whatever q.  Quad maxima, then every row gathers the sixteen of them.
        {
            const uint32_t o1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0xB1, 0xf, 0xf, false);   // quad_perm [1,0,3,2]
            m = o1 > m ? o1 : m;
            const uint32_t o2 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x4E, 0xf, 0xf, false);   // quad_perm [2,3,0,1]
            m = o2 > m ? o2 : m;
        }
        const uint32_t gm = (uint32_t)__shfl((int)m, (lane & 15) * 4, 64);
        int grank = 0;
#define MOC_ROR(n) grank += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)gm, 0x120 + n, 0xf, 0xf, false) > gm ? 1 : 0;
        MOC_ROR(1) MOC_ROR(2) MOC_ROR(3) MOC_ROR(4) MOC_ROR(5) MOC_ROR(6) MOC_ROR(7) MOC_ROR(8)
        MOC_ROR(9) MOC_ROR(10) MOC_ROR(11) MOC_ROR(12) MOC_ROR(13) MOC_ROR(14) MOC_ROR(15)
#undef MOC_ROR
        // T0 = the K-th largest group maximum: K scores are >= it.  (0: fewer than K groups hold a record, or two group
        // maxima tie across the K-th place -- then every record is a candidate.)
        const unsigned long long hit = __ballot(lane < 16 && grank == k - 1 && gm != 0u);
        uint32_t T0 = 0u;
        if (hit != 0ull) T0 = (uint32_t)__builtin_amdgcn_readlane((int)gm, __ffsll((long long)hit) - 1);
        // the records >= T0 take their places in the list by ballot: sixty-four records at a time, a record's place is the
        // count so far (wave-uniform) plus the candidates on the lanes below it.  No LDS counter: an LDS add of per-lane
        // counts is compiled into a serial loop over the lanes that hold any, in front of the add's own round trip.  The
        // order of the list (q-major) is nobody's business: ranks compare unique keys, lsrc carries the record.
        // (an absent record's key half is 0: with the bound raised to 1 one compare tells both; the sixty-fours of records
        // past the slide's last tile are skipped by uniform branches)
        const uint32_t T1 = T0 > 1u ? T0 : 1u;
        int n = 0;
#pragma unroll
        for (int q = 0; q < VQ; ++q) {
            if (q * 64 < nrec) {
                // (the score half again from the key: hi[] need not live across the ranks above -- fewer VGPRs, less scratch at VQ = 16)
                const bool in = (q * 64 + lane < nrec ? (uint32_t)(key[q] >> 32) : 0u) >= T1;
                const unsigned long long bq = __ballot(in);
                const int pos = n + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bq >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bq, 0u));
                if (in && pos < CL) {
                    list[(size_t)c * PS_CAP + pos] = key[q];
                    lsrc[c * CL + pos] = q * 64 + lane;
                }
                n += __popcll(bq);
            }
        }
        // ... and the proof that no score >= T0 is missing from the records: no tile's (TILE_R + 1)-th largest reaches T0
        bool bad = false;
#pragma unroll
        for (int rq = 0; rq < VQ / 4; ++rq)
            bad = bad || (rq * 64 + lane < ntile && rho[rq] != 0u && rho[rq] >= T0);
        __builtin_amdgcn_wave_barrier();                 // (a wave's LDS accesses are served in order: the list is there for its readers)
        const bool fall = __ballot(bad) != 0ull || n > CL || n < k || k <= 0;
        if (lane == 0) { flagc[c] = fall ? 1 : 0; t0s[c] = (unsigned long long)T0 << 32; }
        MOC_STAMP(11);
        if (!fall) {                                                                 // (uniform over the wave)
            const unsigned long long mine = lane < n ? list[(size_t)c * PS_CAP + lane] : 0ull;
            const int jrec = lane < n ? lsrc[c * CL + lane] : 0;
            // the candidate's operands: one round trip, under the ranking loop
            const int64_t rid = a.trid[s_c + jrec];
            const float4 lam = a.tlam[s_c + jrec];
            const float4 scv = a.tsc[s_c + jrec];
            // (the list from LDS, one broadcast read per candidate: a loop of v_readlane on the score words with a count of
            // equal words beside it -- ten instructions per candidate -- was measured LONGER, 0.56 -> 0.68-0.72 us)
            int rank = 0;
            for (int l = 0; l < n; ++l) rank += list[(size_t)c * PS_CAP + l] > mine ? 1 : 0;
            MOC_STAMP(12);
            // The class wave's work ends with the winners: the waves behind the barrier need prid / topk_s for their
            // requests.  The pooled mean (topv) is the fourth wave's business, under its own round trip.
            if (lane < n && rank < k) {
                topk_s[c * K + rank] = (int)(~(unsigned)mine);
                topv[c * 16 + rank] = key_to_float((unsigned)(mine >> 32));
                const int p = c * k + rank;
                prid[p] = rid; plam[p] = lam; psc[p] = scv;
            }
        }
    }
    __syncthreads();
    MOC_STAMP(13);
    bool fast = true;
    for (int c = 0; c < C; ++c) fast = fast && flagc[c] == 0;
    if (wg0 && t == 0 && a.n_pair) {                     // (which path ran: tests, diagnostics; with runs: the largest code of any)
        if (a.n_runs > 0) atomicMax(a.n_pair, fast ? MOC_TILE_PATH_RECORDS : MOC_TILE_PATH_FULL);
        else *a.n_pair = fast ? MOC_TILE_PATH_RECORDS : MOC_TILE_PATH_FULL;
    }
    if (!fast) {
        // ---- fall-back: the same bound T0 (a valid one: K group maxima are K scores >= T0) over ALL mixed scores of the
        // slide.  Compact code, not fast code: it runs when a tile holds more than TILE_R of the candidates.
        if (t < C) ncand[t] = 0;
        __syncthreads();
        for (int c = 0; c < C; ++c) {
            const unsigned long long T0 = t0s[c];
            const float* col = a.mixed_in + (int64_t)c * a.stride + base;
            for (int i = t; i < S; i += 256) {
                const unsigned long long kk = ((unsigned long long)moc_key_desc(col[i]) << 32) | (unsigned)(~(unsigned)i);
                if (kk >= T0) {
                    const int pos = atomicAdd(&ncand[c], 1);
                    if (pos < PS_CAP) list[(size_t)c * PS_CAP + pos] = kk;
                }
            }
        }
        __syncthreads();
        for (int c = wave; c < C; c += 4) {                                          // k rounds of wave maximum
            const int n = ncand[c];
            const bool overflow = n > PS_CAP;                                        // pathological ties: straight from global
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
            if (lane == 0) pooled_s[c] = k > 0 ? sum / (float)k : __uint_as_float(0x7FC00000u);   // mean over no rows = NaN, like torch
            __builtin_amdgcn_wave_barrier();
            if (lane == 0 && wg0) {
                a.pooled_out[(int64_t)b * C + c] = pooled_s[c];
                if (a.topk_cnt_out) a.topk_cnt_out[(int64_t)b * C + c] = k;
            }
            if (a.topk_idx_out && wg0)
                for (int r = lane; r < K; r += 64)
                    a.topk_idx_out[((int64_t)b * C + c) * K + r] = r < k ? topk_s[c * K + r] : -1;
        }
        __syncthreads();
        const int P0 = C * k;
        for (int p = t; p < P0; p += 256) {                                          // the pooled rows' operands, gathered
            const unsigned kinv0 = (65536u + (unsigned)k - 1u) / (unsigned)k;
            const int c = (int)(((unsigned)p * kinv0) >> 16);
            const int sidx = topk_s[c * K + (p - c * k)];
            prid[p] = a.sel_row[base + sidx];
            plam[p] = reinterpret_cast<const float4*>(a.gates)[base + sidx];
            float4 s4;
            s4.x = a.cand[(int64_t)c * a.stride + base + sidx];
            s4.y = a.cand[(int64_t)(C + c) * a.stride + base + sidx];
            s4.z = a.cand[(int64_t)(2 * C) * a.stride + base + sidx];
            s4.w = a.cand[(int64_t)(2 * C + 1) * a.stride + base + sidx];
            psc[p] = s4;
        }
        __syncthreads();
    }
    MOC_STAMP(14);
    MOC_STAMP(15);
    // ---- round trip 2: the pairs' row pieces (three waves) and their hidden activation of unit h (the fourth)
    const int P = C * k;
    float xv_out = 0.f;                                                              // fourth wave, lane c: class c's pooled logit
    if (wave == 3) {
        // Lane p is pair p: P <= 64, for step_plan gives this kernel only shapes with C * K <= 64 (pool_one with train;
        // launch_tile_step_as refuses others).  The wave REQUESTS the pairs' hidden activation, does the cross entropy of
        // the pooled logits under that round trip, and then forms the pairs' dz and dh itself: their operands are dpool
        // (its own), the gates / candidate scores / W2 column (in LDS since the barrier above) and the activation it asked
        // for -- nothing of the row pieces, so no phase of its own between two workgroup barriers.
        float hv = 0.f;
        int pc = 0;                                                                  // the pair's class
        if (lane < P) {                                                              // (then k > 0)
            const unsigned kinv = (65536u + (unsigned)k - 1u) / (unsigned)k;
            pc = (int)(((unsigned)lane * kinv) >> 16);
            hv = a.H1[(base + topk_s[pc * K + (lane - pc * k)]) * H + h];
        }
        // cross entropy, argmax and d loss / d pooled.  The logits sit on lanes 0 .. 15 (C <= 16): the two butterflies over
        // them (partners xor 8, 4, 2, 1; ties to the smaller class) move their operands by DPP, not through the LDS pipe
        // The logits.  Records path: lane c forms class c's pooled mean itself from the winners' values the class wave left
        // in topv -- sixteen independent LDS reads in one batch, then the chain of additions, largest first, k of them (a
        // sum padded with + 0.f would turn a -0 into +0).  Fall-back: pooled_s is there.
        float xv = -INFINITY;
        if (fast) {
            float tv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) tv[r] = topv[(lane < C ? lane : 0) * 16 + r];
            float sum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) sum = r < k ? sum + tv[r] : sum;           // (a select, not an exit: no indexed registers)
            if (lane < C) xv = sum / (float)k;
        } else if (lane < C) xv = pooled_s[lane];
        xv_out = xv;
        float mx = xv;
        int arg = lane < C ? lane : 0x7fffffff;
#define MOC_CE_MAX(OFF)                                                                                               \
        {                                                                                                             \
            const float om = row16_xor<OFF>(mx);                                                                      \
            const int oa = row16_xor<OFF>(arg);                                                                       \
            if (om > mx || (om == mx && oa < arg)) { mx = om; arg = oa; }                                             \
        }
        MOC_CE_MAX(8) MOC_CE_MAX(4) MOC_CE_MAX(2) MOC_CE_MAX(1)
#undef MOC_CE_MAX
        const float ex = lane < C ? expf(xv - mx) : 0.f;
        float se = ex;
        se += row16_xor<8>(se); se += row16_xor<4>(se); se += row16_xor<2>(se); se += row16_xor<1>(se);
        const float lse = mx + logf(se);
        if (lane < C) dpool[lane] = expf(xv - lse) - (lane == y ? 1.f : 0.f);
        const float xy = fast ? __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(xv), y & 15)) : pooled_s[y];
        if (lane == 0 && wg0) {
            a.loss[b] = lse - xy;
            a.pred[b] = arg;
        }
        __builtin_amdgcn_wave_barrier();
        if (lane < P) {                                   // lane = pair: its dz, and dh of hidden unit h
            const int p = lane;
            h1s[p] = hv;
            const float gk = dpool[pc] / (float)k;
            const float4 l4 = plam[p], s4 = psc[p];
            const float lamv[4] = {l4.x, l4.y, l4.z, l4.w}, scs[4] = {s4.x, s4.y, s4.z, s4.w};
            float v = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float dlam = (a.use_bits >> i & 1u) ? gk * scs[i] : 0.f;
                const float dzi = dlam * lamv[i] * (1.f - lamv[i]);
                dz[p * 4 + i] = dzi;
                v = fmaf(dzi, w2s[i], v);
            }
            dhs[p] = hv > 0.f ? v : 0.f;
        }
    } else if (P > 0) {                                                              // (uniform)
        if (!tail_wg) {                                                              // row pieces -> fp32 in LDS: eight in flight per wave
            // (twenty-four rows per round over the three waves: K = 10, C = 2 is ONE round trip; with four per wave it was two)
            const int esz = a.xdt == MOC_F32 ? 4 : 2;
            const int64_t col0 = (int64_t)cb * 256 * esz;
            constexpr int RF = 8;
            for (int p0 = wave; p0 < P; p0 += 3 * RF) {
                const unsigned char* rp[RF];
#pragma unroll
                for (int u = 0; u < RF; ++u) {
                    const int pu = p0 + 3 * u;
                    rp[u] = a.X + prid[pu < P ? pu : p0] * (int64_t)D * esz + col0;
                }
                float4 v[RF];
                if (a.xdt == MOC_F32) {
#pragma unroll
                    for (int u = 0; u < RF; ++u) v[u] = reinterpret_cast<const float4*>(rp[u])[lane];
                } else {
                    const bool f16 = a.xdt == MOC_F16;
                    auto widen = [&](uint2 raw) {
                        float4 o;
                        if (f16) {
                            o.x = moc_f16_to_f32((uint16_t)raw.x); o.y = moc_f16_to_f32((uint16_t)(raw.x >> 16));
                            o.z = moc_f16_to_f32((uint16_t)raw.y); o.w = moc_f16_to_f32((uint16_t)(raw.y >> 16));
                        } else {
                            o.x = __uint_as_float(raw.x << 16); o.y = __uint_as_float(raw.x & 0xFFFF0000u);
                            o.z = __uint_as_float(raw.y << 16); o.w = __uint_as_float(raw.y & 0xFFFF0000u);
                        }
                        return o;
                    };
                    uint2 raw[RF];
#pragma unroll
                    for (int u = 0; u < RF; ++u) raw[u] = reinterpret_cast<const uint2*>(rp[u])[lane];
#pragma unroll
                    for (int u = 0; u < RF; ++u) v[u] = widen(raw[u]);
                }
#pragma unroll
                for (int u = 0; u < RF; ++u) {
                    const int pu = p0 + 3 * u;
                    if (pu < P) reinterpret_cast<float4*>(xs + (size_t)pu * 256)[lane] = v[u];
                }
            }
        }
    }
    __syncthreads();                                     // the ONE barrier in front of the gradient loops: row pieces, dz, dh, h1s
    MOC_STAMP(16);
    MOC_STAMP(17);
    // the slide's outputs of the records path (the fall-back has published its own), by the fourth wave of the publishing
    // workgroup as the LAST thing it does: stores in front of the gradient sums or of Adam would stand in the way of
    // their waits for the parameters' loads
    auto publish = [&]() {
        if (fast && wg0 && wave == 3) {
            if (lane < C) {
                a.pooled_out[(int64_t)b * C + lane] = xv_out;
                if (a.topk_cnt_out) a.topk_cnt_out[(int64_t)b * C + lane] = k;
            }
            if (a.topk_idx_out)
                for (int c = 0; c < C; ++c)
                    for (int r = lane; r < K; r += 64)
                        a.topk_idx_out[((int64_t)b * C + c) * K + r] = r < k ? topk_s[c * K + r] : -1;
        }
    };
    // ---- gradients of the owned elements, every sum over the pairs in ascending order (operands four pairs at a time:
    // the additions stay in order, the LDS reads do not wait for each other.  All operands of up to 24 pairs requested
    // in front of the first fmaf -- thirty reads, one counted wait -- was measured LONGER: 0.76-0.80 -> 1.08 us)
    float gr = 0.f;
    if (!tail_wg) {
        int p = 0;
        for (; p + 4 <= P; p += 4) {
            const float4 d4 = *reinterpret_cast<const float4*>(dhs + p);
            const float x0 = xs[(size_t)p * 256 + t], x1 = xs[(size_t)(p + 1) * 256 + t];
            const float x2 = xs[(size_t)(p + 2) * 256 + t], x3 = xs[(size_t)(p + 3) * 256 + t];
            gr = fmaf(d4.x, x0, gr); gr = fmaf(d4.y, x1, gr); gr = fmaf(d4.z, x2, gr); gr = fmaf(d4.w, x3, gr);
        }
        for (; p < P; ++p) gr = fmaf(dhs[p], xs[(size_t)p * 256 + t], gr);
    }
    float gt = 0.f;
    if (tail >= H + 4 * H) {
        const int i = tail - 5 * H;
        int p = 0;
        for (; p + 4 <= P; p += 4) {
            const float z0 = dz[p * 4 + i], z1 = dz[(p + 1) * 4 + i], z2 = dz[(p + 2) * 4 + i], z3 = dz[(p + 3) * 4 + i];
            gt += z0; gt += z1; gt += z2; gt += z3;
        }
        for (; p < P; ++p) gt += dz[p * 4 + i];
    } else if (tail >= H) {
        int p = 0;
        for (; p + 4 <= P; p += 4) {
            const float z0 = dz[p * 4 + t], z1 = dz[(p + 1) * 4 + t], z2 = dz[(p + 2) * 4 + t], z3 = dz[(p + 3) * 4 + t];
            const float4 h4 = {h1s[p], h1s[p + 1], h1s[p + 2], h1s[p + 3]};
            gt = fmaf(z0, h4.x, gt); gt = fmaf(z1, h4.y, gt); gt = fmaf(z2, h4.z, gt); gt = fmaf(z3, h4.w, gt);
        }
        for (; p < P; ++p) gt = fmaf(dz[p * 4 + t], h1s[p], gt);
    } else if (tail >= 0) {
        int p = 0;
        for (; p + 4 <= P; p += 4) {
            const float4 d4 = *reinterpret_cast<const float4*>(dhs + p);
            gt += d4.x; gt += d4.y; gt += d4.z; gt += d4.w;
        }
        for (; p < P; ++p) gt += dhs[p];
    }
    if (!a.apply_adam) {                                  // gradient out (data-parallel step with a collective)
        if (!tail_wg) a.g_W1[h * D + d] = gr;
        if (tail >= H + 4 * H) a.g_b2[tail - 5 * H] = gt;
        else if (tail >= H) a.g_W2[tail - H] = gt;
        else if (tail >= 0) a.g_b1[tail] = gt;
        publish();
        return;
    }
    const float gs = ak.grad_scale;
    if (!tail_wg) {
        const int64_t e = po + h * D + d;
        adam_update(pw, pm, pv, gr * gs, ak);
        a.W1[e] = pw; a.m_W1[e] = pm; a.v_W1[e] = pv;
        w1_image_store(a.img_dt, a.W1img + imgo, D, h, d, pw);
    }
    if (tail >= 0) {
        adam_update(pT, pTm, pTv, gt * gs, ak);
        if (tail >= H + 4 * H) { const int64_t i = po + tail - 5 * H; a.b2[i] = pT; a.m_b2[i] = pTm; a.v_b2[i] = pTv; }
        else if (tail >= H) { const int i = tail - H; a.W2out[w2outo + i] = pT; a.m_W2[po + i] = pTm; a.v_W2[po + i] = pTv; }
        else { a.b1[po + tail] = pT; a.m_b1[po + tail] = pTm; a.v_b1[po + tail] = pTv; }
    }
    publish();
    MOC_STAMP(18);
    MOC_STAMP_MAX(35);
}
#undef MOC_TILE_KEYS

// ------------------------------------------------------------------ host side
// the argument block of pool_w1_step_tiles_kernel for slide `slide` of B (one run)
// sh: the slide's selected-row count where the host knows it (the caller's host_n_sel, or n_sel_host), -1: not known
void tile_region(const moc_batch_t* B, int slide, int sh, int64_t* slot0, int* tcap, int* tb) {
    const int64_t base = B->row_off_host[slide], seg = B->row_off_host[slide + 1] - base;
    // the slide's region: cap tiles per class; the kernel's loads are issued before n_sel is known and clamped to the
    // tiles the slide can have at all (at most s_bound selected rows)
    *tcap = moc_cdiv(seg, 16) > 0 ? moc_cdiv(seg, 16) : 1;
    int tb_all = moc_cdiv(s_bound(B), 16);
    // the slide's own tile count: fewer record keys per lane in the step
    if (sh >= 0 && moc_cdiv(sh, 16) < tb_all) tb_all = sh > 0 ? moc_cdiv(sh, 16) : 1;
    *tb = *tcap < tb_all ? *tcap : tb_all;
    *slot0 = ((base >> 4) + slide) * (int64_t)B->C * TILE_R;
}

TileStepArgs tile_step_args(const StepPlan& p, const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws, const int64_t* labels, int slide,
                            uint32_t use_bits, const AdamCoef& k, float* W2out, int apply_adam, const StepTab* tab, int S_host = -1) {
    if (S_host < 0 && B->n_sel_host) S_host = B->n_sel_host[slide];   // (callers that do not ask host_n_sel themselves)
    const TileWs T = tile_carve(ws->tile_ws, tile_slots(B->total_rows, B->n_slides, B->C));
    TileStepArgs ta = {};
    ta.tkey = T.key; ta.trho = T.rho; ta.trid = T.rid; ta.tlam = T.lam; ta.tsc = T.sc;
    tile_region(B, slide, S_host, &ta.slot0, &ta.cap, &ta.ntile_bound);
    ta.C = B->C; ta.K = B->topk; ta.D = B->D; ta.slide0 = slide; ta.PS_CAP = p.cap;
    ta.xdt = B->dtype; ta.n_sel = B->n_sel; ta.labels = labels;
    ta.W1 = M->W1; ta.m_W1 = M->m_W1; ta.v_W1 = M->v_W1; ta.W2 = M->W2;
    ta.b1 = M->b1; ta.m_b1 = M->m_b1; ta.v_b1 = M->v_b1; ta.b2 = M->b2; ta.m_b2 = M->m_b2; ta.v_b2 = M->v_b2;
    ta.m_W2 = M->m_W2; ta.v_W2 = M->v_W2;
    ta.base = B->row_off_host[slide]; ta.adam = k;
    ta.row_off = B->row_off; ta.prefetch_next = 0;
    ta.S_host = S_host;
    ta.sink_off = lds::tile_step_lds(B->C, B->topk, p.cap).sink;
    if (tab) { ta.adam_tab = tab->tab; ta.adam_ctr = tab->ctr; ta.adam_pos = tab->pos; }
    ta.apply_adam = apply_adam; ta.use_bits = use_bits; ta.img_dt = B->dtype;
    ta.H1 = ws->H1; ta.X = (const unsigned char*)B->X;
    ta.pooled_out = ws->pooled; ta.topk_idx_out = ws->topk_idx; ta.topk_cnt_out = ws->topk_cnt;
    ta.loss = ws->loss; ta.pred = ws->pred; ta.n_pair = ws->n_pair;
    ta.W1img = (unsigned char*)M->W1_image; ta.W2out = W2out;
    ta.g_W1 = M->g_W1; ta.g_b1 = M->g_b1; ta.g_W2 = M->g_W2; ta.g_b2 = M->g_b2;
    ta.mixed_in = ws->mixed; ta.cand = B->cand; ta.gates = ws->gates; ta.sel_row = B->sel_row; ta.stride = B->total_rows;
    return ta;
}

// launches it -- for ONE meta-learner (the common argument block alone) or for tr.s.n_runs of them (grid.z; the per-run
// scalars behind the common block); the largest tile bound of any run picks the keys per lane
template <typename ArgsT>
int launch_tile_step_as(const StepPlan& p, const moc_batch_t* B, const ArgsT& args, int runs, int tb, hipStream_t s) {
    const TileStepArgs& ta = tile_common(args);
    MOC_REQUIRE(B->C * B->topk <= 64, "moc_fused_step(tiles): C * topk = %d pairs, one wave forms at most 64", B->C * B->topk);
    MOC_REQUIRE(p.smem == (size_t)lds::tile_step_lds(B->C, B->topk, p.cap).bytes && p.smem <= (size_t)lds::TILE_MAX_LDS,
                "pool_w1_step_tiles_kernel: C = %d, topk = %d, cap = %d need %zu B of LDS (> %d)", B->C, B->topk, p.cap, p.smem, lds::TILE_MAX_LDS);
    const dim3 grid(B->D / 256 + (ta.tail_inside ? 0 : 1), H, runs);   // D / 256 column blocks of W1 (+ the tail workgroup), per hidden unit
#define MOC_TILES_LAUNCH(VQ) pool_w1_step_tiles_kernel<VQ, ArgsT><<<grid, 256, p.smem, s>>>(args)
    const int vq = moc_cdiv((int64_t)tb * TILE_R, 64);                 // keys per lane of a class wave
    if (vq <= 4) MOC_TILES_LAUNCH(4);
    else if (vq <= 8) MOC_TILES_LAUNCH(8);
    else if (vq <= 12) MOC_TILES_LAUNCH(12);
    else MOC_TILES_LAUNCH(16);
#undef MOC_TILES_LAUNCH
    MOC_CHECK_LAUNCH("moc_fused_step(tiles)");
    return MOC_OK;
}
template <typename RunsT>
int launch_tile_step_runs(const StepPlan& p, const moc_batch_t* B, const RunsT& tr, hipStream_t s) {
    int tb = tr.s.ntile_bound;
    for (int r = 0; r < tr.s.n_runs; ++r) tb = tr.ntb_r[r] > tb ? tr.ntb_r[r] : tb;
    return launch_tile_step_as(p, B, tr, tr.s.n_runs, tb, s);
}

// whether the tile-record step pulls the next slide's selected rows toward the Infinity Cache (diagnostic: MOC_STEP_PREFETCH=0)
bool step_prefetch_on() {
    static const bool on = !(getenv("MOC_STEP_PREFETCH") && atoi(getenv("MOC_STEP_PREFETCH")) == 0);
    return on;
}

}  // namespace

void moc_meta_internal::tile_step_attrs(raise_lds_fn raise) {
#define MOC_TILES_ATTR(VQ)                                                                                                \
    raise("pool_w1_step_tiles_kernel", (const void*)pool_w1_step_tiles_kernel<VQ, TileStepArgs>, lds::TILE_MAX_LDS);     \
    raise("pool_w1_step_tiles_kernel(runs)", (const void*)pool_w1_step_tiles_kernel<VQ, TileStepArgsRuns>, lds::TILE_MAX_LDS); \
    raise("pool_w1_step_tiles_kernel(runs_hp)", (const void*)pool_w1_step_tiles_kernel<VQ, TileStepArgsRunsHp>, lds::TILE_MAX_LDS)
    MOC_TILES_ATTR(4); MOC_TILES_ATTR(8); MOC_TILES_ATTR(12); MOC_TILES_ATTR(16);
#undef MOC_TILES_ATTR
}

// next_slide: the slide the step after this one works on, in the same work arrays (-1: none / unknown) -- its rows are prefetched
int moc_meta_internal::launch_tile_step(const StepPlan& p, const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws,
                                        const int64_t* labels, int slide, uint32_t use_bits, const AdamCoef& k, float* W2out,
                                        hipStream_t s, int apply_adam, const StepTab* tab, int next_slide, int S_host) {
    TileStepArgs ta = tile_step_args(p, B, M, ws, labels, slide, use_bits, k, W2out, apply_adam, tab, S_host);
    if (step_prefetch_on() && next_slide == slide + 1 && next_slide < B->n_slides && B->C < 4) ta.prefetch_next = 1;
    return launch_tile_step_as(p, B, ta, 1, ta.ntile_bound, s);
}

namespace {
// the common block of the step launch of runs [r0, r0 + nr): M's tensors and both W2 buffers advanced to run r0
TileStepArgs runs_common(const StepPlan& p, const moc_batch_t* B, const moc_meta_t* M, const moc_runs_t* R, const moc_meta_ws_t* ws,
                         const int64_t* labels, int slide, bool more_steps, uint32_t use_bits, int r0, int nr, const AdamCoef& k,
                         float* cur, int64_t cur_stride, float* nxt, int64_t nxt_stride) {
    // four runs or more: throughput, not one run's latency, is what a launch is about -- no tail workgroups
    static const int tail_env = getenv("MOC_RUNS_TAIL_INSIDE") ? atoi(getenv("MOC_RUNS_TAIL_INSIDE")) : -1;   // diagnostic override
    moc_meta_t Mr = meta_of_run(M, R, r0);
    Mr.W2 = cur + (int64_t)r0 * cur_stride;             // the ping-pong buffer this step reads
    TileStepArgs ta = tile_step_args(p, B, &Mr, ws, labels, slide + r0 * R->slide_stride, use_bits, k,
                                     nxt + (int64_t)r0 * nxt_stride, 1, nullptr);
    ta.n_runs = nr; ta.slide_stride = R->slide_stride;
    ta.tail_inside = tail_env >= 0 ? tail_env : (R->n_runs >= 4 ? 1 : 0);
    ta.par_stride = R->par_stride; ta.img_stride = R->image_stride; ta.w2_stride = cur_stride; ta.w2out_stride = nxt_stride;
    // (launches of four runs or more are bound by workgroup slots, not by one run's latency: the prefetch cost eight
    // batched runs 3.6 %)
    if (step_prefetch_on() && more_steps && B->C < 4 && R->n_runs < 4) ta.prefetch_next = 1;
    return ta;
}
// the per-run scalars of runs [r0, r0 + nr) behind it (the arrays' unused entries: zero)
template <typename RunsT>
void runs_per_run(RunsT& tr, const moc_batch_t* B, const moc_runs_t* R, int slide, int r0, int nr, int cap_runs) {
    for (int r = 0; r < cap_runs; ++r) {
        tr.base_r[r] = 0; tr.slot0_r[r] = 0; tr.cap_r[r] = 0; tr.ntb_r[r] = 0;
        if (r >= nr) continue;
        const int sl = slide + (r0 + r) * R->slide_stride;
        tr.base_r[r] = B->row_off_host[sl];
        int cap_, tb_;
        tile_region(B, sl, B->n_sel_host ? B->n_sel_host[sl] : -1, &tr.slot0_r[r], &cap_, &tb_);
        tr.cap_r[r] = cap_; tr.ntb_r[r] = tb_;
    }
}
}  // namespace

int moc_meta_internal::launch_tile_runs(const StepPlan& p, const moc_batch_t* B, const moc_meta_t* M, const moc_runs_t* R,
                                        const moc_meta_ws_t* ws, const int64_t* labels, int slide, bool more_steps, uint32_t use_bits,
                                        int r0, int nr, const AdamCoef* k, bool k_per_run, float* cur, int64_t cur_stride, float* nxt,
                                        int64_t nxt_stride, hipStream_t s) {
    const TileStepArgs common = runs_common(p, B, M, R, ws, labels, slide, more_steps, use_bits, r0, nr, k[0], cur, cur_stride, nxt, nxt_stride);
    MOC_REQUIRE(nr >= 1 && nr <= (k_per_run ? MOC_HP_RUNS : MOC_MAX_RUNS), "moc_fused_step(tiles): %d runs in one launch", nr);
    if (!k_per_run) {       // one AdamCoef per launch: the argument block and the kernel moc_train_steps_runs has always had
        TileStepArgsRuns tr;
        tr.s = common;
        runs_per_run(tr, B, R, slide, r0, nr, MOC_MAX_RUNS);
        return launch_tile_step_runs(p, B, tr, s);
    }
    TileStepArgsRunsHp tr;
    for (int r = 0; r < MOC_HP_RUNS; ++r) tr.adam_r[r] = k[r < nr ? r : 0];   // (unused entries: the first run's)
    tr.s = common;
    runs_per_run(tr, B, R, slide, r0, nr, MOC_HP_RUNS);
    return launch_tile_step_runs(p, B, tr, s);
}
