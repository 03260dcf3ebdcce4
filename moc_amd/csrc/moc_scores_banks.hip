// Phase A, part 1 for prompt-bank selection: the streaming score pass over SEVERAL narrow classifier banks in one read
// of the bags (moc_scores_banks, include/moc_hip.h).
//
// A bank of at most 16 columns is one n-tile of the image moc_prepare_bank writes; G of them back to back are an image
// the streaming kernel's main loop (moc_scores.hip: scores_stream_kernel, NT = G) multiplies as it is.  What differs is
// the row epilogue: the wave's 16 x (G*16) tile is cut into G windows of 16 columns and the one-n-tile epilogue
// (row_stats_emit<4>) runs once per window with that bank's Ce, statistics and flags.  A column's accumulation chain does
// not depend on which other columns share the MFMA and the order over K is the one-n-tile kernel's, so bank g's
// statistics are bit for bit what moc_scores writes over a batch with that bank alone (tests/test_gpu_banks.py).
//
// The kernel is the STATIC walk of scores_stream_kernel, statement for statement (no tickets, no reserved compute
// units: an evaluation pass has the chip to itself), in a translation unit of its own so that the existing kernels'
// code does not change by an instruction (scripts/kernel_isa.py).
#include <stdlib.h>
#include <mutex>
#include "moc_common.h"
#include "moc_scores_stream.h"

namespace {

struct BankWindows {
    float* stats[4];
    uint8_t* sel_flag[4];
    int Ce[4];
};

// NT = banks of the launch.  The two register limits recorded in score_plan (moc_scores_plan.h) hold here as they do there: four
// n-tiles on fp32 bags only, three on 16-bit bags (twelve B fragments per batch leave hipcc short of registers).
template <int NF, bool BF16, int NT, bool F16>
__global__ __launch_bounds__(256, NT == 1 ? 2 : 1) void scores_banks_kernel(ScoresArgs a, BankWindows bw, int slide0, int n_slides) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int ESZ = BF16 ? 2 : 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row_bytes = (int64_t)a.D * ESZ;
    const int U = (int)(row_bytes / (NF * 64));                  // units per tile
    const int img_bytes = BF16 ? (a.D / 32) * 3 * 1024 : (a.D / 16) * 1024;
    constexpr int LDT = NT * 16 + 1;
    const int img_vec = img_bytes / 16;                          // uint4 per n-tile = per bank
    uint4* lds_b = reinterpret_cast<uint4*>(smem);
    float* tile = reinterpret_cast<float*>(smem + (size_t)NT * img_bytes) + wave * 16 * LDT;
    // [n_slides] first slot, [n_slides] first X row, [n_slides + 1] tile prefix, [n_slides] kept rows
    int64_t* s_base = reinterpret_cast<int64_t*>(smem + (size_t)NT * img_bytes + 4 * 16 * LDT * sizeof(float));
    int64_t* s_xbase = s_base + n_slides;
    int* prefix = reinterpret_cast<int*>(s_xbase + n_slides);
    int* s_nk = prefix + n_slides + 1;

    {   // the banks' images -> LDS, four 16-B loads in flight per thread
        const uint4* src = reinterpret_cast<const uint4*>(a.bank);
        const int nvec = NT * img_vec;
        int i = threadIdx.x;
        for (; i + 3 * 256 < nvec; i += 4 * 256) {
            const uint4 t0 = src[i], t1 = src[i + 256], t2 = src[i + 512], t3 = src[i + 768];
            lds_b[i] = t0; lds_b[i + 256] = t1; lds_b[i + 512] = t2; lds_b[i + 768] = t3;
        }
        for (; i < nvec; i += 256) lds_b[i] = src[i];
    }
    for (int b = threadIdx.x; b < n_slides; b += 256) {
        const int64_t base = a.row_off[slide0 + b];
        s_base[b] = base;
        s_xbase[b] = a.x_off ? a.x_off[slide0 + b] : base;
        s_nk[b] = a.kept ? a.n_kept[slide0 + b] : (int)(a.row_off[slide0 + b + 1] - base);
    }
    __syncthreads();
    if (wave == 0) {   // prefix[b] = tiles of slides < b; tiles are cut at absolute multiples of 16 slots, as moc_scores cuts them
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
    const int total = prefix[n_slides];
    const int stride = gridDim.x * 4;

    struct Unit { const unsigned char* p; int64_t base; int row0, nk, kk0; bool last; };
    // kept[] through the scalar cache (one tile's 16 indices are one uniform 64-B read that counts on lgkmcnt)
    typedef const int32_t __attribute__((address_space(4))) * kept_sptr;
    kept_sptr kept_s = (kept_sptr)(uintptr_t)a.kept;
    int cb = -1;                                                // slide of the previous tile (scalar)
    auto locate = [&](int g, int ch, Unit& u) {
        int b;
        if (cb < 0) {
            int lo = 0, hi = n_slides;                         // prefix[lo] <= g < prefix[hi]
            while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (prefix[mid] <= g) lo = mid; else hi = mid; }
            b = __builtin_amdgcn_readfirstlane(lo);
        } else {
            b = cb;
            for (;;) {                                         // (uniform: every lane reads the same words)
                const int i1 = b + 1 < n_slides ? b + 1 : n_slides, i2 = b + 2 < n_slides ? b + 2 : n_slides;
                const int i3 = b + 3 < n_slides ? b + 3 : n_slides;
                const int p1 = prefix[i1], p2 = prefix[i2], p3 = prefix[i3];
                const int adv = (g >= p1) + (g >= p2) + (g >= p3);                   // prefix is non-decreasing; g < prefix[n_slides]
                b = __builtin_amdgcn_readfirstlane(b + adv);
                if (adv < 3) break;
            }
        }
        cb = b;
        u.base = s_base[b];
        const int64_t xbase = s_xbase[b];
        u.nk = __builtin_amdgcn_readfirstlane(s_nk[b]);
        u.row0 = __builtin_amdgcn_readfirstlane((g - prefix[b]) * 16 - (int)(u.base & 15));     // < 0 in a short first tile
        int sel = lane & 15;
        const int first_valid = u.row0 < 0 ? -u.row0 : 0, last_valid = u.nk - 1 - u.row0;          // the tile holds a row
        sel = sel > first_valid ? sel : first_valid;               // clamp: loads stay in the slide
        sel = sel < last_valid ? sel : last_valid;
        int r = u.row0 + sel;
        if (a.kept) {
            const int idx = __builtin_amdgcn_readfirstlane((int)u.base + u.row0);
            int k[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                k[i] = kept_s[idx + i];
                asm volatile("" : "+s"(k[i]));     // pin to an SGPR (no lane-indexed VECTOR load: vmcnt)
            }
            r = k[0];
#pragma unroll
            for (int i = 1; i < 16; ++i) r = sel == i ? k[i] : r;
        }
        u.p = a.X + (xbase + r) * row_bytes + (lane >> 4) * 16 + (int64_t)ch * NF * 64;
        u.kk0 = ch * NF;
        u.last = ch == U - 1;
    };
    f32x4_t acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    auto compute = [&](const u32x4_t (&buf)[NF], const Unit& u) {
        // B fragments come from LDS one A fragment AHEAD of the MFMAs that use them (asm_lds_*)
        constexpr int PER = BF16 ? 3 : 1;                       // 16-B B fragments per A fragment and bank
        constexpr int NB = PER * NT;
        static_assert(NB <= 15, "lgkmcnt is a 4-bit counter");
        unsigned bbase[NT];                                    // LDS byte address of this unit's B rows, per bank
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
            bbase[nt] = (unsigned)(uintptr_t)(lds_b + nt * img_vec + u.kk0 * PER * 64 + lane);
        u32x4_t B0[NB], B1[NB];
        // per bank the chain over K of the one-n-tile kernel: fragment by fragment, term by term (16-bit bags) or
        // column by column (fp32 bags)
        auto mac = [&](const u32x4_t (&Bv)[NB], const u32x4_t& A) {
            if constexpr (BF16) {
#pragma unroll
                for (int term = 0; term < 3; ++term)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)            // independent accumulators back to back
                        acc[nt] = moc_mfma_half<F16>(A, Bv[term * NT + nt], acc[nt]);
            } else {
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(A[m]), __uint_as_float(Bv[nt][m]),
                                                                       acc[nt], 0, 0, 0);
            }
        };
        asm_lds_batch<0, PER, NT, 0, NB>(B0, bbase);
        compute_pairs_impl<0, NF, PER, NT, NB>(buf, B0, B1, bbase, mac);
        if (u.last) {
            wave_lds_order();
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int i = 0; i < 4; ++i) tile[((lane >> 4) * 4 + i) * LDT + nt * 16 + (lane & 15)] = acc[nt][i] * a.oscale;
            wave_lds_order();
            // window g = columns 16 g .. 16 g + 15 of the tile = bank g: the one-n-tile epilogue on its four values per lane
#pragma unroll
            for (int g = 0; g < NT; ++g) {
                ScoresArgs w = a;
                w.Ce = bw.Ce[g];
                w.stats = bw.stats[g];
                w.sel_flag = bw.sel_flag[g];
                float v[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = tile[(lane & 15) * LDT + g * 16 + q * 4 + (lane >> 4)];
                row_stats_emit<4>(w, v, u.base, u.row0, u.nk, tile, LDT);
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
    };
    // Flattened (tile, unit) walk, two register buffers: the NF loads of the next unit are issued, then the wait leaves
    // only those NF outstanding (moc_scores.hip has the reasons).  Tiles by a static stride per wave.
    int g = blockIdx.x * 4 + wave, ch = 0;
    auto advance = [&]() {
        const bool boundary = ++ch == U;
        if (boundary) ch = 0;
        if (boundary) g += stride;
    };
    u32x4_t bufA[NF], bufB[NF];
    Unit uA, uB;
    if (g < total) { locate(g, ch, uA); asm_issue<0, NF>(bufA, uA.p); }
    while (g < total) {
        advance();
        const bool moreB = g < total;
        if (moreB) { locate(g, ch, uB); asm_issue<0, NF>(bufB, uB.p); asm_wait_keep<NF, NF>(bufA); }
        else asm_wait_keep<0, NF>(bufA);
        compute(bufA, uA);
        if (!moreB) break;
        advance();
        const bool moreA = g < total;
        if (moreA) { locate(g, ch, uA); asm_issue<0, NF>(bufA, uA.p); asm_wait_keep<NF, NF>(bufB); }
        else asm_wait_keep<0, NF>(bufB);
        compute(bufB, uB);
    }
}

}  // namespace

// ------------------------------------------------------------------ host entry points
extern "C" int moc_scores_banks_max(int D, int dtype) {
    if (D <= 0 || D % 256 != 0 || (dtype != MOC_F32 && dtype != MOC_BF16 && dtype != MOC_F16)) return 0;
    return score_banks_max(D, dtype);
}

extern "C" size_t moc_bank_set_bytes(int D, int n_banks, int dtype) {
    return D <= 0 || n_banks <= 0 ? 0 : (size_t)n_banks * score_img_bytes(D, dtype);
}

// NT = banks of the launch: raises the instantiation's dynamic-LDS limit once per process (call_once: worker threads) and
// launches it
template <int NF, bool BF, int NT, bool FH>
static void launch_banks(const ScoresArgs& a, const BankWindows& bw, const ScorePlan& P, hipStream_t s, int s0, int ns) {
    static std::once_flag attr;
    std::call_once(attr, [] {
        (void)hipFuncSetAttribute((const void*)scores_banks_kernel<NF, BF, NT, FH>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SCORE_MAX_LDS);
    });
    hipLaunchKernelGGL((scores_banks_kernel<NF, BF, NT, FH>), dim3(P.gx), dim3(256), P.smem, s, a, bw, s0, ns);
}
template <int NF, bool BF, bool FH>
static void launch_banks_nt(const ScoresArgs& a, const BankWindows& bw, const ScorePlan& P, hipStream_t s, int s0, int ns) {
    if (P.NT == 1) launch_banks<NF, BF, 1, FH>(a, bw, P, s, s0, ns);
    else if (P.NT == 2) launch_banks<NF, BF, 2, FH>(a, bw, P, s, s0, ns);
    else if (P.NT == 3) launch_banks<NF, BF, 3, FH>(a, bw, P, s, s0, ns);
}

extern "C" int moc_scores_banks(const moc_batch_t* B, const moc_bank_set_t* S, moc_stream_t stream) {
    MOC_REQUIRE(B && S, "moc_scores_banks: null pointer (batch / bank set)");
    MOC_REQUIRE(S->image, "moc_scores_banks: null pointer (image)");
    MOC_REQUIRE(S->n_banks >= 1 && S->n_banks <= 4, "moc_scores_banks: n_banks=%d outside 1 .. 4", S->n_banks);
    MOC_REQUIRE(S->C >= 2, "moc_scores_banks: need C >= 2, got C=%d", S->C);
    for (int g = 0; g < S->n_banks; ++g) {
        MOC_REQUIRE(S->stats[g] && S->sel_flag[g], "moc_scores_banks: null pointer (stats / sel_flag of bank %d)", g);
        MOC_REQUIRE(S->Ce[g] > S->C && S->Ce[g] <= 16, "moc_scores_banks: bank %d: need C < Ce <= 16 (one n-tile), got C=%d Ce=%d",
                    g, S->C, S->Ce[g]);
    }
    {   // the batch's own C / Ce / topj / topk are not this entry's business
        moc_batch_t T = *B;
        T.C = S->C; T.Ce = S->Ce[0]; T.topj = 1; T.topk = 1;
        if (int rc = moc_check_batch(&T, "moc_scores_banks")) return rc;
    }
    MOC_REQUIRE(!B->tile_ticket && !B->cu_reserved, "moc_scores_banks: an evaluation pass -- static walk over the whole chip only "
                "(tile_ticket / cu_reserved must be null)");
    MOC_REQUIRE(!(B->flags & MOC_STATS_COMPACT), "moc_scores_banks: full statistics layout only (MOC_STATS_COMPACT is for banks "
                "wider than 16 columns)");
    // the streaming static form of moc_scores for G n-tiles: persistent workgroups, slides in chunks whose metadata fits
    // beside the images
    const int G = S->n_banks, gmax = score_banks_max(B->D, B->dtype);
    const ScoreShape shape = {B->D, B->dtype, G, B->n_slides, B->total_rows, B->max_rows, false, false, 0, true};
    const ScorePlan P = score_plan(shape);
    if (gmax == 0)
        MOC_FAIL(MOC_EUNSUPPORTED, "moc_scores_banks: D=%d needs %zu B of LDS for one bank's image, the epilogue tiles and one "
                 "slide (> 160 KiB)", B->D, P.need);
    MOC_REQUIRE(G <= gmax && !P.err, "moc_scores_banks: %d banks, but one launch serves at most %d at D=%d on this storage "
                "(moc_scores_banks_max)", G, gmax, B->D);
    ScoresArgs a = scores_args(B, S->image, G);
    a.C = S->C; a.Ce = 0;
    a.stats = nullptr; a.sel_flag = nullptr;
    a.compact = 0;
    const bool bf = B->dtype != MOC_F32, f16 = B->dtype == MOC_F16;
    BankWindows bw;
    for (int g = 0; g < 4; ++g) {
        const int h = g < G ? g : 0;
        bw.stats[g] = S->stats[h]; bw.sel_flag[g] = S->sel_flag[h]; bw.Ce[g] = S->Ce[h];
    }
    hipStream_t s = (hipStream_t)stream;
    for (int s0 = 0; s0 < B->n_slides; s0 += P.chunk) {
        const int ns = B->n_slides - s0 < P.chunk ? B->n_slides - s0 : P.chunk;
        if (P.unit == 16) {
            if (f16) launch_banks_nt<16, true, true>(a, bw, P, s, s0, ns);
            else if (bf) launch_banks_nt<16, true, false>(a, bw, P, s, s0, ns);
            else if (G == 4) launch_banks<16, false, 4, false>(a, bw, P, s, s0, ns);          // fp32 only: four n-tiles
            else launch_banks_nt<16, false, false>(a, bw, P, s, s0, ns);
        } else {   // 16-bit bags only: fp32 rows are a multiple of 1 KiB because D % 256 == 0
            if (f16) launch_banks_nt<8, true, true>(a, bw, P, s, s0, ns);
            else launch_banks_nt<8, true, false>(a, bw, P, s, s0, ns);
        }
        MOC_CHECK_LAUNCH("moc_scores_banks");
    }
    return MOC_OK;
}
