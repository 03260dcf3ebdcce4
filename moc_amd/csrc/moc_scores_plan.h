// The score pass's launch plan (moc_scores, moc_scores_timed, moc_scores_banks): which kernel form a shape gets, with
// how much dynamic LDS, over which grid and in chunks of how many slides -- decided once, here, for both entries.  Plain
// C++17, no HIP name: tests/native/score_plan_host.cpp includes it with g++ and prints the plan over a grid of shapes
// (tests/test_score_plan_cpu.py holds that against the formulas the entries carried before this header existed).
//
// The KERNELS do not include the layouts below: scores_stream_kernel and scores_banks_kernel carve their LDS with
// expressions of their own (DESIGN.md "Where a new score kernel goes" has the reason: their device code moves when the
// carve is shared).  StreamLds states the same layout for the host; the test checks order, extents and alignment.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/moc_hip.h"

constexpr size_t SCORE_MAX_LDS = 160 * 1024;        // the dynamic-LDS limit every score kernel is raised to

static inline int bank_nt(int Ce) { return (Ce + 15) / 16; }
// one n-tile (16 columns) of the image moc_prepare_bank writes: 16-bit bags hold three 16-bit terms per weight in
// 1 KiB B fragments of 32 rows of K, fp32 bags one fp32 in fragments of 16 rows
static inline size_t score_img_bytes(int D, int dtype) {
    return dtype != MOC_F32 ? (size_t)(D / 32) * 3 * 1024 : (size_t)(D / 16) * 1024;
}
// the four waves' 16 x (16 NT + 1) epilogue tiles
static inline size_t score_tile_bytes(int NT) { return (size_t)4 * 16 * (NT * 16 + 1) * sizeof(float); }
// n-tiles the streaming form takes.  bf16 stops at 3: with 4, the 12 B fragments per batch leave hipcc short of registers
// and it parks in-flight load destinations in AGPRs (tests/test_isa_hazards_cpu.py)
static inline int score_stream_nt_max(int dtype) { return dtype != MOC_F32 ? 3 : 4; }

// ---- wide banks (scores_wide_kernel, scores_wide_ring_kernel)
constexpr int WD_R = 4;               // row tiles per wave
// k-steps (of 32 columns) per chunk: up to 6 n-tiles one k-step per chunk and TWO workgroups per CU (62 KiB of LDS
// and at most 246 registers each: one's DMA waits and row epilogues run beside the other's MFMAs, +12 % at
// 5 n-tiles); wider banks need the registers of a whole SIMD and take two k-steps per chunk
constexpr int wd_kc(int NT) { return NT <= 6 ? 1 : 2; }

// ---- the streaming form's dynamic LDS (scores_stream_kernel, scores_banks_kernel), for a launch over n slides:
//   [NT images][4 waves x 16 x (16 NT + 1) floats][n x 8 B first slot][n x 8 B first X row][(n + 1) x 4 B tile prefix]
//   [n x 4 B kept rows][slack]
// 24 bytes a slide and one more prefix word, which the 16 bytes of slack hold.
struct StreamLds {
    size_t img;      // score_img_bytes
    int NT;
    static constexpr size_t SLIDE = 24, SLACK = 16;
    size_t images() const { return 0; }
    size_t tiles() const { return (size_t)NT * img; }
    size_t meta() const { return tiles() + score_tile_bytes(NT); }
    size_t first_slot(int) const { return meta(); }
    size_t first_row(int n) const { return meta() + (size_t)8 * n; }
    size_t prefix(int n) const { return meta() + (size_t)16 * n; }
    size_t kept_rows(int n) const { return prefix(n) + (size_t)4 * (n + 1); }
    size_t meta_end(int n) const { return kept_rows(n) + (size_t)4 * n; }
    // s_counter of the ticketed walk, (int*)meta + 6 n + 1 in the kernel: the word behind the metadata, that is inside
    // the slack whenever the launch's n is at most the chunk the LDS was sized for
    size_t counter(int n) const { return meta_end(n); }
    size_t fixed() const { return meta() + SLACK; }
    size_t bytes(int n) const { return fixed() + SLIDE * n; }
    bool fits() const { return fixed() + SLIDE <= SCORE_MAX_LDS; }      // image, tiles and at least one slide
    int chunk_max() const { return fits() ? (int)((SCORE_MAX_LDS - fixed()) / SLIDE) : 0; }
};

// banks of at most 16 columns one streaming launch serves (moc_scores_banks_max): the n-tile limit, then LDS
static inline int score_banks_max(int D, int dtype) {
    int g = score_stream_nt_max(dtype);
    while (g > 0 && !StreamLds{score_img_bytes(D, dtype), g}.fits()) --g;
    return g;
}

// ---- the LDS-DMA ring form (scores_ring_kernel, moc_scores_ring.hip): fp32 bags, one n-tile, one persistent workgroup
// per CU of one loader wave and three consumer waves.  The loader moves 16-row x 1 KiB units (the streaming form's unit:
// sixteen 1 KiB A fragments) into ring slots by LDS-DMA; nothing of a tile lives in registers, so the workgroup is small
// enough in registers AND in LDS to share its CU with the training forward.  Its dynamic LDS:
//   [image][slots x 16 KiB][3 waves x 16 x 17 floats][n x 8 B first slot | n x 8 B first X row | (n + 1) x 4 B tile prefix
//   | n x 4 B kept rows][pad to 16][slots x 16 B tile descriptor][slots x 4 B FULL][slots x 4 B FREE]
// The slot count is what is left of the CU's LDS beside ONE workgroup of the training forward at D = 512
// (fks_lds_bytes(512), moc_meta_forward.hip, which asserts the figure here): at D = 256 and 32 slides four slots, at
// D = 512 three.  (The step kernels' launch limit, lds::TILE_MAX_LDS, is the whole CU and leaves room for nothing; a step
// workgroup of the benchmark's shape holds 39 KiB and fits in the same room.)  Fewer than three slots -- one in flight,
// one published, one being read -- and the form does not apply.
constexpr size_t SCORE_RING_BESIDE_LDS = 72256;     // fks_lds_bytes(512)
constexpr size_t SCORE_RING_SLOT = 16 * 1024;
constexpr int SCORE_RING_SLOTS_MIN = 3, SCORE_RING_SLOTS_MAX = 8;
struct RingLds {
    size_t img;
    int n, slots;
    size_t ring() const { return img; }
    size_t tiles() const { return ring() + slots * SCORE_RING_SLOT; }
    size_t meta() const { return tiles() + (size_t)3 * 16 * 17 * sizeof(float); }
    size_t desc() const { return (meta() + (size_t)24 * n + 4 + 15) & ~(size_t)15; }
    size_t full() const { return desc() + (size_t)16 * slots; }
    size_t free_() const { return full() + (size_t)4 * slots; }
    size_t bytes() const { return free_() + (size_t)4 * slots; }
};
// slots of a launch over n slides (0: the ring form does not apply)
constexpr int score_ring_slots(size_t img, int n) {
    const size_t fixed = img + (size_t)3 * 16 * 17 * sizeof(float) + (size_t)24 * n + 4 + 15;
    const size_t room = SCORE_MAX_LDS - SCORE_RING_BESIDE_LDS;
    if (fixed >= room) return 0;
    const size_t s = (room - fixed) / (SCORE_RING_SLOT + 24);
    return s < (size_t)SCORE_RING_SLOTS_MIN ? 0 : s > (size_t)SCORE_RING_SLOTS_MAX ? SCORE_RING_SLOTS_MAX : (int)s;
}

enum { SCORE_STREAM, SCORE_WIDE_RING, SCORE_WIDE, SCORE_GENERIC, SCORE_RING };
enum {
    SCORE_PLAN_OK,
    SCORE_PLAN_SLIDES_LDS,     // streaming, one n-tile: the slides' metadata does not fit in one launch (`need` bytes)
    SCORE_PLAN_RESERVED,       // reserved compute units without a ticket array
    SCORE_PLAN_ROW_LDS,        // generic: one image and the tiles do not fit (`need` bytes)
    SCORE_PLAN_NO_STREAM,      // banks_entry, and the streaming form does not apply (`need`: one bank, one slide)
    SCORE_PLAN_RING_TICKET     // MOC_SCORES_RING with a ticket array or a reserved set: the ring form walks statically, everywhere
};

struct ScoreShape {
    int D, dtype, NT, n_slides;
    int64_t total_rows;
    int max_rows;
    bool ticket, reserved;     // moc_batch_t.tile_ticket / cu_reserved given
    int lookahead_cap;         // workgroups of a launch with a ticket array, at most (0: no cap)
    bool banks_entry;          // moc_scores_banks: the streaming static form or nothing; one n-tile may go in chunks
    bool ring = false;         // moc_batch_t.flags & MOC_SCORES_RING: the ring form where it applies (fp32, one n-tile)
};

struct ScorePlan {
    int form;
    int unit;                  // streaming: NF, 16-byte loads per lane and unit; generic: CH, columns per image chunk; ring: slots
    int NT;
    bool ticketed;             // streaming: the ticketed walk, with the batch's reserved set; else both stay out
    size_t smem;
    int chunk;                 // streaming: slides per launch
    int gx, gy;                // streaming: gx persistent workgroups
    int tpw;                   // ScoresArgs.tpw
    int err;
    size_t need;
};

static inline ScorePlan score_plan(const ScoreShape& q) {
    ScorePlan P = {};
    const bool bf = q.dtype != MOC_F32;          // 16-bit storage (bf16 or fp16): 3-term image, K = 32 per MFMA
    const size_t img = score_img_bytes(q.D, q.dtype);
    P.NT = q.NT;
    P.gy = 1;
    // the ring form, only for a batch that asks for it: never beside a ticket or a reserved set (it has no ticketed walk and
    // needs no free CUs); shapes it does not cover keep the forms below
    if (q.ring && !q.banks_entry) {
        if (q.ticket || q.reserved) {
            P.err = SCORE_PLAN_RING_TICKET;
            return P;
        }
        const int slots = (!bf && q.NT == 1) ? score_ring_slots(img, q.n_slides) : 0;
        if (slots > 0) {
            P.form = SCORE_RING;
            P.unit = slots;
            P.chunk = q.n_slides;
            P.smem = RingLds{img, q.n_slides, slots}.bytes();
            const int64_t tiles = (q.total_rows + 15) / 16 + 2 * (int64_t)q.n_slides;
            P.gx = tiles < 256 ? (int)tiles : 256;         // one workgroup per CU
            return P;
        }
    }
    // streaming form: persistent workgroups over the flat tile list, the whole bank image (all NT n-tiles) resident in
    // LDS.  Applies while image + epilogue tiles + at least one slide's metadata fit; a batch with more slides than fit
    // beside the image goes out in chunks.
    const StreamLds L{img, q.NT};
    if (q.NT <= score_stream_nt_max(q.dtype) && L.fits()) {
        P.form = SCORE_STREAM;
        // fp32 rows are a multiple of 1 KiB because D % 256 == 0: NF = 8 is for 16-bit rows of an odd multiple of 512 B
        P.unit = (q.D * (bf ? 2 : 4)) % 1024 == 0 ? 16 : 8;
        P.chunk = q.n_slides < L.chunk_max() ? q.n_slides : L.chunk_max();
        P.smem = L.bytes(P.chunk);
        if (!q.banks_entry && q.NT == 1 && P.chunk != q.n_slides) {
            P.err = SCORE_PLAN_SLIDES_LDS;
            P.need = L.bytes(q.n_slides);
            return P;
        }
        const int64_t tiles = (q.total_rows + 15) / 16 + 2 * (int64_t)q.n_slides;    // upper bound from the host-known sizes
        int wgs = (int)((tiles + 3) / 4);
        const int resident = 256 * (P.smem <= 80 * 1024 ? 2 : 1);
        if (wgs > resident) wgs = resident;
        // A look-ahead launch (tile_ticket set: it runs beside the meta-steps of the pass before) is kept to fewer
        // persistent workgroups: every wave of this kernel holds up to 32 KiB of loads in flight, 2,048 waves 64 MB --
        // several times what 8 TB/s x the memory latency can use, and every dependent load of a meta-step queues
        // behind them (profiles/NOTES.md round 4: the steps crawl while a full-width score pass streams, whether or
        // not it leaves them compute units).
        if (q.ticket && q.lookahead_cap > 0 && wgs > q.lookahead_cap) wgs = q.lookahead_cap;
        P.gx = wgs;
        if (q.reserved && !q.ticket) {
            P.err = SCORE_PLAN_RESERVED;
            return P;
        }
        // (four n-tiles, fp32 only: the ticketed form leaves the compiler short of registers and it re-uses load
        // destinations still in flight -- tests/test_isa_hazards_cpu.py; that shape keeps the static walk, whole chip)
        P.ticketed = q.ticket && q.NT < 4;
        return P;
    }
    if (q.banks_entry) {
        P.err = SCORE_PLAN_NO_STREAM;
        P.need = StreamLds{img, 1}.bytes(1);
        return P;
    }
    P.chunk = q.n_slides;
    P.gy = q.n_slides;
    // wide banks on 16-bit storage: the K-split form (every bag row read once)
    if (bf && q.NT >= 4 && q.NT <= 8 && q.D % 64 == 0) {
        const size_t kc = wd_kc(q.NT);
        const size_t buf = (size_t)q.NT * kc * 3 * 1024 + (size_t)4 * WD_R * kc * 1024;
        const size_t tiles = score_tile_bytes(q.NT);
        const size_t smem_w = 2 * buf > tiles ? 2 * buf : tiles;
        P.gx = (q.max_rows + 4 * WD_R * 16 - 1) / (4 * WD_R * 16);
        if (q.NT <= 5) {                                               // (6 n-tiles: the register ring spills)
            const size_t ring = (size_t)3 * ((size_t)((q.NT * 3 + 3) / 4) * 4 * 1024);         // three image slots
            P.form = SCORE_WIDE_RING;
            P.smem = ring > tiles ? ring : tiles;
            return P;
        }
        if (smem_w < SCORE_MAX_LDS) {
            P.form = SCORE_WIDE;
            P.smem = smem_w;
            return P;
        }
    }
    // generic: one n-tile of the image at a time, a wave per 16-row tile
    P.form = SCORE_GENERIC;
    P.unit = q.D % 512 == 0 ? 512 : 256;
    P.tpw = 1;
    P.smem = img + score_tile_bytes(q.NT);
    P.gx = (q.max_rows + 64 * P.tpw - 1) / (64 * P.tpw);
    if (P.smem > SCORE_MAX_LDS) {
        P.err = SCORE_PLAN_ROW_LDS;
        P.need = P.smem;
    }
    return P;
}
