// The step kernels' dynamic LDS (the kernels of moc_step_pool.hip, moc_step_fused.hip and moc_step_tiles.hip; step_plan
// in moc_meta.hip): ONE layout per kernel, byte offsets from the start of dynamic LDS plus `bytes`, the total to launch with.  The host sizes the launch with the same function the kernel carves with, so a
// carve cannot move without the launch moving with it.  Plain C++17, no HIP name: tests/native/step_lds_host.cpp
// includes it with g++ and checks order, extents, alignment and the totals over a grid of shapes.
//
// Rules: fields stand in offset order; a round-up happens on an OFFSET, here, never on a pointer in a kernel (a pointer
// rebuilt from an integer is a flat pointer to the compiler, and every access through it a flat_ operation); `bytes`
// keeps the hand-tallied slack of the formulas these layouts replaced, as a named pad per layout -- the tile-record step
// sits 928 bytes under the four-workgroups-per-CU line at the benchmark's shape, and trimming a pad is a change with a
// measurement of its own.
#pragma once

#if defined(__HIPCC__)
#define MOC_HD __host__ __device__
#else
#define MOC_HD
#endif

namespace moc_step_lds {

constexpr int H = 64;                             // hidden units (MOC_HIDDEN: asserted in moc_step_shared.h, which includes this)
constexpr int FIN_CHUNK = 256;                    // finish_kernel: pairs whose H1 rows are staged in LDS at a time (64 KiB)
constexpr int PS_CAP_MAX = 1024;                  // candidate list entries per class (the launch picks cap <= this)
constexpr int TILE_CL = 64;                       // tile-record step: candidates per class
constexpr int TILE_SINK = 1024;                   // ... and the LDS nobody reads (the prefetch's LDS-DMA destination)
constexpr int WD_PCH_MIN = 128;                   // wide step: pairs per chunk of the W1 gradient, at least

// the dynamic-LDS limit each kernel is raised to, and every launch is checked against
constexpr int FS_MAX_DYN_LDS = 160 * 1024 - 64;   // the one-launch step kernels also hold a few static LDS words
constexpr int FINISH_MAX_LDS = 159 * 1024;        // finish_kernel: 1 KiB of static LDS (dpool)
constexpr int POOL_STEP_MAX_LDS = 160 * 1024;     // pool_step_kernel
constexpr int NARROW_MAX_LDS = FS_MAX_DYN_LDS, TILE_MAX_LDS = FS_MAX_DYN_LDS, WIDE_MAX_LDS = FS_MAX_DYN_LDS;

MOC_HD constexpr int lds_up(int off, int align) { return (off + align - 1) & ~(align - 1); }

// candidate list entries per class: PS_CAP of pool_step_kernel, the narrow and the tile-record step
MOC_HD constexpr int step_cap(int C) { return C <= 8 ? PS_CAP_MAX : PS_CAP_MAX / 2; }

// ------------------------------------------------------------------ the pooling block (pool_phase)
// What pool_step_kernel, pool_w1_step_kernel and pool_w1_step_wide_kernel hand to pool_phase.  The lists stand apart from
// the rest in the wide kernel (they share its `region`), so both starts are given.
struct PoolBlockLds {
    int list;        // u64 [C][cap] candidate keys                          (8)
    int wmax;        // u64 [C][16] per-wave maxima                           (8)
    int pooled_s;    // float [C] pooled logits
    int dpool;       // float [C] d loss / d pooled
    int ncand;       // int [C] candidate counts
    int topk_s;      // int [C][K] pooled rows in value order
    int end;
};
MOC_HD constexpr PoolBlockLds pool_block_lds(int list, int wmax, int C, int K) {
    PoolBlockLds L = {};
    L.list = list;
    L.wmax = wmax;
    L.pooled_s = L.wmax + C * 16 * 8;
    L.dpool = L.pooled_s + C * 4;
    L.ncand = L.dpool + C * 4;
    L.topk_s = L.ncand + C * 4;
    L.end = L.topk_s + C * K * 4;
    return L;
}

// ------------------------------------------------------------------ finish_kernel (train; evaluation takes no dynamic LDS)
struct FinishLds {
    int dz;          // float [P][4]                                          (16)
    int prow;        // int [P] position s of the pair's row
    int H1s;         // float [FIN_CHUNK][H]
    int W2s;         // float [4][H]
    int pad, bytes;
};
MOC_HD constexpr FinishLds finish_lds(int C, int K, int train) {
    const int P = train ? C * K : 0;
    FinishLds L = {};
    L.dz = 0;
    L.prow = L.dz + P * 16;
    L.H1s = L.prow + P * 4;
    L.W2s = L.H1s + FIN_CHUNK * H * 4;
    L.pad = 0;
    L.bytes = train ? L.W2s + 4 * H * 4 : 0;
    return L;
}

// finish_lds(..).bytes <= FINISH_MAX_LDS exactly up to this many pairs (topk has no other bound: the launch checks this)
constexpr int FINISH_MAX_PAIRS = (FINISH_MAX_LDS - (FIN_CHUNK + 4) * H * 4) / 20;
static_assert(finish_lds(1, FINISH_MAX_PAIRS, 1).bytes <= FINISH_MAX_LDS && finish_lds(1, FINISH_MAX_PAIRS + 1, 1).bytes > FINISH_MAX_LDS, "");

// ------------------------------------------------------------------ pool_step_kernel
struct PoolStepLds {
    PoolBlockLds pool;
    int dz;          // float [P][4]   (train; evaluation: P = 0)
    int H1s;         // float [P][H]
    int dhs;         // float [P][H]
    int W2s;         // float [4][H]
    int pad, bytes;
};
MOC_HD constexpr PoolStepLds pool_step_lds(int C, int K, int cap, int train) {
    const int P = train ? C * K : 0;
    PoolStepLds L = {};
    L.pool = pool_block_lds(0, C * cap * 8, C, K);
    L.dz = L.pool.end;
    L.H1s = L.dz + P * 16;
    L.dhs = L.H1s + P * H * 4;
    L.W2s = L.dhs + P * H * 4;
    L.pad = 0;
    L.bytes = L.W2s + 4 * H * 4;
    return L;
}

// ------------------------------------------------------------------ pool_w1_step_kernel (narrow)
constexpr int NARROW_PAD = 16;                    // counted for the round-ups of row_s (to 8) and xs (to 16)
struct NarrowStepLds {
    PoolBlockLds pool;
    int dz;          // float [P][4]
    int H1s;         // float [P][H]
    int dhs;         // float [P][H]
    int W2s;         // float [4][H]
    int row_s;       // int64 [P] bag rows of the pairs                       (8)
    int xs;          // float [P][D] the pairs' rows                          (16)
    int pad, bytes;
};
MOC_HD constexpr NarrowStepLds narrow_step_lds(int C, int K, int D, int cap) {
    const int P = C * K;
    NarrowStepLds L = {};
    L.pool = pool_block_lds(0, C * cap * 8, C, K);
    L.dz = L.pool.end;
    L.H1s = L.dz + P * 16;
    L.dhs = L.H1s + P * H * 4;
    L.W2s = L.dhs + P * H * 4;
    const int row_raw = L.W2s + 4 * H * 4;
    L.row_s = lds_up(row_raw, 8);
    L.xs = lds_up(L.row_s + P * 8, 16);
    const int end = L.xs + P * D * 4;
    L.bytes = row_raw + P * 8 + P * D * 4 + NARROW_PAD;      // the arrays, unrounded, and the pad
    L.pad = L.bytes - end;
    return L;
}

// ------------------------------------------------------------------ pool_w1_step_tiles_kernel
// The 16-byte things first.  The sink is the last member: TileStepArgs::sink_off is `sink`.
constexpr int TILE_PAD = 64;                      // counted for no round-up (this carve has none); dhs, carved as [PD], is counted
                                                  // as [P + 4] on top of it -- both kept: the bytes of a launch do not move here
struct TileStepLds {
    int PD;          // floats of dhs: P rounded up to four
    int plam;        // float4 [P] pairs' gates                               (16)
    int psc;         // float4 [P] ... candidate scores                       (16)
    int xs;          // float [P][256] pairs' row pieces                      (16)
    int dhs;         // float [PD] dh of unit h                               (16)
    int dz;          // float [P][4]                                          (16)
    int list;        // u64 [C][cap]                                          (8)
    int t0s;         // u64 [C] the bound T0 (as a key)                       (8)
    int prid;        // int64 [P]                                             (8)
    int lsrc;        // int [C][TILE_CL] record of a candidate
    int topv;        // float [C][16]
    int pooled_s;    // float [C]
    int dpool;       // float [C]
    int ncand;       // int [C] the fall-back's counters (the records' lists are placed by ballot)
    int flagc;       // int [C] 1: the records cannot prove exactness
    int topk_s;      // int [C][K]
    int h1s;         // float [P]
    int w2s;         // float [4]
    int pad;
    int sink;        // TILE_SINK bytes
    int bytes;
};
MOC_HD constexpr TileStepLds tile_step_lds(int C, int K, int cap) {
    const int P = C * K;
    TileStepLds L = {};
    L.PD = (P + 3) & ~3;
    L.plam = 0;
    L.psc = L.plam + P * 16;
    L.xs = L.psc + P * 16;
    L.dhs = L.xs + P * 256 * 4;
    L.dz = L.dhs + L.PD * 4;
    L.list = L.dz + P * 16;
    L.t0s = L.list + C * cap * 8;
    L.prid = L.t0s + C * 8;
    L.lsrc = L.prid + P * 8;
    L.topv = L.lsrc + C * TILE_CL * 4;
    L.pooled_s = L.topv + C * 16 * 4;
    L.dpool = L.pooled_s + C * 4;
    L.ncand = L.dpool + C * 4;
    L.flagc = L.ncand + C * 4;
    L.topk_s = L.flagc + C * 4;
    L.h1s = L.topk_s + P * 4;
    L.w2s = L.h1s + P * 4;
    L.pad = (P + 4 - L.PD) * 4 + TILE_PAD;                   // dhs is counted as [P + 4]
    L.sink = L.w2s + 4 * 4 + L.pad;
    L.bytes = L.sink + TILE_SINK;
    return L;
}

// ------------------------------------------------------------------ pool_w1_step_wide_kernel
constexpr int WIDE_PAD = 16 + 8;                  // counted for the round-ups of dz (to 16) and prow_s (to 8)
struct WideStepLds {
    int PM;            // pairs per plane of the ReLU masks: P + 16 rounded up to four
    int region;        // u64 [C][cap] lists, then raw [pch][D / 16] row pieces of a chunk, then `part`      (16)
    int region_bytes;
    int part;          // float [8][4][64] the halves of a tile product meet here behind the chunk loop       (16)
    PoolBlockLds pool; // (its lists: `region`)
    int dz;            // float [P + 16][4]: sixteen rows of slack behind the pairs, the product walks them in sixteens  (16)
    int h1o;           // float [P][4]
    int mask;          // u32 [2][PM]: bits of hidden units 0..31 | 32..63                                    (16)
    int sidx_s;        // int [P]
    int W2s;           // float [4][H]
    int red;           // float [32]
    int prow_s;        // int64 [P]                                                                           (8)
    int pad, bytes;
};
// list entries per class of the wide step: the lists of all classes within 64 KiB
MOC_HD constexpr int wide_cap(int C) {
    int cap = 1024;
    while (cap > 64 && C * cap * 8 > 64 * 1024) cap >>= 1;
    return cap;
}
// (the kernel's form: the region's size reaches it as an argument, as the sink's offset reaches the tile-record step)
MOC_HD constexpr WideStepLds wide_step_lds_behind(int C, int K, int region_bytes) {
    const int P = C * K;
    WideStepLds L = {};
    L.PM = (P + 16 + 3) & ~3;
    L.region = 0;
    L.region_bytes = region_bytes;
    L.part = L.region;
    L.pool = pool_block_lds(L.region, L.region_bytes, C, K);
    L.dz = lds_up(L.pool.end, 16);
    L.h1o = L.dz + (P + 16) * 16;
    L.mask = L.h1o + P * 16;
    L.sidx_s = L.mask + L.PM * 2 * 4;
    L.W2s = L.sidx_s + P * 4;
    L.red = L.W2s + 4 * H * 4;
    L.prow_s = lds_up(L.red + 32 * 4, 8);
    const int end = L.prow_s + P * 8;
    // the arrays, unrounded, a mask plane counted as [P + 20], and the pad
    L.bytes = L.region_bytes + (L.pool.end - L.pool.wmax) + (P + 16) * 16 + P * 16 + 2 * (P + 20) * 4 + P * 4 + 4 * H * 4 +
              32 * 4 + P * 8 + WIDE_PAD;
    L.pad = L.bytes - end;
    return L;
}
MOC_HD constexpr WideStepLds wide_step_lds(int C, int K, int D, int esz, int pch, int cap) {
    const int lists = C * cap * 8;
    const int rows = pch * ((D / 16) * esz);                 // row pieces of one chunk (dh is formed in the product loop)
    return wide_step_lds_behind(C, K, lds_up(lists > rows ? lists : rows, 16));
}
// pairs per chunk of the W1 gradient: all C * K of them in ONE chunk when its row pieces fit beside the rest
// (EBRAINS-30: 300 pairs, 38 KiB at fp32; the 64-way shape: 640 pairs, 80 KiB at fp16) -- one gather round trip and one
// barrier instead of one per chunk; else the largest multiple of 32 that fits, at least WD_PCH_MIN
MOC_HD constexpr int wide_pch(int C, int K, int D, int esz) {
    int pch = (C * K + 31) & ~31;
    while (pch > WD_PCH_MIN && wide_step_lds(C, K, D, esz, pch, wide_cap(C)).bytes > WIDE_MAX_LDS) pch -= 32;
    return pch < WD_PCH_MIN ? WD_PCH_MIN : pch;
}

// Anchors, from the formulas these layouts replaced (the test walks a grid of shapes for totals, order and alignment)
static_assert(tile_step_lds(2, 10, step_cap(2)).bytes == 40032, "the benchmark's shape: four workgroups per CU need <= 40,960 each");
static_assert(narrow_step_lds(15, 4, 256, step_cap(15)).bytes == 158420 && narrow_step_lds(8, 8, 256, step_cap(8)).bytes > NARROW_MAX_LDS,
              "narrow: 60 pairs fit, 64 pairs at D = 256 take the three-launch step");
static_assert(wide_pch(61, 8, 1024, 4) == 480 && wide_step_lds(61, 8, 1024, 4, 480, wide_cap(61)).bytes == 160340, "wide: 488 pairs in two chunks");
static_assert(8 * 4 * 64 * 4 <= WD_PCH_MIN * (512 / 16) * 2, "the partial sums fit the smallest region");

}  // namespace moc_step_lds
