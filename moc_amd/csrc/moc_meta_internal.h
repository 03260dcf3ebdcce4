// What the sources of phase B share: moc_meta_forward.hip (the meta forward), moc_meta.hip (the training entries and which
// step kernel they run) and the step kernels' sources moc_step_{pool,fused,tiles}.hip.  Private to those sources; nothing
// here is exported from the library.
#pragma once
#include <mutex>   // std::call_once: both halves raise their kernels' LDS limits once, from any thread
#include "moc_common.h"

struct P2pArgs;   // the in-kernel gradient exchange's kernel argument (moc_p2p_proto.h)

namespace moc_meta_internal __attribute__((visibility("hidden"))) {

constexpr int H = MOC_HIDDEN;

// ------------------------------------------------------------------ tile records (round 4)
// The step kernel used to request and rank ALL S x C mixed scores of the slide the forward had just written -- a memory
// round trip of sixteen loads per thread, then the candidate search over them on sixteen waves of one CU.  The forward's
// workgroups now leave, per 16-row tile and class, the tile's TILE_R largest scores as RECORDS -- the key (score | ~row),
// the row's id in the bag, its four gates and its four candidate scores: everything the backward needs of a pooled row
// except its hidden activations and the row itself -- plus rho = the key of the tile's (TILE_R + 1)-th largest score.
// The step kernel reads a class's ceil(S / 16) x TILE_R keys with ONE wave, finds a lower bound T0 of the K-th largest
// score (the K-th largest of sixteen group maxima: group g = the tiles g, g + 16, ...) and pools among the records >= T0.
// That is EXACT whenever every score >= T0 is a record, i.e. when no tile holds more than TILE_R of them: rho < T0 for
// every tile -- checked; otherwise (and for more than 64 candidates) the kernel falls back to the full scores, which the
// forward still writes.  Same rows, same (value desc, row asc) order, same sum: same bits.
constexpr int TILE_R = 4;
constexpr int MOC_MAX_RUNS = 16;        // meta-learners one launch can serve (moc_train_steps_runs)
constexpr int MOC_HP_RUNS = 8;          // ... with Adam coefficients per run (moc_train_steps_runs_hp; TileStepArgsRunsHp, moc_step_tiles.hip)
// floats of one meta-learner: W1 [H][D], b1 [H], W2 [4][H], b2 [4]
constexpr int64_t n_params(int D) { return (int64_t)MOC_HIDDEN * D + MOC_HIDDEN + 4 * MOC_HIDDEN + 4; }
constexpr int MOC_TILE_PATH_RECORDS = 1000001, MOC_TILE_PATH_FULL = 1000002;   // left in ws->n_pair[0] by the tile-record step
struct TileWs {
    float4* lam;                 // [slots] gates of the record's row
    float4* sc;                  // [slots] its candidate scores s_p[c], s_sigma[c], s_delta, s_beta
    unsigned long long* key;     // [slots] (moc_key_desc(score) << 32) | ~row; high word 0: empty
    int64_t* rid;                // [slots] sel_row of the row
    uint32_t* rho;               // [slots / TILE_R] high word of the (TILE_R + 1)-th largest key of the (tile, class); 0: none
};
// Slide b owns the slots from slot0 = ((row_off[b] >> 4) + b) * C * TILE_R on: C * cap * TILE_R of them, cap = ceil(rows of
// the slide / 16), class-major: record r of (tile x, class c) is slot0 + (c * cap + x) * TILE_R + r (a class's records are
// contiguous: one wave reads them); rho of (x, c) is entry slot0 / TILE_R + c * cap + x.
__host__ __device__ inline int64_t tile_slots(int64_t total_rows, int n_slides, int C) {
    return ((total_rows >> 4) + n_slides + 2) * (int64_t)C * TILE_R;
}
__host__ __device__ inline TileWs tile_carve(void* p, int64_t ns) {
    TileWs T;
    unsigned char* q = (unsigned char*)p;
    T.lam = (float4*)q; q += ns * 16;
    T.sc = (float4*)q; q += ns * 16;
    T.key = (unsigned long long*)q; q += ns * 8;
    T.rid = (int64_t*)q; q += ns * 8;
    T.rho = (uint32_t*)q;
    return T;
}
__host__ __device__ inline size_t tile_bytes(int64_t ns) { return (size_t)ns * 48 + (size_t)(ns / TILE_R) * 4 + 16; }

// Epilogue of a forward workgroup: thread t = class * 16 + row holds the mixed score v of (row0 + row, class); the 16 rows
// of a class are 16 consecutive lanes (one DPP row).  Every lane ranks its key (score word | ~row; keys are unique: absent
// rows carry (0 | ~row)) among the row's sixteen, ranks 0 .. TILE_R-1 write their record, rank TILE_R writes rho.
// tile_rank16, the rank: each lane counts the row's score words above its own -- fifteen row rotations of one DPP move and
// one compare.  That count is the rank wherever no two present rows of the tile share a score word; an absent row (score
// word 0, rows at and past S: the tail of the tile) has rank = its place in the tile whatever the others hold, since every
// earlier row beats it by its score or, score words equal, by its row.  A count is never above the true rank, and the true
// ranks of a tile sum to 0 + ... + 15 = 120: the counts are the ranks exactly when the row's sum is 120 (four DPP adds).
// Otherwise -- equal scores, rare -- the wave ranks again on the whole key, two moves and a two-word compare per rotation
// (the only form until the tail was shortened: 105 instructions against 50); the branch is on a ballot, uniform over the
// wave.  `row`: the row in the slide, a multiple of 16 plus the lane's place.
__device__ __forceinline__ int tile_rank16(bool ok, float v, int row) {
    const unsigned hi = ok ? moc_key_desc(v) : 0u;
    int rank = 0;
#define MOC_ROR(n) rank += ((unsigned)__builtin_amdgcn_update_dpp(0, (int)hi, 0x120 + n, 0xf, 0xf, false) > hi) ? 1 : 0;
    MOC_ROR(1) MOC_ROR(2) MOC_ROR(3) MOC_ROR(4) MOC_ROR(5) MOC_ROR(6) MOC_ROR(7) MOC_ROR(8)
    MOC_ROR(9) MOC_ROR(10) MOC_ROR(11) MOC_ROR(12) MOC_ROR(13) MOC_ROR(14) MOC_ROR(15)
#undef MOC_ROR
    if (!ok) rank = row & 15;
    int sum = rank;
    sum += __builtin_amdgcn_update_dpp(0, sum, 0x128, 0xf, 0xf, false);
    sum += __builtin_amdgcn_update_dpp(0, sum, 0x124, 0xf, 0xf, false);
    sum += __builtin_amdgcn_update_dpp(0, sum, 0x122, 0xf, 0xf, false);
    sum += __builtin_amdgcn_update_dpp(0, sum, 0x121, 0xf, 0xf, false);
    if (__builtin_amdgcn_ballot_w64(sum != 120) != 0) {
        const unsigned lo = ~(unsigned)row;
        rank = 0;
#define MOC_ROR(n)                                                                                              \
    {                                                                                                           \
        const unsigned ohi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)hi, 0x120 + n, 0xf, 0xf, false);     \
        const unsigned olo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)lo, 0x120 + n, 0xf, 0xf, false);     \
        rank += (ohi > hi || (ohi == hi && olo > lo)) ? 1 : 0;                                                  \
    }
        MOC_ROR(1) MOC_ROR(2) MOC_ROR(3) MOC_ROR(4) MOC_ROR(5) MOC_ROR(6) MOC_ROR(7) MOC_ROR(8)
        MOC_ROR(9) MOC_ROR(10) MOC_ROR(11) MOC_ROR(12) MOC_ROR(13) MOC_ROR(14) MOC_ROR(15)
#undef MOC_ROR
    }
    return rank;
}
// the stores of a lane whose rank is known (a caller with a store of its own puts it in front: they leave back to back)
__device__ __forceinline__ void tile_store(const TileWs& T, int64_t tc, int rank, bool ok, float v, int row, int64_t rid, float4 lam, float4 sc) {
    const unsigned hi = ok ? moc_key_desc(v) : 0u, lo = ~(unsigned)row;
    if (rank < TILE_R) {
        const int64_t slot = tc * TILE_R + rank;
        T.key[slot] = ((unsigned long long)hi << 32) | lo;
        T.rid[slot] = rid;
        T.lam[slot] = lam;
        T.sc[slot] = sc;
    } else if (rank == TILE_R) {
        T.rho[tc] = hi;
    }
}
__device__ __forceinline__ void tile_emit(const TileWs& T, int64_t tc, bool ok, float v, int row, int64_t rid, float4 lam, float4 sc) {
    tile_store(T, tc, tile_rank16(ok, v, row), ok, v, row, rid, lam, sc);
}

// An entry of an array inside the kernel's (single, by-value) argument struct, read straight from the kernel-argument
// segment by a uniform index: indexing the struct itself with a runtime index makes hipcc copy all of it to scratch.
template <typename T>
__device__ __forceinline__ T kernarg_at(size_t off) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(4))) const char* kp_t;
    kp_t p = (kp_t)__builtin_amdgcn_kernarg_segment_ptr();
    return *(__attribute__((address_space(4))) const T*)(p + off);
#else
    return T();
#endif
}

// ---- W1 image (the forward reads it, the step's W1 update rewrites it) -----------------------
// The forward's B operand is W1^T: B[k][n] = W1[n][k].  Read from the [H][D] parameter tensor,
// a wave's fragment load touches 64 scattered 16-B pieces (16 rows 2 KB apart) and the address
// unit, not HBM, sets the pace.  So the kernels keep a second copy in fragment order -- one
// contiguous 1 KiB per wave-load -- rewritten by the W1 update itself, hence always in sync:
//   bf16 and fp32 bags: [nt][kk][term][lane][8] bf16, element j of lane l = term t of W1[nt*16 + (l&15)][kk*32 + (l>>4)*8 + j]
//              (hi/mid/lo split, 24 mantissa bits: bf16 MFMA with fp32-exact products; fp32 bags split their rows
//              the same way, fwd_split4 / fwd_mfma6 in moc_meta_forward.hip)
//   fp16 bags: as bf16, the three fp16 terms of W1 * 2^10 (moc_common.h); the forward scales back
template <bool F16>
__device__ __forceinline__ void w1_image_store_half(unsigned char* img, int D, int h, int d, float w) {
    const int KK = D / 32;
    const int nt = h >> 4, kk = d >> 5, lane = (((d & 31) >> 3) << 4) | (h & 15), j = d & 7;
    uint16_t* o = reinterpret_cast<uint16_t*>(img) + ((size_t)(nt * KK + kk) * 3 * 64 + lane) * 8 + j;
    uint16_t hi, mid, lo;
    moc_split3<F16>(w, MOC_F16_W1_SCALE, hi, mid, lo);
    o[0] = hi;
    o[64 * 8] = mid;
    o[2 * 64 * 8] = lo;
}
__device__ __forceinline__ void w1_image_store_bf16(unsigned char* img, int D, int h, int d, float w) {
    w1_image_store_half<false>(img, D, h, d, w);
}
__device__ __forceinline__ void w1_image_store_f32(unsigned char* img, int D, int h, int d, float w) {
    w1_image_store_half<false>(img, D, h, d, w);            // the bf16 bags' image: fp32 rows are split into bf16 terms too
}
// storage code (MOC_F32 / MOC_BF16 / MOC_F16) known at run time
__device__ __forceinline__ void w1_image_store(int dt, unsigned char* img, int D, int h, int d, float w) {
    if (dt == MOC_F16) w1_image_store_half<true>(img, D, h, d, w);
    else if (dt == MOC_BF16) w1_image_store_half<false>(img, D, h, d, w);
    else w1_image_store_f32(img, D, h, d, w);
}

// ------------------------------------------------------------------ which step kernel runs (moc_meta.hip)
// Decided ONCE per training call by step_plan, the only reader of the step kernels' shape limits; the launchers take the
// plan and the forward is told (emit_tiles) what it implies.  What depends on the slide stays per step.
enum StepKind { STEP_THREE = 0, STEP_NARROW, STEP_TILES, STEP_WIDE };   // three launches | pool_w1_step{,_tiles,_wide}_kernel
struct StepPlan {
    StepKind kind;
    bool pool_one;                               // pooling + loss in one kernel (pool_step_kernel): the three-launch step, evaluation
    int cap;                                     // PS_CAP: candidate list entries per class
    size_t smem;                                 // dynamic LDS of the one-launch kernel
    int pch, wide_region, wide_cap, external;    // wide: pairs per chunk, its LDS region, its list cap, pooling by topk_mean_kernel first
    bool one_launch() const { return kind != STEP_THREE; }
    bool tiles() const { return kind == STEP_TILES; }
    int mode() const { return kind == STEP_THREE ? 0 : kind == STEP_WIDE ? 2 : 1; }   // as GraphKey records it
};
// exchange: a P2pArgs will be passed to the step (never the tile-record kind); train = 0: pooling + loss only
StepPlan step_plan(const moc_batch_t* B, const moc_meta_ws_t* ws, bool exchange, int train = 1);

int step_attrs();   // raises the step kernels' dynamic-LDS limits, once per process: every entry, before its first launch

// ------------------------------------------------------------------ the step kernels' host side (moc_step_*.hip)
// Scalars exactly as torch hands them to its fp32 kernels: computed in Python doubles,
// rounded to fp32 once.
struct AdamCoef {
    float wd, one_minus_b1, beta2, one_minus_b2, eps;
    float neg_step_size;   // -(lr / (1 - beta1^t))
    float bc2_sqrt;        // sqrt(1 - beta2^t)
    float grad_scale;
};
// device-resident Adam coefficients for graph replay: the step's coefficients are tab[ctr[0] + pos]
struct StepTab { const AdamCoef* tab; const int32_t* ctr; int pos; };
AdamCoef adam_coef(const moc_meta_t* M, int64_t step, float grad_scale);   // the coefficients of Adam step `step` (moc_meta.hip)
// M advanced to run r: every tensor by r * par_stride, the W1 image by r * image_stride
inline moc_meta_t meta_of_run(const moc_meta_t* M, const moc_runs_t* R, int r) {
    moc_meta_t Mr = *M;
    const int64_t po = (int64_t)r * R->par_stride;
    Mr.W1 += po; Mr.b1 += po; Mr.W2 += po; Mr.b2 += po;
    Mr.m_W1 += po; Mr.m_b1 += po; Mr.m_W2 += po; Mr.m_b2 += po;
    Mr.v_W1 += po; Mr.v_b1 += po; Mr.v_W2 += po; Mr.v_b2 += po;
    Mr.W1_image = (unsigned char*)M->W1_image + (int64_t)r * R->image_stride;
    return Mr;
}
// Each source raises the dynamic-LDS limit of its own kernels (hipFuncSetAttribute must name the kernel); step_attrs calls
// the three, in this order, and reports the first failure.
typedef void (*raise_lds_fn)(const char* name, const void* kernel, int bytes);
void pool_step_attrs(raise_lds_fn raise);
void fused_step_attrs(raise_lds_fn raise);
void tile_step_attrs(raise_lds_fn raise);
// ---- moc_step_pool.hip: the three-launch step
int launch_pool(const moc_batch_t* B, const moc_meta_ws_t* ws, int slide0, int n, hipStream_t s);   // topk_mean_kernel over the mixed scores
// pooling + loss (+ pair gradients and the small-parameter step) for slides [slide0, slide0+n)
int launch_pool_finish(const StepPlan& p, const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws, const int64_t* labels,
                       int slide0, int n, int train, int apply_adam, uint32_t use_bits, const AdamCoef& k, hipStream_t s);
int launch_w1(const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws, int apply_adam, const AdamCoef& k, hipStream_t s,
              bool padded_pairs);
// plain Adam over all four tensors from the gradients in M->g_* (+ the W1 image when `img` is given)
int launch_adam_all(const moc_meta_t* M, const AdamCoef& k, unsigned char* img, int img_dt, hipStream_t s, const char* who);
// ---- moc_step_fused.hip: the narrow and the wide one-launch step (x: the gradient exchange, or null)
int launch_fused_kernel(const StepPlan& p, const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws, const int64_t* labels,
                        int slide, uint32_t use_bits, const AdamCoef& k, float* W2out, hipStream_t s, int apply_adam,
                        const P2pArgs* x, const StepTab* tab);
// ---- moc_step_tiles.hip: the one-launch step over the forward's tile records.  One meta-learner (S_host: the slide's
// selected-row count as the forward of this step was given it, host_n_sel; -1: the device's n_sel) ...
int launch_tile_step(const StepPlan& p, const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws, const int64_t* labels,
                     int slide, uint32_t use_bits, const AdamCoef& k, float* W2out, hipStream_t s, int apply_adam,
                     const StepTab* tab, int next_slide, int S_host);
// ... or runs [r0, r0 + nr) of R in one launch (nr <= MOC_MAX_RUNS; per-run coefficients: nr <= MOC_HP_RUNS), each on its
// slide `slide` + run * slide_stride.  cur / nxt: the W2 buffers of run 0 this step reads / writes, a run's 4 H floats
// cur_stride / nxt_stride apart.  k: ONE AdamCoef for all runs, or (k_per_run) run r0 + r's at k[r].
int launch_tile_runs(const StepPlan& p, const moc_batch_t* B, const moc_meta_t* M, const moc_runs_t* R, const moc_meta_ws_t* ws,
                     const int64_t* labels, int slide, bool more_steps, uint32_t use_bits, int r0, int nr, const AdamCoef* k,
                     bool k_per_run, float* cur, int64_t cur_stride, float* nxt, int64_t nxt_stride, hipStream_t s);

// ------------------------------------------------------------------ the forward's host side, as the step calls it
// (moc_meta_forward.hip)
// the argument checks every entry over a meta-learner and its work arrays starts with
int check_meta(const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws, const char* who, bool need_adam,
               bool need_grad, bool need_h1 = true);
// rewrites the W1 image(s) from the parameters; R: one image per run (grid.y = run), NULL: M's one
int launch_w1_images(const moc_batch_t* B, const moc_meta_t* M, const moc_runs_t* R, hipStream_t s);
// the most selected rows a slide of the batch can have
int s_bound(const moc_batch_t* B);
// Slide b's selected-row count S as the HOST knows it, or -1: n_sel_host[b] when the caller has seen a copy arrive, else
// the slide's word of the pinned mailbox compact_kernel writes (moc_batch_t.n_sel_mail) when it carries the expected
// ticket -- one acquire load, never a wait.  A train step asks ONCE, in front of its two launches, and hands both the
// answer by value: forward and step agree on it, and nothing reads the mailbox after the launch.
inline int host_n_sel(const moc_batch_t* B, int b) {
    if (B->n_sel_host) return B->n_sel_host[b];
    if (!B->n_sel_mail || B->n_sel_ticket == 0) return -1;
    const uint64_t w = __atomic_load_n(B->n_sel_mail + b, __ATOMIC_ACQUIRE);
    return (uint32_t)(w >> 32) == B->n_sel_ticket ? (int)(uint32_t)w : -1;
}
// The forward of slides [slide0, slide0 + n) into ws.  emit_tiles (StepPlan::tiles()): the one-launch step over tile records
// follows (training step of one slide): leave the records.  runs != nullptr: the training forward of runs->n_runs meta-learners in one launch
// (moc_train_steps_runs), `M->W2` / `w2_stride` = where their current W2 lives.  S_host (one slide, one run): the slide's
// selected-row count by host_n_sel, -1: not known; the runs read n_sel_host themselves.
int launch_forward(const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws, int slide0, int n, uint32_t use_bits,
                   hipStream_t s, bool emit_tiles = false, const moc_runs_t* runs = nullptr, int64_t w2_stride = 0, int S_host = -1);

}  // namespace moc_meta_internal
