// Phase B, the step: the training entries, and which step kernel a shape gets.  A meta-step is the meta-learner's forward
// (moc_meta_forward.hip: the "senet" over the selected rows, the gated mix) and then top-K mean pooling, cross entropy,
// the analytically sparse backward and Adam over what it has left.
//
// Reference semantics:
//   pooling .............. utils/patch_selection_classifier.py:18-32
//   loss / backward ...... main_moc.py:406-409 (F.cross_entropy, loss.backward())
//   Adam ................. main_moc.py:316, :410 (lr 1e-3, weight_decay 1e-4 coupled, torch defaults)
//
// Only the <= K*C rows that reach the top-K of some class carry gradient, so the
// backward never touches the other S-K*C rows: d mixed[s,c] = dpooled[c]/k for
// those (s,c) "pairs", then the usual chain through sigmoid, Linear, ReLU, Linear.
//
// Per meta-step TWO launches on one stream, no host synchronisation: the forward (16-row tiles, MFMA), then ONE kernel
// for pooling, loss, backward and the whole Adam step, W2 ping-ponged between two buffers.  step_plan picks that kernel
// once per call:
//   tiles ..... pool_w1_step_tiles_kernel (moc_step_tiles.hip): over the forward's tile records; C * topk <= 64 -- the
//               benchmark's default shape, and the lockstep runs of moc_train_steps_runs{,_hp}
//   narrow .... pool_w1_step_kernel (moc_step_fused.hip): the same shapes without records, or with a gradient exchange
//   wide ...... pool_w1_step_wide_kernel (moc_step_fused.hip): C <= 64, D in {512, 1024} (EBRAINS-30)
//   three ..... anything else, and callers without ws->W2_alt: pooling + loss (+ small parameters), then the W1 update
//               (moc_step_pool.hip, which also holds the loss-only entries)
// This file: the plan, the kernels' LDS limits, the training entries over those launchers, the step-graph handle.
// What the step sources share: moc_step_shared.h; what crosses between them: moc_meta_internal.h.
#include <atomic>
#include <chrono>
#include <cstring>
#include <new>
#include "moc_step_shared.h"

constexpr int FS_MAX_XS = 20480; // narrow one-launch step: pair rows staged in LDS, C*K*D <= this many floats (80 KiB)

AdamCoef moc_meta_internal::adam_coef(const moc_meta_t* M, int64_t step, float grad_scale) {
    AdamCoef k;
    k.wd = (float)M->weight_decay;
    k.one_minus_b1 = (float)(1.0 - M->beta1);
    k.beta2 = (float)M->beta2;
    k.one_minus_b2 = (float)(1.0 - M->beta2);
    k.eps = (float)M->eps;
    const double bc1 = 1.0 - pow(M->beta1, (double)step);
    const double bc2 = 1.0 - pow(M->beta2, (double)step);
    k.neg_step_size = (float)(-(M->lr / bc1));
    k.bc2_sqrt = (float)sqrt(bc2);
    k.grad_scale = grad_scale;
    return k;
}

// The ONE place that says which step kernel a shape gets, and why.
StepPlan moc_meta_internal::step_plan(const moc_batch_t* B, const moc_meta_ws_t* ws, bool exchange, int train) {
    static const bool tiles_off = getenv("MOC_TILE_RECORDS") && atoi(getenv("MOC_TILE_RECORDS")) == 0;   // diagnostic: the round-3 step
    StepPlan p = {};
    const int sb = s_bound(B);
    p.cap = lds::step_cap(B->C);
    p.pool_one = B->topk <= 16 && B->C <= 16 && sb <= 64 * 16 * PS_VPT && (!train || B->C * B->topk <= 64);
    if (!train || !ws->W2_alt) return p;                    // the one-launch steps ping-pong W2
    // narrow (pool_w1_step_kernel): pool_step_kernel's shapes, when the pairs' rows fit in LDS
    // (a layout is asked only behind its kernel's shape limits: its offsets are 32-bit)
    const bool rows_fit = p.pool_one && B->D <= 1024 && (int64_t)B->C * B->topk * B->D <= FS_MAX_XS;
    if (rows_fit && lds::narrow_step_lds(B->C, B->topk, B->D, p.cap).bytes <= lds::NARROW_MAX_LDS) {
        p.kind = STEP_NARROW; p.smem = lds::narrow_step_lds(B->C, B->topk, B->D, p.cap).bytes;
        const int tiles = lds::tile_step_lds(B->C, B->topk, p.cap).bytes;
        // over the forward's tile records (pool_w1_step_tiles_kernel): the caller has given the record arrays, a class's
        // records are at most sixteen keys per lane; its workgroups exchange nothing
        const bool records = ws->tile_ws && B->row_off_host &&
                             ws->tile_ws_bytes >= (int64_t)tile_bytes(tile_slots(B->total_rows, B->n_slides, B->C));
        if (!exchange && !tiles_off && records && moc_cdiv(sb, 16) * TILE_R <= 16 * 64 && tiles <= lds::TILE_MAX_LDS) {
            p.kind = STEP_TILES; p.smem = tiles;
        }
        return p;
    }
    // wide (pool_w1_step_wide_kernel): C <= 64, K <= 16, D/16 = 32 or 64 columns per workgroup, every pair's piece in LDS
    if (B->topk <= 16 && B->C <= 64 && B->D % 512 == 0 && B->D <= 1024 && wide_lds(B, WD_PCH_MIN).bytes <= lds::WIDE_MAX_LDS) {
        p.kind = STEP_WIDE; p.pch = lds::wide_pch(B->C, B->topk, B->D, (int)moc_elem_size(B->dtype)); p.wide_cap = lds::wide_cap(B->C);
        p.wide_region = wide_lds(B, p.pch).region_bytes; p.smem = wide_lds(B, p.pch).bytes;
        // pooling inside the kernel: every one of the 16 workgroups ranks all C classes for itself -- fine for a few
        // ten thousand scores, not for EBRAINS-30's 30 x 7,500 (measured: 88 us against 11.4 + 28 with one workgroup per
        // class in topk_mean_kernel first); beyond 8,192 rows it does not fit the registers at all
        p.external = sb > 8192 || (int64_t)B->C * sb > 49152;
    }
    return p;
}

// Raises the dynamic-LDS limit of every step kernel that needs it: once per process (the batched runs call the training
// entries from pool threads) and outside any stream capture -- every entry calls it before its first launch.
int moc_meta_internal::step_attrs() {
    static std::once_flag once;
    static char failed[96] = "";                              // the first kernel whose limit could not be raised, and to what
    std::call_once(once, [] {
        const raise_lds_fn raise = [](const char* name, const void* f, int bytes) {
            if (!failed[0] && hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess)
                snprintf(failed, sizeof(failed), "%s to %d bytes", name, bytes);
        };
        pool_step_attrs(raise);
        fused_step_attrs(raise);
        tile_step_attrs(raise);
    });
    if (failed[0]) MOC_FAIL(MOC_ELAUNCH, "moc_fused_step: cannot raise the dynamic LDS limit of %s", failed);
    return MOC_OK;
}

namespace {

// The one-launch step of plan p.  next_slide: the slide the step after this one works on, in the same work arrays (-1: none /
// unknown) -- the tile-record step prefetches its rows.  x: the gradient exchange, which the tile-record kernel has not got.
// S_host: the slide's selected-row count as this step's forward was given it (host_n_sel; -1: not asked / not known).
int launch_fused_step(const StepPlan& p, const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws, const int64_t* labels,
                      int slide, uint32_t use_bits, const AdamCoef& k, float* W2out, hipStream_t s,
                      int apply_adam = 1, const P2pArgs* x = nullptr, const StepTab* tab = nullptr, int next_slide = -1,
                      int S_host = -1) {
    MOC_REQUIRE(p.one_launch() && !(p.tiles() && x), "moc_fused_step: plan of kind %d%s", (int)p.kind, x ? " with a gradient exchange" : "");
    if (p.tiles())                                         // over the forward's tile records (the forward was told to leave them)
        return launch_tile_step(p, B, M, ws, labels, slide, use_bits, k, W2out, s, apply_adam, tab, next_slide, S_host);
    return launch_fused_kernel(p, B, M, ws, labels, slide, use_bits, k, W2out, s, apply_adam, x, tab);
}

// moc_n_sel_stats: the steps moc_train_steps has issued, and those among them whose S the host knew (process-wide)
std::atomic<int64_t> g_steps_issued{0}, g_steps_known{0};

// Asked ONCE per step, in front of its two launches: slide b's selected-row count for both (host_n_sel), counted.
int step_n_sel(const moc_batch_t* B, int b) {
    const int S = host_n_sel(B, b);
    g_steps_issued.fetch_add(1, std::memory_order_relaxed);
    if (S >= 0) g_steps_known.fetch_add(1, std::memory_order_relaxed);
    return S;
}

// A BOUNDED wait in front of a pass's first step (MOC_N_SEL_SPIN_US microseconds at the most; 0: none): the look-ahead phase A
// of a pass is launched right before the host turns to that pass's steps, and compact_kernel -- its last launch -- stores
// all slides' words within a few microseconds of each other, so the steps the host issues before that moment run on the
// bound and the ones behind it on their count.  The GPU still has the previous pass's steps in its queue meanwhile.
// Measured (profiles/NOTES.md): without the wait 38-70 % of the benchmark's steps know their S, with 100 us 88-99 %, with
// 250 us all of them; `value` is highest at 100.  A word that never comes (no phase A under this ticket) costs the bound
// once per call.
void await_first_word(const moc_batch_t* B, int b) {
    static const int spin_us = getenv("MOC_N_SEL_SPIN_US") ? atoi(getenv("MOC_N_SEL_SPIN_US")) : 100;
    if (spin_us <= 0 || B->n_sel_host || !B->n_sel_mail || B->n_sel_ticket == 0 || host_n_sel(B, b) >= 0) return;
    const auto until = std::chrono::steady_clock::now() + std::chrono::microseconds(spin_us);
    while (host_n_sel(B, b) < 0 && std::chrono::steady_clock::now() < until) {}
}

}  // namespace

extern "C" int moc_n_sel_stats(int64_t* known, int64_t* steps, int reset) {
    const int64_t k = reset ? g_steps_known.exchange(0) : g_steps_known.load();
    const int64_t n = reset ? g_steps_issued.exchange(0) : g_steps_issued.load();
    if (known) *known = k;
    if (steps) *steps = n;
    return MOC_OK;
}

extern "C" int moc_train_grad(const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws,
                              const int64_t* labels, int slide, uint32_t use_bits, moc_stream_t stream) {
    if (int rc = moc_check_batch(B, "moc_train_grad")) return rc;
    if (int rc = check_meta(B, M, ws, "moc_train_grad", false, true)) return rc;
    MOC_REQUIRE(labels && slide >= 0 && slide < B->n_slides, "moc_train_grad: bad labels/slide");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = step_attrs()) return rc;
    const StepPlan p = step_plan(B, ws, false);
    AdamCoef k = {};
    k.grad_scale = 1.f;
    // forward (fresh W1 image: the parameters may have been stepped by moc_adam_step), pooling +
    // loss + pair gradients, W1 gradient -- everything one meta-step does short of the update
    if (int rc = launch_w1_images(B, M, nullptr, s)) return rc;
    if (int rc = launch_forward(B, M, ws, slide, 1, use_bits, s, p.tiles())) return rc;
    if (p.one_launch()) return launch_fused_step(p, B, M, ws, labels, slide, use_bits, k, nullptr, s, 0);
    if (int rc = launch_pool_finish(p, B, M, ws, labels, slide, 1, 1, 0, use_bits, k, s)) return rc;
    return launch_w1(B, M, ws, 0, k, s, p.pool_one);
}

extern "C" int moc_train_steps_dp(const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws,
                                  const int64_t* labels, int slide0, int n, uint32_t use_bits,
                                  float* grad_flat, int64_t grad_count, moc_allreduce_fn allreduce,
                                  void* comm, int world, moc_stream_t stream) {
    if (int rc = moc_check_batch(B, "moc_train_steps_dp")) return rc;
    if (int rc = check_meta(B, M, ws, "moc_train_steps_dp", true, true)) return rc;
    MOC_REQUIRE(labels && slide0 >= 0 && n >= 1 && slide0 + n <= B->n_slides, "moc_train_steps_dp: bad labels/slide range");
    const int64_t n_par = n_params(M->D);
    MOC_REQUIRE(world >= 1 && (world == 1 || allreduce), "moc_train_steps_dp: world %d needs an all-reduce", world);
    MOC_REQUIRE(!allreduce || (grad_flat && grad_count >= n_par && M->g_W1 >= grad_flat &&
                               M->g_W1 + (int64_t)H * M->D <= grad_flat + grad_count),
                "moc_train_steps_dp: the gradient tensors must live in grad_flat[%lld]", (long long)grad_count);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = step_attrs()) return rc;
    const StepPlan p = step_plan(B, ws, false);
    if (int rc = launch_w1_images(B, M, nullptr, s)) return rc;      // afterwards the Adam kernel keeps it in sync
    const int img_dt = B->dtype;
    AdamCoef kg = {};
    kg.grad_scale = 1.f;
    for (int t = 0; t < n; ++t) {
        const int b = slide0 + t;
        if (int rc = launch_forward(B, M, ws, b, 1, use_bits, s, p.tiles())) return rc;
        if (p.one_launch()) {
            if (int rc = launch_fused_step(p, B, M, ws, labels, b, use_bits, kg, nullptr, s, 0)) return rc;
        } else {
            if (int rc = launch_pool_finish(p, B, M, ws, labels, b, 1, 1, 0, use_bits, kg, s)) return rc;
            if (int rc = launch_w1(B, M, ws, 0, kg, s, p.pool_one)) return rc;
        }
        if (allreduce) {   // the ONE collective of a step: sum of the flat gradient over the ranks
            const int rc = allreduce(grad_flat, grad_flat, (size_t)grad_count, 7 /* ncclFloat32 */, 0 /* ncclSum */, comm, stream);
            if (rc != 0) MOC_FAIL(MOC_ELAUNCH, "moc_train_steps_dp: all-reduce failed at step %d (rc=%d)", t, rc);
        }
        const AdamCoef k = adam_coef(M, M->step + 1 + t, 1.f / (float)world);
        if (int rc = launch_adam_all(M, k, (unsigned char*)M->W1_image, img_dt, s, "moc_train_steps_dp")) return rc;
    }
    return MOC_OK;
}

extern "C" int moc_p2p_step_supported(int C, int topk, int D, int topj) {
    // from the run's constants only (not the bag sizes): every rank must take the same path
    moc_batch_t B = {};
    B.C = C; B.topk = topk; B.D = D; B.topj = topj; B.max_rows = 0x7fffffff;
    moc_meta_ws_t ws = {};
    float dummy;
    ws.W2_alt = &dummy;
    return C >= 1 && topk >= 1 && D >= 1 && topj >= 1 && step_plan(&B, &ws, true).one_launch() ? 1 : 0;
}

extern "C" int moc_train_steps_p2p(const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws,
                                   const int64_t* labels, int slide0, int n, uint32_t use_bits,
                                   moc_p2p_t* comm, moc_stream_t stream) {
    if (int rc = moc_check_batch(B, "moc_train_steps_p2p")) return rc;
    if (int rc = check_meta(B, M, ws, "moc_train_steps_p2p", true, false)) return rc;
    MOC_REQUIRE(labels && slide0 >= 0 && n >= 1 && slide0 + n <= B->n_slides, "moc_train_steps_p2p: bad labels/slide range");
    MOC_REQUIRE(comm, "moc_train_steps_p2p: null communicator");
    // Which step kernel runs is decided from the run's constants alone (as moc_p2p_step_supported does), never from
    // this rank's bag sizes: the narrow and the wide kernel assign W1 elements to workgroups differently, and the
    // per-workgroup arrival flags of the exchange only mean something when every rank runs the same one.  (An exchange
    // plan is never the tile-record kind, at any world size: the forward below leaves no records.)
    moc_batch_t Bu = *B;
    Bu.max_rows = 0x7fffffff;
    const StepPlan p = step_plan(&Bu, ws, true);
    MOC_REQUIRE(p.one_launch(), "moc_train_steps_p2p: shape outside the one-launch steps (K <= 16, C <= 64, "
                "D in {512, 1024} beyond C = 16); use moc_train_steps_dp");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = step_attrs()) return rc;
    if (int rc = launch_w1_images(B, M, nullptr, s)) return rc;
    moc_meta_t Mt = *M;
    float* cur = M->W2;
    float* nxt = ws->W2_alt;
    for (int t = 0; t < n; ++t) {
        const int b = slide0 + t;
        P2pArgs x;
        if (int rc = moc_p2p_next_args(comm, &x)) return rc;
        MOC_REQUIRE(x.n_par == n_params(M->D), "moc_train_steps_p2p: communicator made for %lld parameters",
                    (long long)x.n_par);
        const AdamCoef k = adam_coef(M, M->step + 1 + t, 1.f / (float)x.world);
        Mt.W2 = cur;
        if (int rc = launch_forward(B, &Mt, ws, b, 1, use_bits, s)) return rc;
        if (int rc = launch_fused_step(p, &Bu, &Mt, ws, labels, b, use_bits, k, nxt, s, 1, &x)) return rc;
        float* tmp = cur; cur = nxt; nxt = tmp;
    }
    if (cur != M->W2) {
        if (hipMemcpyAsync(M->W2, cur, sizeof(float) * 4 * H, hipMemcpyDeviceToDevice, s) != hipSuccess)
            MOC_FAIL(MOC_ELAUNCH, "moc_train_steps_p2p: copy-back of W2 failed");
    }
    return MOC_OK;
}

struct moc_step_graph;
namespace {
int issue_fused_pass(const StepPlan& p, const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws, const int64_t* labels,
                     int slide0, int n, uint32_t use_bits, hipStream_t s, const moc_step_graph* G);
}

extern "C" int moc_train_steps(const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws,
                               const int64_t* labels, int slide0, int n, uint32_t use_bits,
                               moc_stream_t stream) {
    if (int rc = moc_check_batch(B, "moc_train_steps")) return rc;
    if (int rc = check_meta(B, M, ws, "moc_train_steps", true, false)) return rc;
    MOC_REQUIRE(labels && slide0 >= 0 && n >= 1 && slide0 + n <= B->n_slides, "moc_train_steps: bad labels/slide range");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = step_attrs()) return rc;
    const StepPlan p = step_plan(B, ws, false);
    await_first_word(B, slide0);
    if (p.one_launch()) return issue_fused_pass(p, B, M, ws, labels, slide0, n, use_bits, s, nullptr);
    if (int rc = launch_w1_images(B, M, nullptr, s)) return rc;      // afterwards the W1 update keeps it in sync
    for (int t = 0; t < n; ++t) {
        const int b = slide0 + t;
        const AdamCoef k = adam_coef(M, M->step + 1 + t, 1.f);
        if (int rc = launch_forward(B, M, ws, b, 1, use_bits, s, false, nullptr, 0, step_n_sel(B, b))) return rc;
        if (int rc = launch_pool_finish(p, B, M, ws, labels, b, 1, 1, 1, use_bits, k, s)) return rc;
        if (int rc = launch_w1(B, M, ws, 1, k, s, p.pool_one)) return rc;
    }
    return MOC_OK;
}

// ------------------------------------------------------------------ batched runs: R meta-learners, lockstep
// The reference's real workload is folds x shots of the SAME loop as independent processes (scripts/moc_train.sh:11-31), and
// one run is a chain of dependent 17-us steps that leaves most of the GPU idle.  Here ONE forward launch and ONE step
// launch serve R runs: grid.y / grid.z = run.  Every run stays the exact recurrence of moc_train_steps -- its own slides,
// parameters, Adam moments; the same kernels, the same operation order: bit-identical to running it alone.
extern "C" int moc_train_runs_mode(const moc_batch_t* B, const moc_meta_ws_t* ws) {
    if (!B || !ws) return 0;
    const StepPlan p = step_plan(B, ws, false);
    return p.tiles() ? 1 : p.one_launch() ? 2 : 0;
}

// `hp` == nullptr: the runs share M's hyper-parameters (moc_train_steps_runs: one AdamCoef per launch, the argument block
// and the kernel it has always had); else run r steps with hp[r] (moc_train_steps_runs_hp)
static int train_steps_runs(const moc_batch_t* B, const moc_meta_t* M, const moc_runs_t* R, const moc_meta_ws_t* ws,
                            const int64_t* labels, int slide0, int n, uint32_t use_bits, const moc_adam_hp_t* hp,
                            moc_stream_t stream, const char* who) {
    if (int rc = moc_check_batch(B, who)) return rc;
    if (int rc = check_meta(B, M, ws, who, true, false)) return rc;
    MOC_REQUIRE(R && R->n_runs >= 1 && R->n_runs <= MOC_MAX_RUNS, "%s: 1 .. %d runs", who, MOC_MAX_RUNS);
    MOC_REQUIRE(labels && slide0 >= 0 && n >= 1 && R->slide_stride >= n &&
                slide0 + n + (R->n_runs - 1) * R->slide_stride <= B->n_slides, "%s: bad labels/slide range", who);
    MOC_REQUIRE(R->par_stride >= n_params(B->D) && R->image_stride >= (int64_t)moc_w1_image_bytes(B->D, B->dtype),
                "%s: parameter / image stride smaller than one meta-learner", who);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = step_attrs()) return rc;
    const StepPlan p = step_plan(B, ws, false);
    // run r's hyper-parameters as a moc_meta_t that adam_coef reads: M's, or record r
    auto with_hp = [&](moc_meta_t& Mr, int r) {
        if (!hp) return;
        Mr.lr = hp[r].lr; Mr.beta1 = hp[r].beta1; Mr.beta2 = hp[r].beta2; Mr.eps = hp[r].eps; Mr.weight_decay = hp[r].weight_decay;
    };
    if (!p.tiles()) {
        // Shapes outside the tile-record step (wide banks: EBRAINS-30, the 64-way shape; C > 16, C K > 64, more than 4,096
        // selectable rows): every run's pass through moc_train_steps' own launches, one run after the other on this stream --
        // the same kernels on the same tensors as the run alone, so the same bits.  What the caller still gains is phase A
        // over all runs' slides in one pass and (moc_amd.runs: one group per run) the runs' chains side by side on streams
        // of their own, each of which keeps a few dozen CUs busy.  The one-launch steps only (W2_alt set): the three-launch
        // step's scratch is one per batch.
        MOC_REQUIRE(p.one_launch(), "%s: this shape needs ws->W2_alt (the one-launch steps)", who);
        for (int r = 0; r < R->n_runs; ++r) {
            moc_meta_t Mr = meta_of_run(M, R, r);
            with_hp(Mr, r);
            Mr.g_W1 = Mr.g_b1 = Mr.g_W2 = Mr.g_b2 = nullptr;
            moc_meta_ws_t wr = *ws;
            wr.W2_alt = ws->W2_alt + (int64_t)r * 4 * H;    // (another address, the same plan)
            if (int rc = issue_fused_pass(p, B, &Mr, &wr, labels, slide0 + r * R->slide_stride, n, use_bits, s, nullptr)) return rc;
        }
        return MOC_OK;
    }
    if (int rc = launch_w1_images(B, M, R, s)) return rc;
    moc_meta_t Mt = *M;
    float* cur = M->W2;
    float* nxt = ws->W2_alt;
    int64_t cur_stride = R->par_stride, nxt_stride = 4 * H;
    // more runs than one launch with per-run coefficients carries: even pieces (nine runs: 5 + 4)
    const int hp_pieces = moc_cdiv(R->n_runs, MOC_HP_RUNS), hp_per = moc_cdiv(R->n_runs, hp_pieces);
    for (int t = 0; t < n; ++t) {
        const int b = slide0 + t;
        Mt.W2 = cur;
        if (int rc = launch_forward(B, &Mt, ws, b, 1, use_bits, s, p.tiles(), R, cur_stride)) return rc;
        if (!hp) {
            const AdamCoef k = adam_coef(M, M->step + 1 + t, 1.f);
            if (int rc = launch_tile_runs(p, B, M, R, ws, labels, b, t + 1 < n, use_bits, 0, R->n_runs, &k, false, cur, cur_stride,
                                          nxt, nxt_stride, s)) return rc;
        } else {
            for (int r0 = 0; r0 < R->n_runs; r0 += hp_per) {
                const int nr = R->n_runs - r0 < hp_per ? R->n_runs - r0 : hp_per;
                AdamCoef k[MOC_HP_RUNS];
                for (int r = 0; r < nr; ++r) {
                    // (the arithmetic of adam_coef on record r0 + r: the floats the run alone gets)
                    moc_meta_t Mr = *M;
                    with_hp(Mr, r0 + r);
                    k[r] = adam_coef(&Mr, M->step + 1 + t, 1.f);
                }
                if (int rc = launch_tile_runs(p, B, M, R, ws, labels, b, t + 1 < n, use_bits, r0, nr, k, true, cur, cur_stride,
                                              nxt, nxt_stride, s)) return rc;
            }
        }
        float* tmp = cur; cur = nxt; nxt = tmp;
        const int64_t ts = cur_stride; cur_stride = nxt_stride; nxt_stride = ts;
    }
    if (cur != M->W2) {   // odd number of steps: every run's current W2 lives in the scratch buffer
        if (hipMemcpy2DAsync(M->W2, sizeof(float) * (size_t)R->par_stride, cur, sizeof(float) * 4 * H, sizeof(float) * 4 * H,
                             (size_t)R->n_runs, hipMemcpyDeviceToDevice, s) != hipSuccess)
            MOC_FAIL(MOC_ELAUNCH, "%s: copy-back of W2 failed", who);
    }
    return MOC_OK;
}

extern "C" int moc_train_steps_runs(const moc_batch_t* B, const moc_meta_t* M, const moc_runs_t* R, const moc_meta_ws_t* ws,
                                    const int64_t* labels, int slide0, int n, uint32_t use_bits, moc_stream_t stream) {
    return train_steps_runs(B, M, R, ws, labels, slide0, n, use_bits, nullptr, stream, "moc_train_steps_runs");
}

extern "C" int moc_train_steps_runs_hp(const moc_batch_t* B, const moc_meta_t* M, const moc_runs_t* R, const moc_meta_ws_t* ws,
                                       const int64_t* labels, int slide0, int n, uint32_t use_bits, const moc_adam_hp_t* hp,
                                       moc_stream_t stream) {
    const char* who = "moc_train_steps_runs_hp";
    MOC_REQUIRE(hp, "%s: null hyper-parameter records", who);
    MOC_REQUIRE(R && R->n_runs >= 1 && R->n_runs <= MOC_MAX_RUNS, "%s: 1 .. %d runs", who, MOC_MAX_RUNS);
    for (int r = 0; r < R->n_runs; ++r) {
        const moc_adam_hp_t& h = hp[r];
        // (written so that a NaN fails: every comparison with one is false)
        MOC_REQUIRE(h.lr >= 0.0 && h.lr <= 1.7976931348623157e308, "%s: run %d: lr = %g (finite, >= 0)", who, r, h.lr);
        MOC_REQUIRE(h.eps >= 0.0 && h.eps <= 1.7976931348623157e308, "%s: run %d: eps = %g (finite, >= 0)", who, r, h.eps);
        MOC_REQUIRE(h.weight_decay >= 0.0 && h.weight_decay <= 1.7976931348623157e308,
                    "%s: run %d: weight_decay = %g (finite, >= 0)", who, r, h.weight_decay);
        MOC_REQUIRE(h.beta1 >= 0.0 && h.beta1 < 1.0, "%s: run %d: beta1 = %g (0 <= beta < 1)", who, r, h.beta1);
        MOC_REQUIRE(h.beta2 >= 0.0 && h.beta2 < 1.0, "%s: run %d: beta2 = %g (0 <= beta < 1)", who, r, h.beta2);
    }
    return train_steps_runs(B, M, R, ws, labels, slide0, n, use_bits, hp, stream, who);
}

// ------------------------------------------------------------------ a pass of meta-steps as ONE graph launch
// moc_train_steps issues 2 n + 1 launches per pass (0.2 ms of host time for 32 steps).  In a long run they are
// issued ahead of the GPU and cost nothing; at the START of a run, or of a short timed region, the queue is empty and
// the chain cannot begin before the host has got through its prelude.  The handle below keeps the pass as an
// instantiated hipGraph per (work arrays, meta-learner tensors, slide range): a replay is one hipGraphLaunch.
// What changes from replay to replay -- the Adam step count, i.e. the bias corrections -- is not a kernel argument
// there: the coefficients of steps tab_base + 1 ... tab_base + cap sit in a device table (computed by the host with
// the arithmetic of adam_coef, so the same floats as the eager path) and a device counter holds how many of them have
// been used; the kernel at position t of the pass reads entry ctr + t, the graph's last node advances ctr by n.
struct moc_step_graph {
    int32_t* ctr;            // device: steps taken since tab_base (caller's workspace, first 16 bytes)
    AdamCoef* tab;           // device [cap]: entry i = coefficients of step tab_base + i + 1
    int cap;
    // host mirror
    bool tab_valid;
    double lr, beta1, beta2, eps, wd;
    int64_t tab_base;
    int64_t dev_rel;         // the counter's value once everything issued so far has run (-1: unknown)
    AdamCoef* stage;         // pinned staging of the table upload
    hipEvent_t stage_done;   // the upload that read `stage` has run
    bool stage_busy;
    hipStream_t cap_stream;  // passes are captured here (nothing ever runs on it): the caller's stream may be the
                             // legacy default stream, which cannot be captured
    struct Entry {
        unsigned char key[512];
        hipGraph_t graph;
        hipGraphExec_t exec;
        uint64_t used;
    } e[8];
    int n_entries;
    uint64_t tick;
    int eager_only;          // capture or instantiation failed once: the handle stays on stream launches
    int captures, replays, eager_calls;
    // the counter and the table are shared by every call: a call on ANOTHER stream than the previous one waits for it
    hipStream_t last_stream;
    hipEvent_t last_done;
    bool has_last;
};

namespace {

__global__ void step_ctr_set_kernel(int32_t* ctr, int32_t v) { ctr[0] = v; }
__global__ void step_ctr_add_kernel(int32_t* ctr, int32_t n) { ctr[0] += n; }

struct GraphKey {            // everything a captured pass bakes into its kernel arguments
    const void *X, *row_off, *sel_row, *n_sel, *cand, *labels;
    const void *W1, *b1, *W2, *b2, *mW1, *mb1, *mW2, *mb2, *vW1, *vb1, *vW2, *vb2, *img;
    const void *H1, *gates, *mixed, *pooled, *topk_idx, *topk_cnt, *loss, *pred, *pair_dh, *W2_alt, *pair_row, *n_pair, *tile_ws;
    int64_t total_rows, tile_ws_bytes;
    uint64_t off_hash;       // FNV-1a of row_off_host[slide0 .. slide0 + n]
    int32_t dtype, D, n_slides, C, Ce, topj, topk, s_bound, mode, external, slide0, n;
    uint32_t use_bits, flags;  // flags: MOC_FORWARD_ROWS64 / MOC_FORWARD_FOUR_WAVES pick the forward kernel a capture bakes in
};
static_assert(sizeof(GraphKey) <= 512, "GraphKey outgrew moc_step_graph::Entry::key");

void graph_key(GraphKey* k, const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws, const int64_t* labels,
               int slide0, int n, uint32_t use_bits, const StepPlan& p) {
    memset(k, 0, sizeof(*k));
    k->X = B->X; k->row_off = B->row_off; k->sel_row = B->sel_row; k->n_sel = B->n_sel; k->cand = B->cand; k->labels = labels;
    k->W1 = M->W1; k->b1 = M->b1; k->W2 = M->W2; k->b2 = M->b2; k->mW1 = M->m_W1; k->mb1 = M->m_b1; k->mW2 = M->m_W2;
    k->mb2 = M->m_b2; k->vW1 = M->v_W1; k->vb1 = M->v_b1; k->vW2 = M->v_W2; k->vb2 = M->v_b2; k->img = M->W1_image;
    k->H1 = ws->H1; k->gates = ws->gates; k->mixed = ws->mixed; k->pooled = ws->pooled; k->topk_idx = ws->topk_idx;
    k->topk_cnt = ws->topk_cnt; k->loss = ws->loss; k->pred = ws->pred; k->pair_dh = ws->pair_dh; k->W2_alt = ws->W2_alt;
    k->pair_row = ws->pair_row; k->n_pair = ws->n_pair; k->tile_ws = ws->tile_ws; k->tile_ws_bytes = ws->tile_ws_bytes;
    k->total_rows = B->total_rows;
    uint64_t h = 1469598103934665603ull;
    if (B->row_off_host)
        for (int i = slide0; i <= slide0 + n; ++i) { h ^= (uint64_t)B->row_off_host[i]; h *= 1099511628211ull; }
    k->off_hash = B->row_off_host ? h : 0;
    k->dtype = B->dtype; k->D = B->D; k->n_slides = B->n_slides; k->C = B->C; k->topk = B->topk; k->s_bound = s_bound(B);
    k->mode = p.mode(); k->external = p.external;
    k->slide0 = slide0; k->n = n; k->use_bits = use_bits;
    k->Ce = B->Ce; k->topj = B->topj; k->flags = B->flags;
}

// the 2 n + 1 launches of a fused-step pass; `tab` != null: coefficients from the device table (capture)
int issue_fused_pass(const StepPlan& p, const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws, const int64_t* labels,
                     int slide0, int n, uint32_t use_bits, hipStream_t s, const moc_step_graph* G) {
    if (int rc = launch_w1_images(B, M, nullptr, s)) return rc;      // afterwards the W1 update keeps it in sync
    // two launches per meta-step: forward, then pooling + loss + backward + the whole Adam step.
    // W2 is read by every workgroup of the second kernel while workgroup 0 steps it: ping-pong.
    moc_meta_t Mt = *M;
    float* cur = M->W2;
    float* nxt = ws->W2_alt;
    for (int t = 0; t < n; ++t) {
        const int b = slide0 + t;
        AdamCoef k = {};
        StepTab st = {};
        if (G) { st.tab = G->tab; st.ctr = G->ctr; st.pos = t; }
        else k = adam_coef(M, M->step + 1 + t, 1.f);
        Mt.W2 = cur;
        // the slide's S where the host knows it by now, decided per step and the same for both launches (a captured pass
        // serves other passes: never)
        const int S_host = G ? -1 : step_n_sel(B, b);
        if (int rc = launch_forward(B, &Mt, ws, b, 1, use_bits, s, p.tiles(), nullptr, 0, S_host)) return rc;
        if (int rc = launch_fused_step(p, B, &Mt, ws, labels, b, use_bits, k, nxt, s, 1, nullptr, G ? &st : nullptr, t + 1 < n ? b + 1 : -1,
                                       S_host)) return rc;
        float* tmp = cur; cur = nxt; nxt = tmp;
    }
    if (cur != M->W2) {   // odd number of steps: the current W2 lives in the scratch buffer
        if (hipMemcpyAsync(M->W2, cur, sizeof(float) * 4 * H, hipMemcpyDeviceToDevice, s) != hipSuccess)
            MOC_FAIL(MOC_ELAUNCH, "moc_train_steps: copy-back of W2 failed");
    }
    if (G) {
        step_ctr_add_kernel<<<1, 1, 0, s>>>(G->ctr, n);
        MOC_CHECK_LAUNCH("moc_step_ctr_add");
    }
    return MOC_OK;
}

}  // namespace

extern "C" size_t moc_step_graph_workspace_bytes(int max_steps) {
    return max_steps > 0 ? 16 + sizeof(AdamCoef) * (size_t)max_steps : 0;
}

extern "C" int moc_step_graph_create(void* device_ws, size_t ws_bytes, moc_step_graph_t** out) {
    MOC_REQUIRE(out && device_ws && ((uintptr_t)device_ws & 15) == 0, "moc_step_graph_create: null or unaligned workspace");
    MOC_REQUIRE(ws_bytes >= 16 + sizeof(AdamCoef) * 64, "moc_step_graph_create: workspace of %zu bytes holds fewer than 64 steps", ws_bytes);
    moc_step_graph* G = new (std::nothrow) moc_step_graph();
    MOC_REQUIRE(G, "moc_step_graph_create: out of host memory");
    memset(G, 0, sizeof(*G));
    G->ctr = (int32_t*)device_ws;
    G->tab = (AdamCoef*)((unsigned char*)device_ws + 16);
    G->cap = (int)((ws_bytes - 16) / sizeof(AdamCoef));
    G->dev_rel = -1;
    if (hipHostMalloc((void**)&G->stage, sizeof(AdamCoef) * (size_t)G->cap, hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&G->stage_done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&G->last_done, hipEventDisableTiming) != hipSuccess ||
        hipStreamCreateWithFlags(&G->cap_stream, hipStreamNonBlocking) != hipSuccess) {
        if (G->stage) (void)hipHostFree(G->stage);
        delete G;
        MOC_FAIL(MOC_ELAUNCH, "moc_step_graph_create: cannot allocate the pinned staging buffer");
    }
    *out = G;
    return MOC_OK;
}

extern "C" int moc_step_graph_destroy(moc_step_graph_t* G) {
    if (!G) return MOC_OK;
    for (int i = 0; i < G->n_entries; ++i) {
        (void)hipGraphExecDestroy(G->e[i].exec);
        (void)hipGraphDestroy(G->e[i].graph);
    }
    if (G->stage_busy) (void)hipEventSynchronize(G->stage_done);
    (void)hipEventDestroy(G->stage_done);
    (void)hipEventDestroy(G->last_done);
    (void)hipStreamDestroy(G->cap_stream);
    (void)hipHostFree(G->stage);
    delete G;
    return MOC_OK;
}

extern "C" int moc_step_graph_stats(const moc_step_graph_t* G, int* captures, int* replays, int* eager_calls) {
    MOC_REQUIRE(G, "moc_step_graph_stats: null handle");
    if (captures) *captures = G->captures;
    if (replays) *replays = G->replays;
    if (eager_calls) *eager_calls = G->eager_calls;
    return MOC_OK;
}

extern "C" int moc_train_steps_graph(moc_step_graph_t* G, const moc_batch_t* B, const moc_meta_t* M, const moc_meta_ws_t* ws,
                                     const int64_t* labels, int slide0, int n, uint32_t use_bits, moc_stream_t stream) {
    MOC_REQUIRE(G, "moc_train_steps_graph: null handle");
    if (int rc = moc_check_batch(B, "moc_train_steps_graph")) return rc;
    if (int rc = check_meta(B, M, ws, "moc_train_steps_graph", true, false)) return rc;
    MOC_REQUIRE(labels && slide0 >= 0 && n >= 1 && slide0 + n <= B->n_slides, "moc_train_steps_graph: bad labels/slide range");
    hipStream_t s = (hipStream_t)stream;
    // Grids and kernel shapes follow B->max_rows, which a masked batch tightens to the largest KEPT-row count of the
    // pass (moc_host_max_kept): a different number every pass.  A captured pass must not depend on it, so the graph is
    // built for the largest SLIDE of the range -- an upper bound of every pass's kept rows (surplus workgroups leave at
    // once on n_sel).
    // Nor on a pass's selected-row counts: n_sel_host or the mailbox would bake one pass's S, forward grid and tile bound into
    // the graph, and GraphKey has no field for them -- a captured pass always reads the device n_sel.
    moc_batch_t Bg = *B;
    Bg.n_sel_host = nullptr;
    Bg.n_sel_mail = nullptr;
    Bg.n_sel_ticket = 0;
    if (B->row_off_host) {
        int64_t mx = 1;
        for (int i = slide0; i < slide0 + n; ++i) {
            const int64_t r = B->row_off_host[i + 1] - B->row_off_host[i];
            if (r > mx) mx = r;
        }
        Bg.max_rows = (int32_t)(mx < 0x7fffffff ? mx : 0x7fffffff);
    }
    const moc_batch_t* Bo = B;     // as handed in: for the stream-launch fall-back
    B = &Bg;
    const StepPlan p = step_plan(B, ws, false);
    if (!p.one_launch() || G->eager_only || n > G->cap) {            // shapes of the three-launch step, or a handle that gave up
        G->eager_calls++;
        G->dev_rel = -1;
        return moc_train_steps(Bo, M, ws, labels, slide0, n, use_bits, stream);
    }
    if (int rc = step_attrs()) return rc;                  // (before any capture)
    if (G->has_last && G->last_stream != s) {              // the previous pass ran elsewhere: order the two on the device
        if (hipStreamWaitEvent(s, G->last_done, 0) != hipSuccess) MOC_FAIL(MOC_ELAUNCH, "moc_train_steps_graph: stream wait");
    }
    // ---- the coefficient table covers steps M->step + 1 ... M->step + n with these hyper-parameters?
    const bool same_hp = G->tab_valid && G->lr == M->lr && G->beta1 == M->beta1 && G->beta2 == M->beta2 &&
                         G->eps == M->eps && G->wd == M->weight_decay;
    if (!same_hp || M->step < G->tab_base || M->step + n > G->tab_base + G->cap) {
        if (G->stage_busy) {                               // the previous upload still owns the staging buffer
            if (hipEventSynchronize(G->stage_done) != hipSuccess) MOC_FAIL(MOC_ELAUNCH, "moc_train_steps_graph: staging event");
            G->stage_busy = false;
        }
        for (int i = 0; i < G->cap; ++i) G->stage[i] = adam_coef(M, M->step + 1 + i, 1.f);
        if (hipMemcpyAsync(G->tab, G->stage, sizeof(AdamCoef) * (size_t)G->cap, hipMemcpyHostToDevice, s) != hipSuccess ||
            hipEventRecord(G->stage_done, s) != hipSuccess)
            MOC_FAIL(MOC_ELAUNCH, "moc_train_steps_graph: upload of the coefficient table failed");
        G->stage_busy = true;
        G->tab_valid = true;
        G->lr = M->lr; G->beta1 = M->beta1; G->beta2 = M->beta2; G->eps = M->eps; G->wd = M->weight_decay;
        G->tab_base = M->step;
        G->dev_rel = -1;
    }
    // ---- the device counter stands where this optimizer's step count is?  (someone else may have stepped it, or a
    // checkpoint was loaded: one tiny launch puts it right, value by kernel argument)
    const int64_t rel = M->step - G->tab_base;
    if (G->dev_rel != rel) {
        step_ctr_set_kernel<<<1, 1, 0, s>>>(G->ctr, (int32_t)rel);
        MOC_CHECK_LAUNCH("moc_step_ctr_set");
        G->dev_rel = rel;
    }
    {   // diagnostic: the table-reading kernels as plain stream launches (separates what the table costs from what the graph costs)
        static const char* mode_env = getenv("MOC_STEP_GRAPH_MODE");
        if (mode_env && strcmp(mode_env, "table") == 0) {
            if (int rc = issue_fused_pass(p, B, M, ws, labels, slide0, n, use_bits, s, G)) return rc;
            G->eager_calls++;
            G->dev_rel = rel + n;
            G->has_last = hipEventRecord(G->last_done, s) == hipSuccess;
            G->last_stream = s;
            return MOC_OK;
        }
    }
    // ---- find or capture the pass
    GraphKey key;
    graph_key(&key, B, M, ws, labels, slide0, n, use_bits, p);
    moc_step_graph::Entry* hit = nullptr;
    for (int i = 0; i < G->n_entries; ++i)
        if (memcmp(G->e[i].key, &key, sizeof(key)) == 0) { hit = &G->e[i]; break; }
    if (!hit) {
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        int rc = MOC_OK;
        hipError_t he = hipStreamBeginCapture(G->cap_stream, hipStreamCaptureModeRelaxed);
        if (he != hipSuccess) rc = MOC_ELAUNCH;
        else {
            rc = issue_fused_pass(p, B, M, ws, labels, slide0, n, use_bits, G->cap_stream, G);
            he = hipStreamEndCapture(G->cap_stream, &graph);          // (always: leaves the stream out of capture mode)
            if (rc == MOC_OK && (he != hipSuccess || !graph)) rc = MOC_ELAUNCH;
        }
        if (rc == MOC_OK && (he = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0)) != hipSuccess) rc = MOC_ELAUNCH;
        if (rc != MOC_OK) {                                // no graph on this runtime: stream launches from now on
            moc_set_error("moc_train_steps_graph: capture / instantiation failed (%s); falling back to stream launches",
                          hipGetErrorString(he));
            if (graph) (void)hipGraphDestroy(graph);
            (void)hipGetLastError();
            G->eager_only = 1;
            G->eager_calls++;
            G->dev_rel = -1;
            return moc_train_steps(Bo, M, ws, labels, slide0, n, use_bits, stream);
        }
        if (G->n_entries < 8) hit = &G->e[G->n_entries++];
        else {                                             // replace the entry that was used longest ago
            hit = &G->e[0];
            for (int i = 1; i < 8; ++i) if (G->e[i].used < hit->used) hit = &G->e[i];
            (void)hipGraphExecDestroy(hit->exec);
            (void)hipGraphDestroy(hit->graph);
        }
        memset(hit->key, 0, sizeof(hit->key));
        memcpy(hit->key, &key, sizeof(key));
        hit->graph = graph;
        hit->exec = exec;
        G->captures++;
    }
    hit->used = ++G->tick;
    if (hipGraphLaunch(hit->exec, s) != hipSuccess) MOC_FAIL(MOC_ELAUNCH, "moc_train_steps_graph: hipGraphLaunch failed");
    G->replays++;
    G->dev_rel = rel + n;
    G->has_last = hipEventRecord(G->last_done, s) == hipSuccess;
    G->last_stream = s;
    return MOC_OK;
}

extern "C" size_t moc_tile_ws_bytes(int64_t total_rows, int n_slides, int C) {
    if (total_rows <= 0 || n_slides <= 0 || C <= 0) return 0;
    return tile_bytes(tile_slots(total_rows, n_slides, C));
}
