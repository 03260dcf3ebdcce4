"""Drop-in for the hot-path callables of the reference's main_moc.py
(senet :299-312, slide_process :322-375, train :378-410, zs_evaluation :412-460,
evaluation :462-520, ablation_evaluation :523-582): same names, arguments, return
structures and quirks, computed by libmoc_hip on the MI355X.

Like the reference, train/evaluation read the classifier bank from module
globals `zeroshot_weights` / `zeroshot_weights_ext` (set them directly or through
set_classifier_bank).

How the loops map onto the GPU
  * slide_process has no trainable parameter, so for a whole loader pass its
    work (mask -> scores -> 4 selectors -> union -> candidates: "phase A") is done
    for ALL slides in a handful of batched launches before the meta-learner runs;
  * train then takes one fused Adam step per slide, in loader order, without
    ever synchronising the host (moc_train_steps); results are those of the
    reference's sequential loop because phase A does not depend on the parameters;
  * evaluation / zs_evaluation have no sequential dependence at all and are
    batched end to end; only the [n_slides, C] pooled logits come back to the
    host, where sklearn computes the AUC as in the reference.
  * the row mask is drawn on the CPU default generator, one `torch.rand(N) > 0.5`
    per slide in loader order (main_moc.py:330).  Given the same generator state at
    the first slide, the bits are the reference's.  What differs is what ELSE draws
    from that generator: the reference iterates a DataLoader(num_workers=1), and every
    DataLoader.__iter__ -- train and each evaluation pass -- first draws a 64-bit base
    seed from the same generator.  A torch DataLoader handed to train()/evaluation()
    here makes that draw too (same stream as the reference); a ResidentBags split does
    not unless built with `loader_seed_draw=True` (then every pass over it consumes the
    draw, and phase A is no longer issued a pass ahead: the generator state the next
    train() will find is not known in advance).
"""
from __future__ import annotations

import contextlib
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from sklearn.metrics import roc_auc_score
from tqdm import tqdm

from . import engine
from .engine import Bank, MetaState, SlideBatch
from .patch_selection_classifier import (bottomk_irrel_classifier_pooling, delta_diff_classifier_pooling,
                                         delta_softmax_classifier_pooling, topj_pooling)

zeroshot_weights = None        # [D, C]      main_moc.py:161-202
zeroshot_weights_ext = None    # [D, C+4]

CONCH_TEMPERATURE = 56.3477    # main_moc.py:443, :505
# slides are processed in chunks of at most this many bag bytes per phase-A batch
MAX_BATCH_BYTES = 24 << 30


def set_classifier_bank(W: torch.Tensor, W_ext: torch.Tensor):
    global zeroshot_weights, zeroshot_weights_ext
    zeroshot_weights, zeroshot_weights_ext = W, W_ext


class _SenetFn(torch.autograd.Function):
    """`model(selected_feat)` for a caller who keeps the reference's loop body (main_moc.py:390-410) around
    slide_process: the forward is the training step's own forward kernel (moc_meta_forward over the given rows), the
    backward moc_senet_backward -- only the rows whose lambdas carry gradient (the <= K*C pooled ones) are touched."""

    @staticmethod
    def forward(ctx, x, W1, b1, W2, b2, model):
        S, D = x.shape
        xc = x.detach().contiguous()
        batch = engine.CompactBatch(1, S, S, D, xc.dtype, 2, 3, S, 1, xc.device, X=xc)
        batch.n_sel.fill_(S)
        batch.set_layout([0, S])
        meta = MetaState(model)
        keep = any(ctx.needs_input_grad[1:5])            # (grad mode is off inside forward(): ask the context)
        engine.meta_forward(batch, meta, 0, 1, 0, keep_hidden=True)
        t, _ = batch.meta_ws()
        if keep:
            ctx.save_for_backward(xc, t["H1"], t["gates"], W2.detach())
            ctx.hold = (batch, meta)                       # (the work arrays live as long as the graph)
        return t["gates"].clone()

    @staticmethod
    def backward(ctx, g):
        xc, H1, gates, W2 = ctx.saved_tensors
        S, D = xc.shape
        dev = xc.device
        g = g.detach().to(torch.float32).contiguous()
        f32 = dict(dtype=torch.float32, device=dev)
        gW1, gb1 = torch.empty((engine.HIDDEN, D), **f32), torch.empty(engine.HIDDEN, **f32)
        gW2, gb2 = torch.empty((4, engine.HIDDEN), **f32), torch.empty(4, **f32)
        dz, dh = torch.empty((S, 4), **f32), torch.empty((S, engine.HIDDEN), **f32)
        rows, n = torch.empty(S, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        engine.check(engine.lib().moc_senet_backward(
            engine.ptr(xc), engine._dtype_code(xc.dtype), S, D, engine.ptr(H1), engine.ptr(gates), engine.ptr(g), engine.ptr(W2),
            engine.ptr(gW1), engine.ptr(gb1), engine.ptr(gW2), engine.ptr(gb2), engine.ptr(dz), engine.ptr(dh), engine.ptr(rows),
            engine.ptr(n), engine._stream()), "moc_senet_backward")
        return None, gW1, gb1, gW2, gb2, None


class senet(nn.Module):
    """The meta-learner; same modules / state_dict keys as main_moc.py:299-312.
    train()/evaluation() below do not go through forward(): they hand the parameter tensors to the fused kernels.
    forward() itself -- for a caller-written loop -- runs the same forward kernel and a HIP backward (_SenetFn)."""

    def __init__(self, in_dim, out_dim):
        super(senet, self).__init__()
        self.hidden_dim = 64
        self.model = nn.Sequential(
            nn.Linear(in_dim, self.hidden_dim),
            nn.ReLU(),
            nn.Linear(self.hidden_dim, out_dim),
            nn.Sigmoid()
        )

    def forward(self, x):
        lin1, lin2 = self.model[0], self.model[2]
        if not x.is_cuda:
            raise RuntimeError(f"moc_amd.senet: the meta-learner runs on the GPU only (got a {x.device} tensor); "
                               "there is no CPU fallback")
        assert x.dim() == 2 and x.size(1) == lin1.in_features, f"senet: expected [S, {lin1.in_features}] rows"
        assert lin2.out_features == 4 and lin1.in_features % 256 == 0, \
            "senet: the HIP forward takes D a multiple of 256 and four gates (main_moc.py:314)"
        if x.requires_grad:
            raise NotImplementedError("senet: no gradient w.r.t. the bag rows on the MOC path (selected_feat is data)")
        if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            x = x.to(torch.float32)
        return _SenetFn.apply(x, lin1.weight, lin1.bias, lin2.weight, lin2.bias, self)


# --------------------------------------------------------------------------
def _bag_dtype(args, default):
    want = getattr(args, "bag_dtype", None)
    if want in (None, "keep"):
        return default
    return {"fp32": torch.float32, "float32": torch.float32, "bf16": torch.bfloat16,
            "bfloat16": torch.bfloat16, "fp16": torch.float16, "float16": torch.float16}[want]


def _pack(bags, device, dtype):
    """list of [N_i, D] tensors -> one contiguous [sum N_i, D] device array."""
    sizes = [int(b.size(0)) for b in bags]
    X = torch.empty((sum(sizes), bags[0].size(1)), dtype=dtype, device=device)
    o = 0
    for b, n in zip(bags, sizes):
        X[o:o + n].copy_(b.to(device, non_blocking=True))
        o += n
    return X, sizes


def _chunks(sizes, D, itemsize):
    out, cur, cur_bytes = [], [], 0
    for i, n in enumerate(sizes):
        nb = n * D * itemsize
        if cur and cur_bytes + nb > MAX_BATCH_BYTES:
            out.append(cur)
            cur, cur_bytes = [], 0
        cur.append(i)
        cur_bytes += nb
    if cur:
        out.append(cur)
    return out


class ResidentBags:
    """Slides kept packed in HBM across epochs with the
    loader/dataset protocol main_moc.py's loops use (iteration yields batch_size=1
    items; .dataset.real_len(), .dataset.repeat_num, len()).  train/evaluation
    recognise it and skip the per-epoch re-read + host->device copy."""

    def __init__(self, bags, labels, device, dtype=None, repeat_num=None, paths=None, loader_seed_draw=False, cache_scores=None,
                 coords=None):
        dtype = dtype or bags[0].dtype
        # opt-in: keep the per-row statistics of the split (28 B per row at two classes) from one unmasked score pass and let
        # every train pass copy its kept rows' statistics instead of reading the bags again: the same bits, phase A without
        # its HBM-bound kernel.  NOT the configuration bench.py's `value` is measured in (engine.build_stats_cache)
        self.cache_scores = (os.environ.get("MOC_CACHE_SCORES", "0") == "1") if cache_scores is None else bool(cache_scores)
        self._stats_caches = {}
        # True: every pass over this split first draws the 64-bit base seed a DataLoader.__iter__ would draw from the
        # CPU default generator (the reference's loaders do, train and evaluation alike), so a seeded run sees the
        # reference's mask stream exactly; phase A is then not issued a pass ahead (module docstring)
        self.loader_seed_draw = bool(loader_seed_draw)
        self.next_pass_len = None          # see resident_pass_done
        self.pass_after_next_len = None    # ... and the one after that, when it differs (mask draws run two passes ahead)
        self.X, self.sizes = _pack(bags, device, dtype)
        self.labels = [int(v) for v in labels]
        self.repeat_num = repeat_num
        self.paths = paths or [f"slide_{i}.h5" for i in range(len(bags))]
        self.starts = [0]
        for n in self.sizes:
            self.starts.append(self.starts[-1] + n)
        # patch coordinates (host int64 [total_rows, 2], rows as in X; zeros for bags without any) and a view per slide --
        # for the patch maps (moc_amd.patch_maps).  __iter__ does not hand them out.
        self.coords = np.zeros((self.starts[-1], 2), dtype=np.int64)
        for k, c in enumerate(coords or ()):
            if c is not None:
                c = np.asarray(c, dtype=np.int64).reshape(-1, 2)
                assert c.shape[0] == self.sizes[k], f"slide {k}: {c.shape[0]} coordinates for {self.sizes[k]} patches"
                self.coords[self.starts[k]:self.starts[k + 1]] = c
        self.slide_coords = [self.coords[self.starts[k]:self.starts[k + 1]] for k in range(len(self.sizes))]
        self.dataset = self
        self._plans = {}
        self._last_train_key = None
        self._order = None

    def train_plan(self, C_, Ce, topj, topk, discard):
        """Work arrays, labels and pinned mask staging for train() over the current visit order,
        built once and reused every epoch (only the mask bytes change)."""
        order = self.visit_order()                         # (a cached tuple)
        key = (order, C_, Ce, topj, topk, tuple(sorted(discard)) if discard else ())
        self._last_train_key = key
        plan = self._plans.get(key)
        if plan is None:
            if len(self._plans) > 8:
                self._plans.clear()
            sizes = [self.sizes[k] for k in order]
            T = sum(sizes)
            # two sets of work arrays: while the meta-learner steps through epoch e on one, phase A of
            # epoch e+1 (parameter-free) fills the other on a side stream (_resident_pass_setup)
            batches = [SlideBatch(self.X, sizes, C_, Ce, topj, topk, discard, mask=torch.ones(T, dtype=torch.uint8),
                                  x_starts=[self.starts[k] for k in order]) for _ in range(2)]
            if self.cache_scores:
                bank_ = _bank_for(self.X, self.X.device)
                ck = (id(bank_), C_, Ce)
                if ck not in self._stats_caches:
                    self._stats_caches.clear()
                    self._stats_caches[ck] = (engine.build_stats_cache(self.X, self.sizes, self.starts[:-1], bank_, topj, topk), bank_)
                for b in batches:
                    b.stats_cache = self._stats_caches[ck][0]
            if PREFETCH_PHASE_A and Ce <= 16 and not self.loader_seed_draw and not self.cache_scores:     # (loader_seed_draw: phase A always runs in line)
                # phase A runs beside the meta-steps of the pass before: leave them CUs, or (MOC_SCORE_RING) share every CU
                # with them.  (Banks of one n-tile only: wider
                # ones run ONE score workgroup per CU -- thirty classes with 64 CUs left free: score pass 242 -> 447 us,
                # 18.9 -> 18.8 k meta-steps/s.)
                for b in batches:
                    b.lookahead()
            lab = torch.tensor([self.labels[k] for k in order], dtype=torch.int64).to(self.X.device)
            stage = [torch.empty(T, dtype=torch.uint8).pin_memory() for _ in range(2)]     # (only when torch itself must draw)
            drawer = engine.MaskDrawer(T, batches[0]._row_off_c, len(sizes))
            side = torch.cuda.Stream(device=self.X.device)
            # the side stream reads X and writes the work arrays: tell the caching allocator, so that memory freed
            # while a pass-ahead phase A is still in flight is not handed to someone else under it
            self.X.record_stream(side)
            for b in batches:
                for t in (b.kept, b.n_kept, b.stats, b.sel_flag, b.sel_idx, b.sel_row, b.n_sel, b.cand, b.row_off, b.x_off, b.ticket):
                    if t is not None:
                        t.record_stream(side)
            plan = self._plans[key] = {"batch": batches[0], "batches": batches, "labels": lab, "stage": stage,
                                       "stage_free": [None, None], "turn": 0, "ahead": None, "side": side, "drawer": drawer}
        return plan

    def eval_plan(self, C_, Ce, topj, topk, discard):
        """Work arrays + labels for an un-masked pass over the current visit order, reused across calls."""
        order = tuple(self.visit_order())
        key = ("eval", order, C_, Ce, topj, topk, tuple(sorted(discard or ())))
        plan = self._plans.get(key)
        if plan is None:
            if len(self._plans) > 8:
                self._plans.clear()
            sizes = [self.sizes[k] for k in order]
            batch = SlideBatch(self.X, sizes, C_, Ce, topj, topk, discard, x_starts=[self.starts[k] for k in order])
            lab = torch.tensor([self.labels[k] for k in order], dtype=torch.int64).to(self.X.device)
            plan = self._plans[key] = {"batch": batch, "labels": lab, "label_list": [self.labels[k] for k in order]}
        return plan

    def real_len(self):
        return len(self.sizes)

    def __len__(self):
        return self.repeat_num if self.repeat_num else len(self.sizes)

    def visit_order(self):
        """Slide of each visit (repeat_num visits wrap around the real slides, dataset_generic.py:380-393); the
        tuple is cached per length: plans are keyed by it, once per pass."""
        n = len(self)
        if self._order is None or len(self._order) != n:
            self._order = tuple(i % len(self.sizes) for i in range(n))
        return self._order

    def __iter__(self):
        for k in self.visit_order():
            x = self.X[self.starts[k]:self.starts[k + 1]]
            yield (x.unsqueeze(0), torch.tensor([self.labels[k]]),
                   torch.zeros(1, x.size(0), 2, dtype=torch.int64), [self.paths[k]])


def _collect(loader, device, args, extras=None):
    """One pass over a loader -> (X, sizes, x_starts|None, labels).  `extras` (a list): gets (coords int64 [N, 2], path)
    per visit appended (the patch maps)."""
    if isinstance(loader, ResidentBags):
        order = loader.visit_order()
        sizes = [loader.sizes[k] for k in order]
        if extras is not None:
            extras.extend((loader.slide_coords[k], loader.paths[k]) for k in order)
        return loader.X, sizes, [loader.starts[k] for k in order], [loader.labels[k] for k in order]
    bags, labels = [], []
    for data in tqdm(loader, bar_format="{l_bar}{bar:10}{r_bar}", disable=args.disable_tqdm):
        feats, lbl, coords, full_path = data
        bags.append(feats.squeeze(0))
        labels.append(int(lbl.reshape(-1)[0]))
        if extras is not None:
            c = np.asarray(coords.numpy() if torch.is_tensor(coords) else coords, dtype=np.int64).reshape(-1, 2)
            p = full_path[0] if isinstance(full_path, (list, tuple)) else full_path
            extras.append((c, str(p)))
    dtype = _bag_dtype(args, bags[0].dtype if bags[0].dtype in (torch.float32, torch.bfloat16, torch.float16) else torch.float32)
    X, sizes = _pack(bags, device, dtype)
    return X, sizes, None, labels


def _sub_batch(X, sizes, x_starts, ids, C_, Ce, topj, topk, discard, masks=None):
    """SlideBatch over slides `ids` of a collected pass (views, no copies)."""
    if x_starts is None:
        starts, o = [], 0
        for n in sizes:
            starts.append(o)
            o += n
    else:
        starts = x_starts
    m = torch.cat([masks[i] for i in ids]) if masks is not None else None
    return SlideBatch(X, [sizes[i] for i in ids], C_, Ce, topj, topk, discard, mask=m,
                      x_starts=[starts[i] for i in ids])


def _bank_for(X, device, fg_from_ext=False):
    assert zeroshot_weights is not None and zeroshot_weights_ext is not None, \
        "set moc_amd.main_moc.zeroshot_weights / zeroshot_weights_ext first (set_classifier_bank)"
    return Bank.get(zeroshot_weights, zeroshot_weights_ext, X.dtype, device, fg_from_ext)


# --------------------------------------------------------------------------
def slide_process(feat, zeroshot_weights, zeroshot_weights_ext,
                  n_classes, topj=10, random_mask=False,
                  discard_classifiers=[]) -> dict:
    """main_moc.py:322-375.  `selected_index` indexes the MASKED rows, ascending."""
    device = zeroshot_weights.device
    if device.type != "cuda":
        raise RuntimeError("moc_amd.slide_process: the classifier bank must live on the GPU (no CPU fallback)")
    feat = feat.to(device)
    if feat.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        feat = feat.to(torch.float32)
    feat = feat.contiguous()
    N = feat.size(0)
    mask = None
    if random_mask:
        mask, _ = engine.draw_row_masks(N)               # == torch.rand(N) > 0.5 on the CPU default generator
    C_, Ce = zeroshot_weights.size(1), zeroshot_weights_ext.size(1)
    assert C_ == n_classes, "n_classes must equal zeroshot_weights.size(1)"
    batch = SlideBatch(feat, [N], C_, Ce, topj, 1, discard_classifiers, mask=mask)
    bank = Bank.get(zeroshot_weights, zeroshot_weights_ext, feat.dtype, device)
    batch.scores(bank)
    batch.select()
    sel_feat = batch.gather_candidates(with_feat=True)
    S = int(batch.n_sel.item())
    cand = batch.cand[:, :S]
    return {
        "selected_index": batch.sel_idx[:S].tolist(),
        "selected_feat": sel_feat[:S],
        "logits_top_classifier": cand[:C_].t().contiguous(),
        "logits_delta_softmax_classifier": cand[C_:2 * C_].t().contiguous(),
        "logits_delta_diff_classifier": cand[2 * C_].unsqueeze(1).expand(S, C_).contiguous(),
        "logits_bottomk_irrel_classifier": cand[2 * C_ + 1].unsqueeze(1).expand(S, C_).contiguous(),
    }


PREFETCH_PHASE_A = os.environ.get("MOC_PREFETCH_PHASE_A", "1") != "0"
MASK_AHEAD = os.environ.get("MOC_MASK_AHEAD", "1") != "0"   # keep flags drawn a pass ahead on a helper thread (engine.MaskDrawer)
_TRACE = os.environ.get("MOC_BENCH_TRACE") == "1"          # host time of train()'s four parts on stderr (diagnostic)


def _issue_phase_a(plan, turn, bank, rng_before, host_wait=None, chain_plan=None):
    """Draw the masks that follow generator state `rng_before` (main_moc.py:330: same stream of bits),
    upload them and run phase A into work-array set `turn` on the CURRENT stream.  `chain_plan`: the plan of the pass
    AFTER the one these masks are for, when it visits other rows (its drawer then starts on the flags that follow).
    -> generator state after the draws (None: the state's layout is unknown, torch drew and advanced itself)."""
    batch = plan["batches"][turn]
    same = chain_plan is None or chain_plan is plan
    drawn = plan["drawer"].take(rng_before, chain=same) if MASK_AHEAD else None    # usually ready: drawn a pass ahead on the helper thread
    if drawn is not None:
        stage, kept, max_kept, rng_after, buf = drawn
        if not same:
            chain_plan["drawer"].prefetch(rng_after)
    else:                                               # generator layout unknown to the replay: torch draws, in line
        if plan["stage_free"][turn] is not None:
            plan["stage_free"][turn].synchronize()      # the phase A that read that pinned buffer has run
        stage, kept, rng_after = engine.draw_row_masks_from(rng_before, batch.total, plan["stage"][turn])
        max_kept, buf = None, None
    if host_wait is not None:
        host_wait.synchronize()                         # (after the draw: the host works while it would wait)
    batch.use_host_mask(stage, kept, max_kept)          # read in place by the compaction kernel: no upload
    batch.phase_a(plan["bank"])
    ev = torch.cuda.Event()
    ev.record(engine.stream_obj())
    if buf is not None:
        plan["drawer"].attach(buf, ev)                  # ... so the buffer is free again when phase A has run
    else:
        plan["stage_free"][turn] = ev
    return rng_after


def _resident_pass_setup(res, device, args, defer_rng=False):
    """Train pass over a resident split: nothing is copied or allocated per epoch except the new mask
    bytes.  Returns (batch with this epoch's phase A issued, device labels, bank).

    Phase A has no trainable parameter, so the pass for epoch e+1 is issued one call AHEAD, on a side
    stream, while the sequential meta-steps of epoch e occupy a fraction of the GPU (resident_pass_done).
    It is speculative only in what the CPU generator will hold when train() is called again: the masks
    are drawn from a COPY of the state, torch's generator is left where epoch e put it, and the next call
    adopts the work only if it finds exactly that state (and the same bank); otherwise it is dropped and
    phase A runs here, as before."""
    bank = _bank_for(res.X, device)
    assert bank.C == args.n_classes
    plan = res.train_plan(bank.C, bank.Ce, args.topj, args.topk, args.discard_classifiers)
    plan["bank"] = bank
    lab = plan["labels"]
    now = torch.get_rng_state()
    ahead, plan["ahead"] = plan["ahead"], None
    plan["rng_after"] = None
    if ahead is not None and ahead["bank"] is bank and ahead["after"] is not None and torch.equal(ahead["before"], now):
        # the draws happened: the generator is put where they leave it -- by the caller, AFTER the pass's launches are
        # issued (train(): 3 us that the first launch of the pass need not wait for)
        if defer_rng:
            plan["rng_after"] = ahead["after"]
        else:
            torch.set_rng_state(ahead["after"])
        ahead["done"].wait(engine.stream_obj())         # (the current stream waits; its Stream object is a cached one)
        plan["turn"] = ahead["turn"]
    else:
        if ahead is not None:
            ahead["done"].synchronize()                 # dropped work still owns that set of arrays until it ends
        plan["turn"] = 1 - plan["turn"]
        after = _issue_phase_a(plan, plan["turn"], bank, now)
        if after is not None:
            torch.set_rng_state(after)
    plan["batch"] = plan["batches"][plan["turn"]]
    return plan["batch"], lab, bank


def _next_plan(res, plan, bank, args, which="next_pass_len"):
    """The plan of the pass that follows this one: the same visits (the reference's epoch loop), or what the caller
    announced in `res.next_pass_len` (0: no pass follows -> None).  which="pass_after_next_len": the pass after that."""
    hint = getattr(res, which, None)
    if hint == 0:
        return None
    if hint is None and which != "next_pass_len":
        hint = getattr(res, "next_pass_len", None)       # (not announced: as the next one)
        if hint == 0:
            return None
    if hint is None or hint == len(res):
        return plan
    keep, res.repeat_num = res.repeat_num, (hint if hint != res.real_len() else None)
    try:
        return res.train_plan(bank.C, bank.Ce, args.topj, args.topk, args.discard_classifiers)
    finally:
        res.repeat_num = keep


def resident_pass_done(res, device, args):
    """Call after the pass's meta-steps are issued: starts phase A of the NEXT pass on the side stream.

    The next pass is taken to visit what this one visited (the reference's epoch loop, main_moc.py:606-628).  A
    caller that knows better says so in `res.next_pass_len`: a number of visits (bench.py's partial passes), or 0
    for "no pass follows" (nothing is issued ahead)."""
    if not PREFETCH_PHASE_A or res.loader_seed_draw:
        return
    bank = _bank_for(res.X, device)
    plan = res.train_plan(bank.C, bank.Ce, args.topj, args.topk, args.discard_classifiers)
    # a set of arrays is free again when the meta-steps that read it have run: mark this pass's end on `main`;
    # the other set was last read by the PREVIOUS pass's meta-steps (their mark was left one call ago), so the
    # side stream waits for that one only and phase A of the next pass overlaps THIS pass's meta-steps
    mark = torch.cuda.Event()
    mark.record(engine.stream_obj())                    # (on the current stream -- `main` below)
    plan.setdefault("steps_done", [None, None])[plan["turn"]] = mark
    nplan = _next_plan(res, plan, bank, args)
    if nplan is None:
        return
    if nplan is not plan and nplan.get("ahead") is not None:     # (an unadopted speculation of that plan still owns a set)
        nplan["ahead"]["done"].synchronize()
        nplan["ahead"] = None
    nplan["bank"] = bank
    other, side = 1 - nplan["turn"], nplan["side"]
    before = torch.get_rng_state()
    # The HOST waits for that mark, not the side stream: a stream-side wait on an event of the main stream
    # cost ~45 us of GPU time per pass here (scripts/diag_overlap.py: 0.76 ms per epoch against 0.72), and
    # the host is a pass ahead with this pass's launches already queued, so its wait starves nothing.
    chain = _next_plan(res, plan, bank, args, which="pass_after_next_len")
    with torch.cuda.stream(side):
        after = _issue_phase_a(nplan, other, bank, before, host_wait=nplan.setdefault("steps_done", [None, None])[other],
                               chain_plan=chain)
        done = torch.cuda.Event()
        done.record(side)
    if after is None:                                   # torch drew for us and moved its generator: undo, no speculation
        torch.set_rng_state(before)
    nplan["ahead"] = {"turn": other, "before": before, "after": after, "done": done, "bank": bank}


def train(model, train_loader, optimizer, device, args):
    """main_moc.py:378-410: one Adam step per slide, in loader order."""
    if not model.training:
        model.train()
    use = engine.train_use_bits(args.discard_classifiers)
    if isinstance(train_loader, ResidentBags):
        _loader_seed_draw(train_loader)
        if _TRACE:
            import time
            t0 = time.perf_counter()
        batch, lab, bank = _resident_pass_setup(train_loader, device, args, defer_rng=True)      # phase A issued (or adopted)
        if _TRACE:
            t1 = time.perf_counter()
        meta = MetaState.cached(model, optimizer)
        if _TRACE:
            t2 = time.perf_counter()
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
        engine.train_steps(batch, meta, lab, 0, batch.n_slides, use)
        plan_ = train_loader._plans.get(train_loader._last_train_key)
        if plan_ is not None and plan_.get("rng_after") is not None:
            torch.set_rng_state(plan_["rng_after"])     # (see _resident_pass_setup)
            plan_["rng_after"] = None
        if _TRACE:
            ev1.record()
            train.trace_events = getattr(train, "trace_events", [])[-200:] + [(batch.n_slides, ev0, ev1)]
            t3 = time.perf_counter()
        resident_pass_done(train_loader, device, args)
        if _TRACE:
            t4 = time.perf_counter()
            # (kept, not printed: a print inside a timed region is 30 us of it; bench.py prints the list afterwards)
            train.trace_host = getattr(train, "trace_host", [])[-200:] + [
                f"setup {(t1 - t0) * 1e6:.0f}  meta {(t2 - t1) * 1e6:.0f}  launches {(t3 - t2) * 1e6:.0f}  pass_done {(t4 - t3) * 1e6:.0f} us"]
        train.last = (batch, lab)
        return
    X, sizes, x_starts, labels = _collect(train_loader, device, args)
    mask_all, _ = engine.draw_row_masks(sum(sizes))      # main_moc.py:330, one draw per slide, in order
    masks, o = [], 0
    for n in sizes:
        masks.append(mask_all[o:o + n])
        o += n
    meta = MetaState(model, optimizer)
    bank = _bank_for(X, device)
    C_, Ce = bank.C, bank.Ce
    assert C_ == args.n_classes
    for ids in _chunks(sizes, X.size(1), X.element_size()):
        batch = _sub_batch(X, sizes, x_starts, ids, C_, Ce, args.topj, args.topk, args.discard_classifiers, masks)
        lab = torch.tensor([labels[i] for i in ids], dtype=torch.int64).to(device, non_blocking=True)
        batch.phase_a(bank)
        engine.train_steps(batch, meta, lab, 0, len(ids), use)
        train.last = (batch, lab)    # keeps the buffers alive until the stream has drained; also for tests


_run_sets = {}


def train_runs(models, train_loaders, optimizers, device, args, generators=None, per_run_adam=False, banks=None, bank_of_run=None):
    """main_moc.py:378-410 for several independent runs at once -- what scripts/moc_train.sh:11-31 starts as one process per
    (fold, shot): `train(models[r], train_loaders[r], optimizers[r], device, args)` for every r, stepped in lockstep by one
    launch pair per meta-step (moc_amd.runs.TrainRuns; include/moc_hip.h moc_train_steps_runs).  Per run bit-identical to
    `train` from the same mask stream; run r's masks come from `generators[r]` (a private CPU torch.Generator each; by
    default seeded from the default generator on the first call).  The loaders are resident splits (ResidentBags); their
    passes may differ in length (runs.group_runs: one lockstep chain per length).  `args` may be a list of one namespace per
    run: run r then trains with args[r].topj / .topk / .discard_classifiers (a hyper-parameter grid; runs that name the same
    split object and hold equal generator states share one draw and one score pass per pass -- DESIGN.md section 9h).
    `per_run_adam`: every run steps with its own optimizer's lr / betas / eps / weight_decay (re-read every pass) instead
    of the runs having to share them -- the cells of an lr x weight-decay grid in one lockstep chain.
    `banks` = [(W, W_ext), ...] with `bank_of_run`: run r trains under banks[bank_of_run[r]] instead of the module's bank (a
    bank grid: the runs of one split and generator state share one draw and one multi-bank score pass -- DESIGN.md section 9l).
    -> the TrainRuns object (kept for the next pass: call again with the same lists)."""
    from .runs import TrainRuns
    hp = lambda a: (a.topj, a.topk, tuple(sorted(a.discard_classifiers or ())))
    key = (tuple(id(m) for m in models), tuple(id(o) for o in optimizers), tuple(id(l) for l in train_loaders),
           tuple(hp(a) for a in args) if isinstance(args, (list, tuple)) else hp(args), tuple(len(l) for l in train_loaders),
           bool(per_run_adam), None if banks is None else (tuple((id(b[0]), id(b[1])) for b in banks), tuple(bank_of_run or ())))
    ent = _run_sets.get(key)
    if ent is None:
        if len(_run_sets) > 2:
            _run_sets.clear()
        ent = _run_sets[key] = (TrainRuns(models, optimizers, train_loaders, device, args, generators=generators, per_run_adam=per_run_adam,
                                          banks=banks, bank_of_run=bank_of_run),
                                list(models), list(optimizers), list(train_loaders))
    rs = ent[0]
    rs.train_pass()
    train_runs.last = rs
    return rs


def _binary_auc(pos: np.ndarray, score: np.ndarray) -> float:
    """Area under the ROC curve of `score` for the boolean labels `pos`: the Mann-Whitney statistic with
    mid-ranks for ties, which is what the trapezoid over sklearn's roc_curve thresholds adds up to."""
    order = np.argsort(score, kind="mergesort")
    s = score[order]
    # mid-rank of every tie group: first occurrence index + (group size - 1) / 2, 1-based
    # (plain array writes, not np.r_: its index-trick machinery is 25 us a call, a third of this function)
    start = np.empty(s.size, dtype=bool)
    start[0] = True
    np.not_equal(s[1:], s[:-1], out=start[1:])
    first = np.flatnonzero(start)
    size = np.empty(first.size, dtype=np.int64)
    size[:-1] = first[1:] - first[:-1]
    size[-1] = s.size - first[-1]
    mid = np.repeat(first + (size - 1) / 2.0 + 1.0, size)
    n_pos = int(pos.sum())
    n_neg = pos.size - n_pos
    return float((mid[pos[order]].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


def _auc(y_true: np.ndarray, y_score: np.ndarray) -> float:
    """roc_auc_score(y, p[:, 1]) for two classes, roc_auc_score(y, p, multi_class='ovo', average='macro')
    otherwise (main_moc.py:507-514), computed directly: sklearn's input validation and per-pair Python
    machinery cost 0.4 ms per binary call and 0.1-0.6 s per call at 30-64 classes -- more than the GPU
    side of the whole evaluation.  Anything sklearn would reject (a class missing from y_true, ...) is
    handed to sklearn so that the same exception comes out."""
    classes = np.unique(y_true)
    if y_score.ndim == 1:
        if classes.size != 2:
            return roc_auc_score(y_true, y_score)
        return _binary_auc(y_true == classes[1], y_score)
    if classes.size != y_score.shape[1] or classes.size < 2 or not np.array_equal(classes, np.arange(classes.size)):
        return roc_auc_score(y_true, y_score, multi_class="ovo", average="macro")
    n, Cn = y_score.shape
    if n <= 4 * Cn * (Cn - 1):        # n^2 comparisons against C (C - 1) sorts of ~2n/C values: many classes, few slides
        # every pair at once.  G[i, j] = [p[i, y_i] > p[j, y_i]] + [==] / 2; U[a, b] = sum of G over i in a, j in b
        # = n_a n_b x the AUC of class a against class b on column a (Mann-Whitney, ties at one half).  Sums of
        # multiples of 1/2: exact.  (np.bincount, not a matrix product: BLAS starts a thread per visible core.)
        own = y_score[np.arange(n), y_true]
        cols = y_score[:, y_true].T
        G = (own[:, None] > cols) + 0.5 * (own[:, None] == cols)
        pair = (y_true[:, None] * Cn + y_true[None, :]).ravel()
        U = np.bincount(pair, weights=G.ravel(), minlength=Cn * Cn).reshape(Cn, Cn)
        cnt = np.bincount(y_true, minlength=Cn).astype(np.float64)
        A = U / np.outer(cnt, cnt)
        return float((A.sum() - np.trace(A)) / (Cn * (Cn - 1)))
    masks = [y_true == c for c in classes]
    total, n_pairs = 0.0, 0
    for a in range(classes.size):
        for b in range(a + 1, classes.size):
            ab = masks[a] | masks[b]
            a_true = masks[a][ab]
            total += (_binary_auc(a_true, y_score[ab, a]) + _binary_auc(~a_true, y_score[ab, b])) / 2.0
            n_pairs += 1
    return total / n_pairs


def _metrics(pooled_cpu, labels, losses, n_div, real_len, args):
    """The shared tail of the three evaluation loops (main_moc.py:439-460, :501-520)."""
    test_loss = 0
    for v in losses:
        test_loss += v
    test_loss /= n_div
    lbl_all = torch.tensor(labels, dtype=torch.int64)
    correct = int((pooled_cpu.argmax(dim=1) == lbl_all).sum().item())
    if args.pretrain == 'conch':
        temperature = CONCH_TEMPERATURE
    else:
        raise NotImplementedError
    probs = F.softmax(pooled_cpu * temperature, dim=1)
    class_probs = probs[:, 1] if probs.shape[1] == 2 else probs
    auc = _auc(lbl_all.numpy(), class_probs.numpy())
    return {"loss": test_loss, "acc": correct / real_len, "auc": auc}


@contextlib.contextmanager
def _every_slide_once(*loaders, restore="len"):
    """The scope of every evaluation pass: no gradients, and each loader's dataset visits every slide once
    (repeat_num = real_len()) -> real_len() of the first.  On exit, an exception included, repeat_num is put back, last
    loader first, in one of two ways -- both the reference's, both observable:
      "len":  to what len(dataset) was (evaluation, main_moc.py:470, :499): a split that came with None leaves with real_len();
      "attr": to what the attribute was (zs_evaluation, main_moc.py:418, :437): None stays None.
    The metrics' divisor is len(dataset) AFTER the exit."""
    assert restore in ("len", "attr")
    saved = []
    with torch.no_grad():
        for ld in loaders:
            ds = ld.dataset
            saved.append((ds, ds.repeat_num if restore == "attr" else len(ds)))
            ds.repeat_num = ds.real_len()
        try:
            yield loaders[0].dataset.real_len()
        finally:
            for ds, was in reversed(saved):
                ds.repeat_num = was


class _Chunks:
    """The host side of a pass: per key the chunks' [n, C + 1] rows (pooled | loss; slabs=True: [n_K, n, C + 1], one slab
    per topk) and the labels of the slides, in visit order -> the pass's rows, or its metrics."""

    def __init__(self, keys=(None,), slabs=False):
        self.parts, self.labels, self.dim = {k: [] for k in keys}, [], int(slabs)

    def rows(self, key=None, of=None):
        """(pooled [N, C], labels, losses) of a key; `of`: these rows only."""
        v = torch.cat(self.parts[key], 0)
        if of is None:
            return v[:, :-1].contiguous(), self.labels, v[:, -1].tolist()
        return v[of, :-1].contiguous(), [self.labels[i] for i in of.tolist()], v[of, -1].tolist()

    def metrics(self, key, loader, real_len, args):
        """_metrics of a key's rows; slabs: one dict per topk."""
        n_div = len(loader.dataset)
        if not self.dim:
            return _metrics(*self.rows(key), n_div, real_len, args)
        v = torch.cat(self.parts[key], 1)
        return [_metrics(s[:, :-1].contiguous(), self.labels, s[:, -1].tolist(), n_div, real_len, args) for s in v]


_ZS_KINDS = {topj_pooling: "topj", delta_softmax_classifier_pooling: "delta_softmax",
             delta_diff_classifier_pooling: "delta_diff", bottomk_irrel_classifier_pooling: "bottomk"}


def _zs_columns(st, C_, kind):
    """(keys, vals, smallest, key_shared) of a fused zero-shot pooling function over the full statistics layout."""
    if kind == "topj":
        return st[:C_], st[:C_], False, False
    if kind == "delta_softmax":
        return st[C_:2 * C_], st[:C_], False, False
    if kind == "delta_diff":
        return st[2 * C_:2 * C_ + 1], st[:C_], False, True
    return st[2 * C_ + 1:2 * C_ + 2], st[:C_], True, True      # bottomk: K rows of smallest background mass


def _host_rows(batch):
    """A chunk's pooled logits | loss on the host, [n, C + 1]: the one device->host transfer of the chunk."""
    t, _ = batch.meta_ws()
    return torch.cat([t["pooled"], t["loss"].unsqueeze(1)], 1).cpu()


def _zs_step(batch, kind, lab, topk):
    """A chunk of a fused zero-shot pass, over a batch whose statistics exist (full layout)."""
    t, _ = batch.meta_ws()
    keys, vals, small, shared = _zs_columns(batch.stats, batch.C, kind)
    t["pooled"].copy_(engine.topk_mean(keys, vals, topk, smallest=small, key_shared=shared, seg_off=batch.row_off))
    engine.loss_only(batch, lab, 0, batch.n_slides)
    return _host_rows(batch)


def _eval_step(batch, meta, lab, use_bits, bank=None):
    """A chunk of evaluation(): from `bank`, phase A as evaluation issues it; bank=None: the batch's statistics exist (a
    bank set's score pass), the rest of that phase A follows them.  Then the meta forward and the pooling."""
    if bank is not None:
        batch.phase_a(bank, for_eval=True)
    else:
        batch.select_for_eval()
    engine.meta_forward(batch, meta, 0, batch.n_slides, use_bits, keep_hidden=False)
    engine.pool_loss(batch, lab, 0, batch.n_slides)
    return _host_rows(batch)


def _eval_batches(loader, device, args, mode, extras=None):
    """(batch, device labels, label list) per chunk of an evaluation pass.  `extras`: see _collect."""
    discard = args.discard_classifiers if mode == "eval" else []
    if isinstance(loader, ResidentBags) and loader.X.numel() * loader.X.element_size() <= MAX_BATCH_BYTES:
        bank = _bank_for(loader.X, device, fg_from_ext=(mode == "zs_bottomk"))
        plan = loader.eval_plan(bank.C, bank.Ce, args.topj, args.topk, discard)
        if extras is not None:
            extras.extend((loader.slide_coords[k], loader.paths[k]) for k in loader.visit_order())
        return bank, [(plan["batch"], plan["labels"], plan["label_list"])]
    X, sizes, x_starts, labels = _collect(loader, device, args, extras)
    bank = _bank_for(X, device, fg_from_ext=(mode == "zs_bottomk"))
    out = []
    for ids in _chunks(sizes, X.size(1), X.element_size()):
        batch = _sub_batch(X, sizes, x_starts, ids, bank.C, bank.Ce, args.topj, args.topk, discard)
        lab_list = [labels[i] for i in ids]
        out.append((batch, torch.tensor(lab_list, dtype=torch.int64).to(device, non_blocking=True), lab_list))
    return bank, out


def _loader_seed_draw(loader):
    """What `DataLoader.__iter__` takes from the CPU default generator before the first item (its base seed)."""
    if isinstance(loader, ResidentBags) and loader.loader_seed_draw:
        torch.empty((), dtype=torch.int64).random_()


_ext_as_bank = {}


def _ext_logits_bank(X, device):
    """A bank whose "foreground" columns are ALL of zeroshot_weights_ext (plus one zero background column, which the
    bank layout needs): after batch.scores(bank), stats[:Ce] is `feats @ zeroshot_weights_ext` (main_moc.py:428)."""
    We = zeroshot_weights_ext
    key = (We.data_ptr(), We._version, tuple(We.shape))
    pad = _ext_as_bank.get(key)
    if pad is None:
        _ext_as_bank.clear()
        pad = _ext_as_bank[key] = torch.cat([We, torch.zeros_like(We[:, :1])], 1).contiguous()
    return Bank.get(We, pad, X.dtype, device)


def _eval_pass_custom(loader, device, args, pooling_func):
    """zs_evaluation with a pooling function that is not one of this package's four: the reference calls anything
    else as `pooling_func(feats @ zeroshot_weights_ext, [args.topk], coords_list=args.n_classes)[1][args.topk]`
    (main_moc.py:431-432).  The logits are formed by the score kernel, slide-batched; the callable then runs per
    slide on the device tensor, as it would in the reference."""
    _loader_seed_draw(loader)
    X, sizes, x_starts, labels = _collect(loader, device, args)
    bank = _ext_logits_bank(X, device)
    Ce = bank.C
    out = _Chunks()
    out.labels = labels
    for ids in _chunks(sizes, X.size(1), X.element_size()):
        batch = _sub_batch(X, sizes, x_starts, ids, bank.C, bank.Ce, args.topj, args.topk, [])
        batch.scores(bank)
        rows = []
        for b in range(len(ids)):
            o, n = batch.row_off_host[b], batch.sizes[b]
            logits_ext = batch.stats[:Ce, o:o + n].t().contiguous()
            rows.append(pooling_func(logits_ext, [args.topk], coords_list=args.n_classes)[1][args.topk].reshape(1, -1))
        pooled = torch.cat(rows, 0).to(torch.float32).contiguous()
        lab = torch.tensor([labels[i] for i in ids], dtype=torch.int64).to(device)
        loss, _ = engine.ce_loss(pooled, lab)
        out.parts[None].append(torch.cat([pooled, loss.unsqueeze(1)], 1).cpu())
    return out.rows()


def _eval_pass(loader, device, args, mode, model=None):
    """One pass in `mode` ("eval", "ablation", "zs_" + a fused kind) -> (pooled [N, C] on the host, labels, losses)."""
    _loader_seed_draw(loader)
    bank, batches = _eval_batches(loader, device, args, mode)
    meta = MetaState(model) if model is not None else None
    use_bits = engine.eval_use_bits(args.discard_classifiers) if mode == "eval" else 0
    out = _Chunks()
    for batch, lab, lab_list in batches:
        if mode.startswith("zs"):
            batch.scores(bank)
            rows = _zs_step(batch, mode[3:], lab, args.topk)
        elif mode == "eval":
            rows = _eval_step(batch, meta, lab, use_bits, bank)
        else:
            batch.phase_a(bank)
            engine.mix_fixed(batch, 0, batch.n_slides, args.ablation_study)
            engine.pool_loss(batch, lab, 0, batch.n_slides)
            rows = _host_rows(batch)
        out.parts[None].append(rows)
        out.labels.extend(lab_list)
    return out.rows()


def zs_evaluation(loader, device, args, pooling_func=topj_pooling):
    """main_moc.py:412-460."""
    with _every_slide_once(loader, restore="attr") as real_len:
        if pooling_func in _ZS_KINDS:
            pooled, labels, losses = _eval_pass(loader, device, args, "zs_" + _ZS_KINDS[pooling_func])
        else:           # any other callable, as the reference accepts (main_moc.py:429-432)
            pooled, labels, losses = _eval_pass_custom(loader, device, args, pooling_func)
    return _metrics(pooled, labels, losses, len(loader.dataset), real_len, args)


def evaluation(model, loader, device, args):
    """main_moc.py:462-520 (incl. the eval-side mix quirk, see engine.eval_use_bits)."""
    if model.training:                   # (nn.Module.eval() walks the module tree: 20 us of an 1 ms pass)
        model.eval()
    with _every_slide_once(loader) as real_len:
        pooled, labels, losses = _eval_pass(loader, device, args, "eval", model=model)
    return _metrics(pooled, labels, losses, len(loader.dataset), real_len, args)


# ---- sensitivity sweeps: the (topj, topk, discard) table of one split from ONE score pass ---------------------------------
SWEEP_MAX_TOPK = engine.MULTI_MAX_K     # one ranking serves every K up to here bit for bit (moc_topk_mean_multi)
ZS_POOLING_FUNCS = (topj_pooling, delta_softmax_classifier_pooling, delta_diff_classifier_pooling,
                    bottomk_irrel_classifier_pooling)


def _sweep_checks(who, loader, topks):
    topks = [int(k) for k in topks]
    assert len(topks) >= 1, f"{who}: no topk given"
    assert all(1 <= k <= SWEEP_MAX_TOPK for k in topks), \
        f"{who}: every topk must lie in [1, {SWEEP_MAX_TOPK}] (above {SWEEP_MAX_TOPK} a K's mean is no prefix of a longer ranking's sum); got {topks}"
    assert isinstance(loader, ResidentBags), f"{who}: resident splits only (main_moc.ResidentBags)"
    assert not loader.loader_seed_draw, f"{who}: loader_seed_draw splits are not swept"
    return topks


def _sweep_axes(who, args, topjs, discard_sets):
    """The (topj, discard) axes of a model sweep -> the distinct (topj, discard tuple) pairs, topj outermost;
    discard_sets=None: the one of args."""
    topjs = [int(j) for j in topjs]
    assert topjs and min(topjs) >= 1, f"{who}: topj must be >= 1"
    sets = [tuple(d) for d in ([args.discard_classifiers or ()] if discard_sets is None else discard_sets)]
    assert sets, f"{who}: no discard set given"
    return list(dict.fromkeys((j, d) for j in topjs for d in sets))


def _pool_slabs(keys, vals, topks, lab, n, small=False, shared=False, seg_off=None, seg_len=None):
    """[n_K, n, C + 1] on the device: per K the pooled logits of moc_topk_mean at that K | their loss (moc_ce_loss) -- one
    ranking per group of at most eight K."""
    Cc = vals.size(0)
    out = torch.empty((len(topks), n, Cc + 1), dtype=torch.float32, device=vals.device)
    for g0 in range(0, len(topks), engine.MULTI_MAX_NK):
        ks = topks[g0:g0 + engine.MULTI_MAX_NK]
        slabs = engine.topk_mean_multi(keys, vals, ks, smallest=small, key_shared=shared, seg_off=seg_off, seg_len=seg_len)
        for i in range(len(ks)):
            out[g0 + i, :, :Cc] = slabs[i]
            out[g0 + i, :, Cc] = engine.ce_loss(slabs[i], lab)[0]
    return out


def _pool_loss_slabs(batch, topks, lab, n):
    """The same [n_K, n, C + 1] by evaluation()'s own launch, moc_pool_loss, once per K (the batch's topk set to it).  For
    3 .. 16 classes: there evaluation() may pool and take the loss in ONE kernel (moc_meta.hip pool_step_kernel, K <= 16),
    whose cross entropy adds the C exponentials in a butterfly where moc_ce_loss adds them in class order -- the same sum
    for one or two classes, and never taken above sixteen, but in between a loss could differ in its last bit.  The cell
    must be evaluation()'s float, so it takes evaluation()'s launch; the ranking it repeats is the cheap end of a tail."""
    t, ws = batch.meta_ws()
    Cc = batch.C
    out = torch.empty((len(topks), n, Cc + 1), dtype=torch.float32, device=batch.device)
    w = type(ws).from_buffer_copy(ws)
    idx = torch.empty((n, Cc, max(topks)), dtype=torch.int32, device=batch.device)     # (the batch's own holds args.topk rows)
    w.topk_idx = engine.ptr(idx)
    keep = batch.c.topk
    try:
        for i, k in enumerate(topks):
            batch.c.topk = k
            engine.check(engine.lib().moc_pool_loss(engine.C.byref(batch.c), engine.C.byref(w), engine.ptr(lab), 0, n,
                                                    engine._stream()), "moc_pool_loss")
            out[i, :, :Cc] = t["pooled"]
            out[i, :, Cc] = t["loss"]
    finally:
        batch.c.topk = keep
    return out


def _sweep_configs(batch, meta, lab, acc, configs, topks, g=()):
    """evaluation_sweep's loop over a batch whose statistics exist (flags cleared by the score pass): per (topj, discard)
    of `configs` the selection, the candidates, the meta forward and the pooled logits | loss of every topk, appended to
    acc.parts[g + (topj, discard)].  Leaves the batch's topj / discard_bits changed: see SlideBatch.borrowed."""
    n = batch.n_slides
    tensors, _ = batch.meta_ws()
    for ci, (j, d) in enumerate(configs):
        batch.select_for_eval(j, d, clear=ci > 0)
        engine.meta_forward(batch, meta, 0, n, engine.eval_use_bits(d), keep_hidden=False)
        mixed = tensors["mixed"]
        if batch.C <= 2 or batch.C > 16:
            slabs = _pool_slabs(mixed, mixed, topks, lab, n, seg_off=batch.row_off, seg_len=batch.n_sel)
        else:
            slabs = _pool_loss_slabs(batch, topks, lab, n)
        acc.parts[g + (j, d)].append(slabs.cpu())


def _sweep_cells(acc, configs, topks, loader, real_len, args, g=()):
    """{(topj, topk, discard): metrics} from the slabs kept under g + (topj, discard)."""
    return {(j, k, d): m for j, d in configs for k, m in zip(topks, acc.metrics(g + (j, d), loader, real_len, args))}


def evaluation_sweep(model, loader, device, args, topjs, topks, discard_sets=None):
    """{(topj, topk, tuple(discard)): evaluation(model, loader, device, args')} for every combination, args' = args with
    those three fields -- the same floats -- from ONE score pass per chunk: the statistics depend on none of the three.  Per
    chunk: mask compaction + scores once; per (topj, discard) the selection, the candidates and the meta forward; one
    moc_topk_mean_multi over the mixed scores for all topk (each at most 64) and moc_ce_loss per K (3 .. 16 classes:
    _pool_loss_slabs); one device-to-host copy per (topj, discard).
    discard_sets=None: [args.discard_classifiers].  Resident splits without loader_seed_draw only."""
    topks = _sweep_checks("evaluation_sweep", loader, topks)
    configs = _sweep_axes("evaluation_sweep", args, topjs, discard_sets)
    if model.training:
        model.eval()
    acc = _Chunks(configs, slabs=True)
    with _every_slide_once(loader) as real_len:
        bank, batches = _eval_batches(loader, device, args, "eval")
        meta = MetaState(model)
        for batch, lab, lab_list in batches:
            with batch.borrowed():                   # (the batch may be a cached plan's)
                batch.scores_for_eval(bank)          # once
                _sweep_configs(batch, meta, lab, acc, configs, topks)
            acc.labels.extend(lab_list)
    return _sweep_cells(acc, configs, topks, loader, real_len, args)


def zs_evaluation_sweep(loader, device, args, topks, pooling_funcs=ZS_POOLING_FUNCS):
    """{(pooling_func.__name__, topk): zs_evaluation(loader, device, args', pooling_func)} with args'.topk = topk -- the
    same floats -- from one score pass (full statistics layout) and one moc_topk_mean_multi per pooling function, with
    that function's key / value columns.  (bottomk_irrel_classifier_pooling ranks the logits of zeroshot_weights_ext: it
    shares the pass when those foreground columns ARE zeroshot_weights, and gets a pass of its own otherwise.)  Only the
    four fused pooling functions; any other callable stays with zs_evaluation."""
    topks = _sweep_checks("zs_evaluation_sweep", loader, topks)
    funcs = _zs_funcs("zs_evaluation_sweep", pooling_funcs)
    ext_is_fg = _ext_is_fg(zeroshot_weights, zeroshot_weights_ext)
    passes = {}                          # fg_from_ext -> the functions scored by that bank
    for f in funcs:
        passes.setdefault(_ZS_KINDS[f] == "bottomk" and not ext_is_fg, []).append(f)
    acc = _Chunks(funcs, slabs=True)
    with _every_slide_once(loader, restore="attr") as real_len:
        for pi, (from_ext, fs) in enumerate(passes.items()):
            bank, batches = _eval_batches(loader, device, args, "zs_bottomk" if from_ext else "zs_topj")
            for batch, lab, lab_list in batches:
                batch.scores(bank)
                for f in fs:
                    acc.parts[f].append(_zs_slabs(batch, _ZS_KINDS[f], topks, lab))
                if pi == 0:
                    acc.labels.extend(lab_list)
    return _zs_cells(acc, funcs, topks, loader, real_len, args)


def _zs_funcs(who, pooling_funcs):
    funcs = list(pooling_funcs)
    assert funcs and all(f in _ZS_KINDS for f in funcs), \
        f"{who}: only the four fused pooling functions (others: zs_evaluation, one call each)"
    return funcs


def _zs_slabs(batch, kind, topks, lab):
    """A chunk of a fused zero-shot sweep, over a batch whose statistics exist: [n_K, n, C + 1] on the host."""
    keys, vals, small, shared = _zs_columns(batch.stats, batch.C, kind)
    return _pool_slabs(keys, vals, topks, lab, batch.n_slides, small, shared, seg_off=batch.row_off).cpu()


def _zs_cells(acc, funcs, topks, loader, real_len, args, of=lambda f: f):
    """{(pooling function's name, topk): metrics} from the slabs kept under of(f)."""
    return {(f.__name__, k): m for f in funcs for k, m in zip(topks, acc.metrics(of(f), loader, real_len, args))}


# ---- bank sweeps: several prompt banks of one class count from ONE read of the bags per group of banks ------------------
def _bank_checks(who, loader, banks):
    """The refusals of the bank forms, before any launch -> the banks as (W, W_ext) tuples."""
    assert isinstance(loader, ResidentBags), f"{who}: resident splits only (main_moc.ResidentBags)"
    assert not loader.loader_seed_draw, f"{who}: loader_seed_draw splits are not swept"
    banks = [(b[0], b[1]) for b in banks]
    assert banks, f"{who}: no bank given"
    Cs = sorted({int(W.size(1)) for W, _ in banks})
    assert len(Cs) == 1, f"{who}: banks of different C ({Cs}) do not share a score pass; group them by class count"
    for g, (W, We) in enumerate(banks):
        assert W.dim() == 2 and We.dim() == 2 and W.size(0) == We.size(0) == loader.X.size(1), f"{who}: bank {g}: bad shapes"
        assert We.size(1) <= engine.BANK_SET_MAX_CE, \
            (f"{who}: bank {g} has Ce={We.size(1)} columns; the multi-bank score pass takes banks of at most "
             f"{engine.BANK_SET_MAX_CE} (one n-tile each) -- wide banks keep zs_evaluation / evaluation per bank")
    return banks


def _chunks_banks(sizes, D, itemsize, n_banks, C_):
    """_chunks for a pass over `n_banks` banks: MAX_BATCH_BYTES bounds a chunk's bags once and, separately, its per-bank
    work arrays n_banks times (engine.bank_work_row_bytes a row and bank).  Pure."""
    per_row_work = n_banks * engine.bank_work_row_bytes(C_)
    out, cur, bag_b, work_b = [], [], 0, 0
    for i, n in enumerate(sizes):
        nb, nw = n * D * itemsize, n * per_row_work
        if cur and (bag_b + nb > MAX_BATCH_BYTES or work_b + nw > MAX_BATCH_BYTES):
            out.append(cur)
            cur, bag_b, work_b = [], 0, 0
        cur.append(i)
        bag_b += nb
        work_b += nw
    if cur:
        out.append(cur)
    return out


def _bank_batches(loader, device, args, entries, discard):
    """Per chunk of the split: (one scored light batch per entry of the bank set, device labels, label list)."""
    X, sizes, x_starts, labels = _collect(loader, device, args)
    bank_set = engine.BankSet(entries, X.dtype, device)
    for ids in _chunks_banks(sizes, X.size(1), X.element_size(), bank_set.n_banks, bank_set.C):
        parent = _sub_batch(X, sizes, x_starts, ids, bank_set.C, bank_set.Ce[0], args.topj, args.topk, discard)
        views = parent.scores_banks(bank_set)
        lab_list = [labels[i] for i in ids]
        yield views, torch.tensor(lab_list, dtype=torch.int64).to(device, non_blocking=True), lab_list


def _ext_is_fg(W, We):
    return bool(torch.equal(We[:, :W.size(1)].to(device=W.device, dtype=torch.float32), W.to(torch.float32)))


def zs_evaluation_banks(loader, device, args, banks, pooling_func=topj_pooling):
    """[zs_evaluation(loader, device, args, pooling_func) after set_classifier_bank(*banks[g]) for every g] -- the same
    floats -- from one read of the bags per group of banks (engine.BankSet: banks of one class count, at most 16 columns
    each).  The four fused pooling functions; the module's bank globals are not touched."""
    banks = _bank_checks("zs_evaluation_banks", loader, banks)
    assert pooling_func in _ZS_KINDS, "zs_evaluation_banks: only the four fused pooling functions (others: zs_evaluation per bank)"
    kind = _ZS_KINDS[pooling_func]
    entries = [(W, We, kind == "bottomk") for W, We in banks]        # (zs_evaluation's own image for this function)
    acc = _Chunks(range(len(banks)))
    with _every_slide_once(loader, restore="attr") as real_len:
        for views, lab, lab_list in _bank_batches(loader, device, args, entries, []):
            for g, v in enumerate(views):
                acc.parts[g].append(_zs_step(v, kind, lab, args.topk))
            acc.labels.extend(lab_list)
    return [acc.metrics(g, loader, real_len, args) for g in acc.parts]


def zs_evaluation_sweep_banks(loader, device, args, banks, topks, pooling_funcs=ZS_POOLING_FUNCS):
    """[zs_evaluation_sweep(loader, device, args, topks, pooling_funcs) under banks[g] for every g] -- the same floats --
    from one read of the bags per group of banks.  For bottomk_irrel_classifier_pooling under a bank whose
    W_ext[:, :C] is not W, the fg_from_ext image is one more entry of the set, not a pass of its own."""
    topks = _sweep_checks("zs_evaluation_sweep_banks", loader, topks)
    banks = _bank_checks("zs_evaluation_sweep_banks", loader, banks)
    funcs = _zs_funcs("zs_evaluation_sweep_banks", pooling_funcs)
    entries, jobs = [], []                                       # jobs: (entry, bank, its functions)
    for g, (W, We) in enumerate(banks):
        own_ext = [f for f in funcs if _ZS_KINDS[f] == "bottomk" and not _ext_is_fg(W, We)]
        shared = [f for f in funcs if f not in own_ext]
        for from_ext, fs in ((False, shared), (True, own_ext)):
            if fs:
                jobs.append((len(entries), g, fs))
                entries.append((W, We, from_ext))
    acc = _Chunks([(g, f) for g in range(len(banks)) for f in funcs], slabs=True)
    with _every_slide_once(loader, restore="attr") as real_len:
        for views, lab, lab_list in _bank_batches(loader, device, args, entries, []):
            for e, g, fs in jobs:
                for f in fs:
                    acc.parts[(g, f)].append(_zs_slabs(views[e], _ZS_KINDS[f], topks, lab))
            acc.labels.extend(lab_list)
    return [_zs_cells(acc, funcs, topks, loader, real_len, args, of=lambda f, g=g: (g, f)) for g in range(len(banks))]


def _bank_models(who, models, n_banks):
    """One model for all banks, or one per bank (checkpoints trained under their own banks) -> a list of n_banks."""
    if isinstance(models, nn.Module):
        models = [models]
    models = list(models)
    assert len(models) in (1, n_banks), f"{who}: one model, or one per bank ({n_banks}); got {len(models)}"
    models = models * n_banks if len(models) == 1 else models
    for m in models:
        if m.training:
            m.eval()
    return models


def evaluation_banks(models, loader, device, args, banks):
    """[evaluation(models[g], loader, device, args) under banks[g] for every g] -- the same floats -- from one read of the
    bags per group of banks.  `models`: one model, or one per bank."""
    banks = _bank_checks("evaluation_banks", loader, banks)
    models = _bank_models("evaluation_banks", models, len(banks))
    acc = _Chunks(range(len(banks)))
    with _every_slide_once(loader) as real_len:
        metas = [MetaState(m) for m in models]
        use = engine.eval_use_bits(args.discard_classifiers)
        for views, lab, lab_list in _bank_batches(loader, device, args, [(W, We, False) for W, We in banks],
                                                  args.discard_classifiers):
            for g, v in enumerate(views):
                acc.parts[g].append(_eval_step(v, metas[g], lab, use))
            acc.labels.extend(lab_list)
    return [acc.metrics(g, loader, real_len, args) for g in acc.parts]


def evaluation_sweep_banks(models, loader, device, args, banks, topjs, topks, discard_sets=None):
    """[evaluation_sweep(models[g], loader, device, args, topjs, topks, discard_sets) under banks[g] for every g] -- the
    same floats: per bank, once its statistics exist, evaluation_sweep's own loop."""
    topks = _sweep_checks("evaluation_sweep_banks", loader, topks)
    banks = _bank_checks("evaluation_sweep_banks", loader, banks)
    models = _bank_models("evaluation_sweep_banks", models, len(banks))
    configs = _sweep_axes("evaluation_sweep_banks", args, topjs, discard_sets)
    acc = _Chunks([(g,) + c for g in range(len(banks)) for c in configs], slabs=True)
    with _every_slide_once(loader) as real_len:
        metas = [MetaState(m) for m in models]
        for views, lab, lab_list in _bank_batches(loader, device, args, [(W, We, False) for W, We in banks], []):
            for g, v in enumerate(views):
                _sweep_configs(v, metas[g], lab, acc, configs, topks, g=(g,))
            acc.labels.extend(lab_list)
    return [_sweep_cells(acc, configs, topks, loader, real_len, args, g=(g,)) for g in range(len(banks))]


# plans of evaluation_runs, least recently used first.  A caller that evaluates one fixed set every epoch and a varying
# subset of another (run_moc.main_runs: all train + validation splits, then the test splits of the runs that improved)
# keeps its fixed plan for good: it is used between any two subset plans, so it is never the least recently used.  A new
# plan is built AFTER the oldest ones are dropped, so its work arrays come out of the blocks those gave back.
_eval_run_plans = {}
EVAL_RUN_PLANS = 3


def pack_splits(loaders):
    """Pack resident splits side by side now (what evaluation_runs does on its first call with them): a caller that will
    evaluate varying subsets of them (the test splits of the runs that improved) packs all of them once."""
    assert all(isinstance(ld, ResidentBags) for ld in loaders), "pack_splits: resident splits only"
    _pack_loaders(list(loaders))


def _pack_loaders(loaders):
    """The resident arrays of the distinct splits side by side in ONE array (as runs.TrainRuns lays out its runs): a one-time
    copy, after which every split's `X` is a view of the packed array (its own allocation is released; the split's plans,
    which held the old array, are dropped).  Splits that share an array already (the same slides loaded once) stay shared.
    -> (X, first row of every loader's split in X)."""
    distinct = {}
    for ld in loaders:
        distinct.setdefault((ld.X.data_ptr(), ld.X.size(0)), ld.X)
    views = list(distinct.values())
    base = views[0]._base if views[0]._base is not None else views[0]
    packed = all((v._base if v._base is not None else v) is base for v in views) and base.dim() == 2 and base.is_contiguous()
    if not packed:
        base = torch.cat(views, 0) if len(views) > 1 else views[0]
        row0 = {}
        o = 0
        for key, v in distinct.items():
            row0[key] = o
            o += v.size(0)
        keys = {id(ld): (ld, (ld.X.data_ptr(), ld.X.size(0))) for ld in loaders}      # (a split may be named twice)
        for ld, key in keys.values():
            if len(views) > 1:
                ld.X = base[row0[key]:row0[key] + key[1]]
                ld._plans.clear()
                ld._stats_caches.clear()
        del views, distinct
    rb = base.size(1) * base.element_size()
    return base, [(ld.X.data_ptr() - base.data_ptr()) // rb for ld in loaders]


def _eval_runs_plan(loaders, model_of_run, device, args):
    """Batches over the visits of ALL loaders (an unmasked pass over every split, run after run), chunked by slides under
    MAX_BATCH_BYTES: per chunk (batch, device labels, device int32 model of each slide relative to its group's first model,
    [(first model, models, first slide, slides)] per group of at most sixteen models)."""
    discard = tuple(sorted(args.discard_classifiers or ()))
    X, row0 = _pack_loaders(loaders)                      # (first: packing moves the splits' arrays, which the key names)
    key = (tuple(id(ld) for ld in loaders), tuple(ld.X.data_ptr() for ld in loaders), tuple(len(ld) for ld in loaders),
           tuple(model_of_run), args.n_classes, args.topj, args.topk, discard, MAX_BATCH_BYTES,
           id(zeroshot_weights), id(zeroshot_weights_ext))
    plan = _eval_run_plans.pop(key, None)
    if plan is not None:
        _eval_run_plans[key] = plan                       # (most recently used: last)
        return plan
    while len(_eval_run_plans) >= EVAL_RUN_PLANS:         # (a plan owns the work arrays of all its rows)
        del _eval_run_plans[next(iter(_eval_run_plans))]
    bank = _bank_for(X, device)
    assert bank.C == args.n_classes
    sizes, starts, labels, run_of = [], [], [], []
    for r, ld in enumerate(loaders):
        for k in ld.visit_order():
            sizes.append(ld.sizes[k])
            starts.append(row0[r] + ld.starts[k])
            labels.append(ld.labels[k])
            run_of.append(r)
    chunks = []
    for ids in _chunks(sizes, X.size(1), X.element_size()):
        batch = SlideBatch(X, [sizes[i] for i in ids], bank.C, bank.Ce, args.topj, args.topk, list(discard),
                           x_starts=[starts[i] for i in ids])
        batch.eval_only = True                            # (no H1 / gates: 272 of ~350 work-array bytes per row)
        lab = torch.tensor([labels[i] for i in ids], dtype=torch.int64).to(device)
        groups, rel = [], []
        for j, i in enumerate(ids):                       # (consecutive slides whose models lie in one block of sixteen)
            mi = model_of_run[run_of[i]]
            g0 = mi // 16 * 16
            if not groups or groups[-1][0] != g0:
                groups.append([g0, 0, j, 0])
            groups[-1][1] = max(groups[-1][1], mi - g0 + 1)
            groups[-1][3] += 1
            rel.append(mi - g0)
        chunks.append((batch, lab, torch.tensor(rel, dtype=torch.int32).to(device), [tuple(g) for g in groups]))
    plan = _eval_run_plans[key] = {"bank": bank, "chunks": chunks, "labels": labels, "run_of": run_of, "keep": list(loaders)}
    return plan


def evaluation_runs(models, loaders, device, args):
    """`[evaluation(models[r], loaders[r], device, args) for r in range(R)]` in ONE pass: one batch of visits over all
    loaders' slides, phase A once, one forward in which every slide is scored by its run's meta-learner
    (moc_meta_forward_by_slide), one pooling launch, one device-to-host copy -- per chunk of MAX_BATCH_BYTES of bag rows,
    which may hold slides of several runs -- then the metrics per run on that run's rows.  Entry r equals evaluation() of run
    r exactly (the same floats).  A model may be named more than once (its train and its validation split in one call).
    The models' parameters are read where they are when they already lie in one arena (after
    train_runs), from a scratch copy otherwise (engine.ModelArena.of_models).
    Refused (an AssertionError; evaluate such runs one by one): loaders that are not ResidentBags, `loader_seed_draw`
    splits, splits of different storage type or width, models of different width.  The resident arrays of distinct splits
    are packed side by side on the first call (a one-time copy; the splits' `X` become views of the packed array)."""
    R = len(models)
    assert R >= 1 and len(loaders) == R, "evaluation_runs: one loader per model"
    assert all(isinstance(ld, ResidentBags) for ld in loaders), "evaluation_runs: resident splits only (main_moc.ResidentBags)"
    assert not any(ld.loader_seed_draw for ld in loaders), "evaluation_runs: loader_seed_draw splits are not batched"
    dt, D = loaders[0].X.dtype, loaders[0].X.size(1)
    assert all(ld.X.dtype == dt and ld.X.size(1) == D for ld in loaders), "evaluation_runs: one storage type and width"
    for m in models:
        if m.training:
            m.eval()
    with torch.no_grad():
        uniq = {}
        for m in models:
            uniq.setdefault(id(m), (len(uniq), m))
        arena = engine.ModelArena.of_models([m for _, m in uniq.values()])
        model_of_run = [uniq[id(m)][0] for m in models]
        assert arena.D == D, "evaluation_runs: the models' width is not the bags'"
    acc = _Chunks()
    with _every_slide_once(*loaders):                # (a split named twice ends where it began: restored last first)
        plan = _eval_runs_plan(loaders, model_of_run, device, args)
        use = engine.eval_use_bits(args.discard_classifiers)
        for batch, lab, rel, groups in plan["chunks"]:
            batch.phase_a(plan["bank"], for_eval=True)
            for g0, gm, s0, sn in groups:
                engine.meta_forward_by_slide(batch, arena, g0, gm, rel, s0, sn, use)
            engine.pool_loss(batch, lab, 0, batch.n_slides)
            acc.parts[None].append(_host_rows(batch))
    acc.labels = plan["labels"]
    run_of = torch.tensor(plan["run_of"])
    evaluation_runs.last_pooled = []
    res = []
    for r, ld in enumerate(loaders):
        pooled, labels, losses = acc.rows(of=(run_of == r).nonzero().flatten())
        evaluation_runs.last_pooled.append(pooled)
        res.append(_metrics(pooled, labels, losses, len(ld.dataset), ld.dataset.real_len(), args))
    return res


def ablation_evaluation(loader, device, args):
    """main_moc.py:523-582, args.ablation_study in {avg, sum, max}."""
    with _every_slide_once(loader) as real_len:
        pooled, labels, losses = _eval_pass(loader, device, args, "ablation")
    return _metrics(pooled, labels, losses, len(loader.dataset), real_len, args)
