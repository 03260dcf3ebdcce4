"""Several independent training runs in ONE process, stepped in lockstep (include/moc_hip.h: moc_train_steps_runs).

The reference trains folds x shots of the same loop as separate processes -- `scripts/moc_train.sh:11-31` starts one
`python main_moc.py` per (fold, shot) and packs five of them onto a GPU.  One run is a chain of dependent meta-steps
(main_moc.py:380-410) that leaves most of an MI355X idle; here R runs share every launch: one forward and one step launch
per meta-step serve all of them (grid.y / grid.z = run), and phase A (mask -> scores -> selectors -> union, parameter free)
runs over all R x n slides in the same four launches, one pass ahead on a side stream.

Every run stays the exact recurrence of `main_moc.train`: its own slides in loader order, its own parameters and Adam
state, its own stream of row masks -- `torch.rand(N) > 0.5` per slide drawn from the run's OWN CPU generator (the
reference's runs are separate processes, each with its own default generator).  Per run the result is bit-identical to
training it alone with `main_moc.train` from the same generator state (tests/test_gpu_runs.py).

What the runs share: the classifier bank, the hyper-parameters of Adam (unless `per_run_adam`: then every run steps with its
own optimizer's lr / betas / eps / weight_decay, still in one chain -- DESIGN.md section 9i), storage type and width.  topj / topk /
discard_classifiers are common when `args` is one namespace and per run when it is a list of R of them (a hyper-parameter
grid: DESIGN.md section 9h).  The models' parameter tensors and the optimizers' moments are re-seated as views into one arena per kind
(state_dict() / load_state_dict() keep working; the tensors' values are preserved).

Runs need NOT be alike in the number of visits per pass or in the Adam steps already taken (a shots x folds grid:
`scripts/moc_train.sh` trains 1, 2, 4, 8 and 16 shots).  They are grouped by (visits per pass, step count) -- `group_runs`
-- and every group is one lockstep chain with its own moc_meta_t copy (so its own `step`) on a stream of its own, as the
chains of more than eight like runs already were; a chain ends its pass when its runs have made their visits.  The step
kernels are the same.  Phase A still covers all runs' slides of a pass in one go, and every run still draws its masks
from its private generator in its own loader order.

A hyper-parameter grid trains the configurations of one (fold, shot, seed) on the same bags, and from equal generator states
they draw the same masks: the kept-row lists, the score pass and the row statistics -- everything in front of moc_select --
depend on none of topj / topk / discard_classifiers.  Runs whose split is the same object and whose generators hold the same
state form a MASK GROUP per pass (`mask_groups`): its first run, the leader, draws and is scored; the others' slots are
filled by moc_stats_share, and the selection runs once per distinct (topj, discard) over that configuration's slides.
MOC_RUNS_SHARE=0 makes every run its own leader.

A BANK GRID (`banks` / `bank_of_run`: DESIGN.md section 9l) trains the runs of one (fold, seed) under several narrow prompt
banks.  They draw the same masks too, but a bank's statistics are its own: the followers receive the kept-row lists alone
(moc_kept_share) and ONE moc_scores_banks launch per leader block and pass of the bank set reads the leader's rows and writes
bank g's statistics straight into the slots of the run that trains under bank g -- the per-bank pointers of the launch are
the batch's own arrays advanced by the distance between the two runs' slots (`bank_score_plan`).
MOC_RUNS_BANKS_FUSED=0 scores every (mask group, bank) with a moc_scores launch of its own instead: the same bits.
"""
from __future__ import annotations

import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import torch

from . import engine
from ._lib import MocAdamHp, MocBankSet, MocRuns, check, lib, ptr
from .engine import HIDDEN, MetaState, SlideBatch

MAX_RUNS = 32           # runs of one TrainRuns (five shots x five folds and some); one moc_train_steps_runs call: 16
MAX_CHAIN = 16          # runs one moc_train_steps_runs call serves (MOC_MAX_RUNS of the library)


def group_runs(keys, cap=8):
    """Lockstep chains for runs whose passes are not alike.  `keys[r]`: what the runs of a chain must share (the number of
    visits per pass, or a tuple with the Adam step count too).  Runs with equal keys form a group, in order of first
    appearance, the runs inside it in their given order; a group of more than `cap` runs is cut into chains of at most `cap`
    (`cap` <= 16, what one moc_train_steps_runs call serves; measured best: eight).  -> list of lists of run indices: every
    run in exactly one chain.  Pure."""
    cap = int(cap)
    assert 1 <= cap <= MAX_CHAIN, f"group_runs: 1 .. {MAX_CHAIN} runs per chain"
    by_key = {}
    for r, k in enumerate(keys):
        by_key.setdefault(k, []).append(r)
    chains = []
    for rs in by_key.values():
        n_chains = (len(rs) + cap - 1) // cap
        per = (len(rs) + n_chains - 1) // n_chains           # (even chains: nine runs are 5 + 4, not 8 + 1)
        chains += [rs[i:i + per] for i in range(0, len(rs), per)]
    return chains


def mask_groups(keys):
    """Leader of every run for one pass' draw.  `keys[r]`: (id of the run's split, bytes of its generator's state) -- or None
    for a run that takes no part.  Runs with equal keys form a group whose first member leads; -> list `leader` with
    leader[r] = r for a leader (singletons and None keys included), else the index of the group's first run.  Pure."""
    first, leader = {}, []
    for r, k in enumerate(keys):
        leader.append(r if k is None else first.setdefault(k, r))
    return leader


def adam_hp(group):
    """An optimizer param group's Adam hyper-parameters as (lr, beta1, beta2, eps, weight_decay), Python floats."""
    b1, b2 = group["betas"]
    return (float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]))


def hp_records(hps):
    """[(lr, beta1, beta2, eps, weight_decay)] -> the host array of moc_adam_hp_t that moc_train_steps_runs_hp reads."""
    arr = (MocAdamHp * len(hps))()
    for rec, hp in zip(arr, hps):
        rec.lr, rec.beta1, rec.beta2, rec.eps, rec.weight_decay = hp
    return arr


def steps_runs_hp(batch_c, meta_c, runs_c, ws_c, labels_ptr, slide0, n, use_bits, records, stream):
    """moc_train_steps_runs_hp; `records`: hp_records(...) of runs_c.n_runs runs, or None.  A refusal -- the library launches
    nothing then -- is a RuntimeError with the library's text."""
    rc = lib().moc_train_steps_runs_hp(C.byref(batch_c), C.byref(meta_c), C.byref(runs_c), C.byref(ws_c), labels_ptr,
                                       slide0, n, use_bits, records, stream)
    if rc != 0:
        raise RuntimeError(f"moc_train_steps_runs_hp failed (code {rc}): {lib().moc_last_error().decode(errors='replace')}")
    return rc


def consecutive_blocks(items):
    """[a, a+1, a+2, b, b+1] -> [(a, 3), (b, 2)]: blocks of consecutive integers, in the given order.  Pure."""
    out = []
    for v in items:
        if out and v == out[-1][0] + out[-1][1]:
            out[-1] = (out[-1][0], out[-1][1] + 1)
        else:
            out.append((v, 1))
    return out


def bank_heads(leader, bank_of_run):
    """{(mask-group leader, bank): the first run of that group that trains under that bank} -- the run whose slots the score
    pass writes; the group's later runs under the same bank are filled from it (moc_stats_share).  Pure."""
    head = {}
    for r, (l, g) in enumerate(zip(leader, bank_of_run)):
        head.setdefault((l, g), r)
    return head


def bank_score_plan(leader, bank_of_run, run_slide0, run_n, row_off_host, passes):
    """The moc_scores_banks launches of one draw.  leader[r]: the mask-group leader of run r (mask_groups); bank_of_run[r]:
    its bank; run_slide0 / run_n: first slide and slides of every run in the batch; row_off_host: first slot of every slide
    (n_slides + 1 entries); passes: [(first bank, banks)] of the bank set (engine.plan_bank_passes).
    -> [(leader slide0, n, first bank of the launch, [(bank, delta slots | None), ...])]: the launch reads slides
    [slide0, slide0 + n) -- a block of consecutive leader runs -- under the consecutive banks listed, and bank g's statistics
    of the slot row_off[b] + i land at slot row_off[b] + i + delta: the slots of the group's first run under bank g
    (`bank_heads`).  None: no run of the block trains under that bank (its statistics go to scratch); a pass is trimmed to
    the banks between its first and last bank with a run, and dropped when it has none.  Consecutive leaders share a launch
    when their deltas agree bank for bank (runs ordered bank-major: always).
    delta is ONE number per (leader, bank) because both runs visit the same slides in the same order: asserted here slide
    by slide.  Pure: host integers only."""
    R = len(leader)
    assert len(bank_of_run) == R and len(run_slide0) == R and len(run_n) == R
    per_leader = {}
    for (l, g), h in bank_heads(leader, bank_of_run).items():
        assert leader[l] == l and h >= l, "bank_score_plan: a leader is the first run of its group"
        assert run_n[h] == run_n[l], f"bank_score_plan: runs {l} and {h} share masks but not the number of visits"
        sl, sh = run_slide0[l], run_slide0[h]
        d = row_off_host[sh] - row_off_host[sl]
        for k in range(run_n[l] + 1):
            assert row_off_host[sh + k] - row_off_host[sl + k] == d, \
                f"bank_score_plan: runs {l} and {h} do not visit slides of the same sizes in the same order (visit {k})"
        per_leader.setdefault(l, {})[g] = int(d)
    blocks = []                                              # [[leader runs], {bank: delta}]
    for l in sorted(per_leader):
        if blocks and blocks[-1][0][-1] == l - 1 and blocks[-1][1] == per_leader[l]:
            blocks[-1][0].append(l)
        else:
            blocks.append([[l], per_leader[l]])
    plan = []
    for runs_, deltas in blocks:
        s0, n = run_slide0[runs_[0]], sum(run_n[r] for r in runs_)
        for g0, ng in passes:
            present = [g for g in range(g0, g0 + ng) if g in deltas]
            if present:
                plan.append((s0, n, present[0], [(g, deltas.get(g)) for g in range(present[0], present[-1] + 1)]))
    return plan


class TrainRuns:
    """R (model, optimizer, resident train split) triples trained in lockstep.  `generators`: one CPU torch.Generator
    per run -- the run's mask stream (default: fresh generators seeded from the default generator, in run order).
    `banks`: [(W [D, C], W_ext [D, Ce]), ...] of one C, every Ce <= 16, and `bank_of_run[r]`: the bank run r trains under (a
    bank grid; the module's classifier bank is neither read nor changed).  Default: every run under the module's bank."""

    def __init__(self, models, optimizers, splits, device, args, generators=None, per_run_adam=False, banks=None, bank_of_run=None):
        from . import main_moc as M
        # per_run_adam: every run steps with its OWN optimizer's lr / betas / eps / weight_decay (moc_train_steps_runs_hp) --
        # the cells of an lr x weight-decay grid stay in one lockstep chain; default: the runs must share them
        self.per_run_adam = bool(per_run_adam)
        R = len(models)
        assert 1 <= R <= MAX_RUNS and len(optimizers) == R and len(splits) == R, f"1 .. {MAX_RUNS} runs"
        per_run = isinstance(args, (list, tuple))
        args_list = list(args) if per_run else [args] * R
        assert len(args_list) == R, "train_runs: one namespace, or one per run"
        args = args_list[0]
        assert all(a.n_classes == args.n_classes for a in args_list), "train_runs: the runs share the classifier bank"
        # run r's (topj, topk, discard_bits); everything else is common
        self.cfg = [(int(a.topj), int(a.topk), engine._lib.discard_bits(a.discard_classifiers)) for a in args_list]
        self.run_use = [engine.train_use_bits(a.discard_classifiers) for a in args_list]
        self.share = os.environ.get("MOC_RUNS_SHARE", "1") != "0"
        assert all(isinstance(sp, M.ResidentBags) for sp in splits), "train_runs: resident splits (main_moc.ResidentBags)"
        self.R, self.models, self.optimizers, self.splits, self.device = R, list(models), list(optimizers), list(splits), device
        self.run_n = [len(sp) for sp in splits]               # visits per pass of each run
        self.n = self.run_n[0] if len(set(self.run_n)) == 1 else None      # (the common number, when there is one)
        self.run_slide0 = [sum(self.run_n[:r]) for r in range(R)]         # first slide of each run in the batches
        dt, D = splits[0].X.dtype, splits[0].X.size(1)
        assert all(sp.X.dtype == dt and sp.X.size(1) == D for sp in splits), "train_runs: one storage type and width"
        assert not any(sp.loader_seed_draw for sp in splits), "train_runs: loader_seed_draw splits are not batched"
        if banks is not None:                                # refused before anything is allocated
            banks = [tuple(b) for b in banks]
            assert banks and all(len(b) == 2 and b[0].dim() == 2 and b[1].dim() == 2 for b in banks), "train_runs: banks = [(W, W_ext), ...]"
            assert bank_of_run is not None and len(bank_of_run) == R and all(0 <= int(g) < len(banks) for g in bank_of_run), \
                "train_runs: bank_of_run names one of the banks for every run"
            assert all(b[0].size(1) == args.n_classes for b in banks), \
                f"train_runs: banks of different C do not share a pass (n_classes = {args.n_classes}; got {[int(b[0].size(1)) for b in banks]})"
            assert all(b[1].size(1) <= engine.BANK_SET_MAX_CE for b in banks), \
                f"train_runs: a bank wider than {engine.BANK_SET_MAX_CE} columns ({[int(b[1].size(1)) for b in banks]}) trains in a run of its own"
            assert all(b[0].size(0) == D and b[1].size(0) == D for b in banks), "train_runs: the banks are for another width"
            assert os.environ.get("MOC_CACHE_SCORES", "0") != "1" and not any(sp.cache_scores for sp in splits), \
                "train_runs: a score cache belongs to one bank (cache_scores splits and banks do not combine)"
        else:
            assert bank_of_run is None, "train_runs: bank_of_run without banks"
        self.bank_of_run = None if banks is None else [int(g) for g in bank_of_run]
        self.banks_fused = os.environ.get("MOC_RUNS_BANKS_FUSED", "1") != "0"
        if generators is None:
            generators = []
            for _ in range(R):
                g = torch.Generator()
                g.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
                generators.append(g)
        assert len(generators) == R and all(g is not torch.default_generator for g in generators), \
            "train_runs: one private CPU generator per run (the masks of a pass are drawn a pass ahead)"
        self.generators = list(generators)
        # ---- all runs' bags in one packed array (a one-time copy), the visits of run r at slides r * n ...
        # (splits that are the same object -- the configurations of one fold -- are placed once: their visits name the same rows)
        uniq, split_row0 = [], {}
        for sp in splits:
            if id(sp) not in split_row0:
                split_row0[id(sp)] = sum(u.X.size(0) for u in uniq)
                uniq.append(sp)
        self.X = torch.cat([sp.X for sp in uniq], 0) if len(uniq) > 1 else uniq[0].X
        sizes, starts, labels = [], [], []
        self.run_rows = []                                   # (first flag, flags) of each run's pass
        for sp in splits:
            order = sp.visit_order()
            rows, row0 = 0, split_row0[id(sp)]
            for k in order:
                sizes.append(sp.sizes[k])
                starts.append(row0 + sp.starts[k])
                labels.append(sp.labels[k])
                rows += sp.sizes[k]
            self.run_rows.append((sum(s_ for s_ in sizes) - rows, rows))
        self.bank_set = self.banks_alone = self._bank_scratch = None
        if banks is None:
            bank = M._bank_for(self.X, device)
        else:
            # one image for all banks; the batch struct's Ce is read by the score pass alone (every launch of one carries its
            # own bank's), so the batch keeps the largest
            bank = self.bank_set = engine.BankSet(banks, self.X.dtype, device)
            if not self.banks_fused:
                self.banks_alone = [engine.Bank(W_, We_, self.X.dtype, device) for W_, We_ in banks]
        assert bank.C == args.n_classes
        batch_Ce = bank.Ce if banks is None else max(bank.Ce)
        self.bank, self.args, self.args_list = bank, args, args_list
        T = sum(sizes)
        # (the batch's own topj / discard: run 0's; its topk: the largest, which sizes the work arrays -- every launch of a
        # grid takes a copy of the struct carrying its configuration's values)
        self.batches = [SlideBatch(self.X, sizes, bank.C, batch_Ce, args.topj, max(k for _, k, _ in self.cfg), args.discard_classifiers,
                                   mask=torch.ones(T, dtype=torch.uint8), x_starts=starts) for _ in range(2)]
        # (round 4 measurements, profiles/NOTES.md: the meta-steps crawl while a score pass streams beside them whether or not
        # it leaves them compute units, so phase A here runs at full width; MOC_RUNS_RESERVE_CUS brings the reservation back)
        self.reserve = int(os.environ.get("MOC_RUNS_RESERVE_CUS", "0"))
        self.lookahead = os.environ.get("MOC_RUNS_LOOKAHEAD", "0") != "0"
        self.upload_flags = os.environ.get("MOC_RUNS_UPLOAD_FLAGS", "0") != "0"    # (measured: no gain from the copy)
        if banks is None and bank.Ce <= 16 and self.reserve > 0:
            for b in self.batches:
                b.reserve_cus(self.reserve)
        if os.environ.get("MOC_CACHE_SCORES", "0") == "1" or all(sp.cache_scores for sp in splits):
            # opt-in (main_moc.ResidentBags cache_scores): the statistics of every row once, then no score pass per epoch
            all_sizes, all_starts, r0_ = [], [], 0
            for sp in uniq:
                all_sizes += sp.sizes
                all_starts += [r0_ + st for st in sp.starts[:-1]]
                r0_ += sp.X.size(0)
            cache = engine.build_stats_cache(self.X, all_sizes, all_starts, bank, args.topj, args.topk)
            for b in self.batches:
                b.stats_cache = cache
        self.labels = torch.tensor(labels, dtype=torch.int64).to(device)
        self.flags = [torch.empty(T, dtype=torch.uint8).pin_memory() for _ in range(3)]
        self.flag_busy = [None, None, None]
        self.side = torch.cuda.Stream(device=device)
        self.X.record_stream(self.side)
        for b in self.batches:
            for t in (b.kept, b.n_kept, b.stats, b.sel_flag, b.sel_idx, b.sel_row, b.n_sel, b.cand, b.row_off, b.x_off, b.ticket):
                if t is not None:
                    t.record_stream(self.side)
        self.pool = ThreadPoolExecutor(R)
        # ---- parameters, moments and operand images: one arena per kind, run r at r * stride
        H = HIDDEN
        n_par = H * D + H + 4 * H + 4
        self.par_stride = (n_par + 63) // 64 * 64
        f32 = dict(dtype=torch.float32, device=device)
        self.P, self.Mo, self.Vo = (torch.zeros((R, self.par_stride), **f32) for _ in range(3))
        img_b = max(lib().moc_w1_image_bytes(D, engine._lib.MOC_BF16), lib().moc_w1_image_bytes(D, engine._lib.MOC_F32))
        self.img_stride = (img_b + 255) // 256 * 256
        self.images = torch.empty((R, self.img_stride), dtype=torch.uint8, device=device)
        self.W2_alt = torch.empty((R, 4, H), **f32)
        offs = (0, H * D, H * D + H, H * D + H + 4 * H)
        shapes = ((H, D), (H,), (4, H), (4,))
        group0, run_steps, self._adam_groups = None, [], []
        for r, (model, opt) in enumerate(zip(self.models, self.optimizers)):
            meta = MetaState(model, opt)                      # (validates the pair; creates Adam's state if it is new)
            g = meta._group
            hp = (float(g["lr"]), tuple(float(b) for b in g["betas"]), float(g["eps"]), float(g["weight_decay"]))
            group0 = group0 or hp
            assert self.per_run_adam or hp == group0, "train_runs: the runs must share Adam's hyper-parameters"
            self._adam_groups.append(g)
            run_steps.append(int(meta.c.step))
            for p, o, shp in zip(meta.params, offs, shapes):
                cnt = p.numel()
                for arena, src in ((self.P, p.data), (self.Mo, opt.state[p]["exp_avg"]), (self.Vo, opt.state[p]["exp_avg_sq"])):
                    arena[r, o:o + cnt].copy_(src.reshape(-1))
                p.data = self.P[r, o:o + cnt].view(shp)
                opt.state[p]["exp_avg"] = self.Mo[r, o:o + cnt].view(shp)
                opt.state[p]["exp_avg_sq"] = self.Vo[r, o:o + cnt].view(shp)
        self.meta = MetaState(self.models[0], self.optimizers[0])            # run 0's tensors: the base of every arena
        self.meta.c.W1_image = ptr(self.images)
        self.turn, self.ahead, self.steps_done = 0, None, [None, None]
        self.last = None
        # mask groups of the pass in each work-array set; `last_phase_a`: slides / scored_slides / shared_slides of the most
        # recent draw (the look-ahead draws the NEXT pass' masks at the end of a pass), `trained_phase_a`: of the pass whose
        # steps were issued last
        self.pass_info, self.last_phase_a, self.trained_phase_a, self._lead_dev = [None, None], None, None, {}
        # The runs step in lockstep inside a GROUP; several groups are independent chains on streams of their own, whose
        # latency-bound kernels interleave on the device (one group: every launch serves all R runs)
        # Shapes outside the tile-record step (wide banks): moc_train_steps_runs takes a group's runs one after the other,
        # so every run is a group of its own -- R chains of (forward, top-K, wide step) side by side, each of which keeps
        # a few dozen CUs busy (include/moc_hip.h moc_train_runs_mode)
        # asked per configuration: K <= 16 and C K <= 64 decide the step kernel
        configs = list(dict.fromkeys(self.cfg))
        topks = sorted({k for _, k, _ in configs})
        for b in self.batches:
            self._workspace_slabs(b, topks)
        cfg_mode = {}
        for c_ in configs:
            cfg_mode[c_] = int(lib().moc_train_runs_mode(C.byref(self._struct(self.batches[0].c, c_)), C.byref(self.batches[0].meta_ws()[1])))
            assert cfg_mode[c_] != 0, "train_runs: this shape takes the three-launch step, whose scratch is one per batch -- train the runs one by one"
        self.run_mode = [cfg_mode[c_] for c_ in self.cfg]
        self.mode = max(self.run_mode)
        cap = 8                                               # (measured, lockstep: chains of up to eight runs)
        env_cap = False
        if "MOC_RUNS_GROUPS" in os.environ:
            G = max(1, min(R, int(os.environ["MOC_RUNS_GROUPS"])))
            cap, env_cap = min(MAX_CHAIN, (R + G - 1) // G), True
        # a chain's runs share the visits per pass, the step count and the configuration (one moc_train_steps_runs call has
        # one batch struct and one use_bits), and lie a constant stride apart in the arenas and in the batches: chains are cut
        # where the run indices stop being consecutive
        chains = []
        for chain in group_runs([(n_, st_, c_) for n_, st_, c_ in zip(self.run_n, run_steps, self.cfg)], cap):
            if self.run_mode[chain[0]] == 2 and not env_cap:  # (outside the tile-record step: every run a chain of its own)
                chains += [[r] for r in chain]
            else:
                chains.append(chain)
        self.groups = []
        for chain in chains:
            pieces = [[chain[0]]]
            for r in chain[1:]:
                if r == pieces[-1][-1] + 1:
                    pieces[-1].append(r)
                else:
                    pieces.append([r])
            for piece in pieces:
                r0, n_ = piece[0], self.run_n[piece[0]]
                mc = type(self.meta.c).from_buffer_copy(self.meta.c)
                for name in ("W1", "b1", "W2", "b2", "m_W1", "m_b1", "m_W2", "m_b2", "v_W1", "v_b1", "v_W2", "v_b2"):
                    setattr(mc, name, getattr(self.meta.c, name) + 4 * r0 * self.par_stride)
                mc.W1_image = ptr(self.images) + r0 * self.img_stride
                self.groups.append({"r0": r0, "n": n_, "slide0": self.run_slide0[r0], "meta": mc, "cfg": self.cfg[r0],
                                    "use": self.run_use[r0],
                                    "runs": MocRuns(n_runs=len(piece), slide_stride=n_, par_stride=self.par_stride,
                                                    image_stride=self.img_stride),
                                    "w2alt": ptr(self.W2_alt) + 4 * r0 * 4 * H,
                                    "stream": None if not self.groups else torch.cuda.Stream(device=device)})

    # ---- struct copies: a configuration's values, a slide range
    @staticmethod
    def _struct(c0, cfg):
        """A copy of the batch struct `c0` carrying configuration `cfg` = (topj, topk, discard_bits): what a chain, or a
        selection over that configuration's slides, hands the library."""
        c = type(c0).from_buffer_copy(c0)
        c.topj, c.topk, c.discard_bits = cfg
        return c

    @staticmethod
    def _view(c, slide0, n):
        """Slides [slide0, slide0 + n) of the batch struct `c` as a batch of their own: the per-slide arrays advanced by
        slide0, n_slides = n.  The slot arrays are addressed absolutely through row_off (mask, kept, stats, sel_flag, sel_idx,
        sel_row, cand: every kernel of phase A forms `array + row_off[b]`), so they stay; max_rows may stay the batch's."""
        v = type(c).from_buffer_copy(c)
        v.n_slides = n
        v.row_off = c.row_off + 8 * slide0
        v.row_off_host = c.row_off_host + 8 * slide0
        if c.x_off:
            v.x_off = c.x_off + 8 * slide0
        if c.n_kept:
            v.n_kept = c.n_kept + 4 * slide0
        v.n_sel = c.n_sel + 4 * slide0
        v.n_sel_host = None
        if c.n_sel_mail:                                       # (a per-slide array too: the view's slide 0 is word slide0)
            v.n_sel_mail = c.n_sel_mail + 8 * slide0
        return v

    def _workspace_slabs(self, batch, topks):
        """The step workspace of a grid.  moc_meta_ws_t.topk_idx is indexed [slide, C, topk] with the BATCH's topk as its
        stride: chains of different K, which run side by side on their own streams, would write overlapping regions (slides
        0-2 at K = 10 and slides 3-5 at K = 5), so every K gets a slab of its own, [n_slides, C, K].  Nothing else needs one:
        topk_cnt / pooled / loss / pred are per slide without K; pair_dh / pair_row belong to the three-launch step, which
        moc_train_runs_mode == 0 refuses; the tile records are laid out by (slide, C) alone (moc_tile_ws_bytes)."""
        t, ws = batch.meta_ws()
        batch._topk_slabs = {}
        if topks == [batch.topk]:
            return
        Cc = batch.C
        for K in topks:
            batch._topk_slabs[K] = t["topk_idx"] if K == batch.topk else \
                torch.empty((batch.n_slides, Cc, K), dtype=torch.int32, device=batch.device)
        # the tile records exist when ANY configuration can take the tile-record step (meta_ws decided by the largest K)
        if t["tile_ws"] is None and engine.TILE_RECORDS and Cc <= 16 and any(K <= 16 and Cc * K <= 64 for K in topks):
            nb = lib().moc_tile_ws_bytes(batch.total, batch.n_slides, Cc)
            t["tile_ws"] = torch.empty(nb, dtype=torch.uint8, device=batch.device)
            ws.tile_ws, ws.tile_ws_bytes = ptr(t["tile_ws"]), nb

    def topk_idx(self, r):
        """[n_r, C, K_r] pooled positions of run r's slides in the last pass (its configuration's slab)."""
        batch, K = self.last[0], self.cfg[r][1]
        slab = batch._topk_slabs.get(K, batch.meta_ws()[0]["topk_idx"])
        return slab[self.run_slide0[r]:self.run_slide0[r] + self.run_n[r]]

    # ---- the masks of one pass: every mask group's leader draws, side by side (moc_host_draw_masks releases the GIL)
    def _draw(self, buf):
        """-> (kept rows of the leaders, the largest kept-row count of any slide, leader of every run)."""
        off_c = self.batches[0]._row_off_c
        gens = self.generators
        if self.share:
            leader = mask_groups([(id(sp), g.get_state().numpy().tobytes()) for sp, g in zip(self.splits, gens)])
        else:
            leader = list(range(self.R))

        def one(r):
            g = gens[r]
            st = g.get_state()
            first, rows = self.run_rows[r]
            kept = lib().moc_host_draw_masks(ptr(st), st.numel(), rows, buf.data_ptr() + first)
            if kept < 0:                                       # a generator whose state the replay does not know: torch draws
                m = torch.rand(rows, generator=g) > 0.5
                buf[first:first + rows].copy_(m)
                kept = int(m.sum())
            else:
                g.set_state(st)
            # the run's slides are slides run_slide0[r] ... of the batch: its largest kept-row count, from the same thread
            mk = lib().moc_host_max_kept(buf.data_ptr(), C.c_void_p(C.addressof(off_c) + 8 * self.run_slide0[r]), self.run_n[r])
            return int(kept), int(mk)
        leaders = [r for r in range(self.R) if leader[r] == r]
        res = list(self.pool.map(one, leaders))
        for r in range(self.R):                                # a follower's stream goes on where its leader's does
            if leader[r] != r:
                gens[r].set_state(gens[leader[r]].get_state())
        return sum(k for k, _ in res), max(m for _, m in res), leader

    def _free_flags(self):
        for i, ev in enumerate(self.flag_busy):
            if ev is None or ev.query():
                self.flag_busy[i] = None
                return i
        self.flag_busy[0].synchronize()
        self.flag_busy[0] = None
        return 0

    def _phase_a(self, turn, head_only=False):
        """Masks + phase A of the next pass into work-array set `turn`, on the CURRENT stream (head_only: the flags and the
        kept-row lists only; `_phase_a_tail` does the rest)."""
        i = self._free_flags()
        kept, max_kept, leader = self._draw(self.flags[i])
        batch = self.batches[turn]
        if self.upload_flags:
            # one asynchronous copy of the flags (the compaction kernel reading 4 MB of them in place over PCIe takes as
            # long as the link: 77 us at eight runs), the grids still tightened to the largest kept-row count
            batch.set_mask(self.flags[i], kept)
            batch.c.max_rows = max(1, max_kept)
        else:
            batch.use_host_mask(self.flags[i], kept, max_kept)
        scored = sum(self.run_n[r] for r in range(self.R) if leader[r] == r)
        # one configuration and nobody to share with: the batch's own four launches, as ever
        plain = scored == batch.n_slides and len(set((j, d) for j, _, d in self.cfg)) == 1 and self.bank_set is None
        self.pass_info[turn] = {"leader": leader, "plain": plain,
                                "report": {"slides": batch.n_slides, "scored_slides": scored, "shared_slides": batch.n_slides - scored}}
        if self.bank_set is not None:
            plan = bank_score_plan(leader, self.bank_of_run, self.run_slide0, self.run_n, batch.row_off_host, self.bank_set.passes)
            self.pass_info[turn]["plan"] = plan
            self.pass_info[turn]["report"]["bank_passes"] = len(plan) if self.banks_fused else 0
        self.last_phase_a = self.pass_info[turn]["report"]
        if plain:
            if head_only:
                batch.phase_a_head(self.bank)
            else:
                batch.phase_a(self.bank)
                batch._n_sel_request()                         # (the lockstep launches take all counts or none: the copy)
        else:
            # head: the leaders' kept-row lists (a launch per block of consecutive leader runs)
            bank = self.bank
            assert bank.D == batch.D and bank.C == batch.C and bank.dtype == batch.X.dtype
            assert batch.Ce == (bank.Ce if self.bank_set is None else max(bank.Ce))
            batch._layout(engine.COMPACT_STATS and batch.Ce > 16)
            batch._n_sel_stale()
            for s0, n_ in self._slide_blocks([r for r in range(self.R) if leader[r] == r]):
                check(lib().moc_mask_compact(C.byref(self._view(batch.c, s0, n_)), engine._stream()), "moc_mask_compact")
            if not head_only:
                self._phase_a_tail(turn)
        ev = torch.cuda.Event()
        ev.record(engine.stream_obj())
        self.flag_busy[i] = ev
        return ev

    def _slide_blocks(self, runs):
        """(first slide, slides) of every block of consecutive runs among `runs` (their slides are consecutive too)."""
        return [(self.run_slide0[r0], sum(self.run_n[r0:r0 + k])) for r0, k in consecutive_blocks(runs)]

    def _phase_a_tail(self, turn):
        """The rest of phase A of set `turn`: the leaders' score pass, the share, the selection per configuration."""
        batch, info = self.batches[turn], self.pass_info[turn]
        self.trained_phase_a = info["report"]
        if info["plain"]:
            batch.phase_a_tail(self.bank)
            batch._n_sel_request()
            return
        leader, st = info["leader"], engine._stream()
        if self.bank_set is not None:
            self._score_banks(batch, info, st)
        else:
            for s0, n_ in self._slide_blocks([r for r in range(self.R) if leader[r] == r]):
                v = self._view(batch.c, s0, n_)
                if batch.stats_cache is not None:
                    cache, compact = batch.stats_cache
                    assert compact == bool(batch.c.flags & engine._lib.MOC_STATS_COMPACT) and cache.size(1) == self.X.size(0)
                    check(lib().moc_scores_from_cache(C.byref(v), ptr(cache), cache.size(1), st), "moc_scores_from_cache")
                else:
                    check(lib().moc_scores(C.byref(v), ptr(self.bank.image), st), "moc_scores")
            if any(leader[r] != r for r in range(self.R)):
                # the followers' slots: kept rows, statistics and cleared union flags from their leaders' (moc_stats_share)
                check(lib().moc_stats_share(C.byref(batch.c), ptr(self._leader_of_slide(leader)), 0, batch.n_slides, st), "moc_stats_share")
        batch._n_sel_stale()
        by_sel = {}
        for r, (j, _, d) in enumerate(self.cfg):               # moc_select / moc_gather_candidates read topj and discard_bits only
            by_sel.setdefault((j, d), []).append(r)
        for (j, d), rs in by_sel.items():
            c = self._struct(batch.c, (j, batch.topk, d))
            for s0, n_ in self._slide_blocks(rs):
                v = self._view(c, s0, n_)
                check(lib().moc_select(C.byref(v), st), "moc_select")
                check(lib().moc_gather_candidates(C.byref(v), None, st), "moc_gather_candidates")
        batch._n_sel_request()

    def _leader_of_slide(self, source, tag=None):
        """Device int32 [n_slides] for the share kernels: the slide that slide b copies from -- slide k of run source[r] for slide
        k of run r -- or -1 where source[r] == r.  Kept per (tag, source)."""
        key = (tag, tuple(source))
        lead = self._lead_dev.get(key)
        if lead is None:
            if len(self._lead_dev) > 8:
                self._lead_dev.clear()
            of_slide = []
            for r in range(self.R):
                d = self.run_slide0[source[r]] - self.run_slide0[r]
                of_slide += [-1 if d == 0 else s_ + d for s_ in range(self.run_slide0[r], self.run_slide0[r] + self.run_n[r])]
            lead = self._lead_dev[key] = torch.tensor(of_slide, dtype=torch.int32).to(self.device)
            lead.record_stream(self.side)
        return lead

    def _score_banks(self, batch, info, st):
        """The score pass of a bank grid (behind the leaders' moc_mask_compact): the lists to every follower, then bank g's
        statistics of a mask group into the slots of the group's first run under bank g, then to the group's other runs
        under that bank."""
        leader, bs, R = info["leader"], self.bank_set, self.R
        if any(leader[r] != r for r in range(R)):
            check(lib().moc_kept_share(C.byref(batch.c), ptr(self._leader_of_slide(leader)), 0, batch.n_slides, st), "moc_kept_share")
        heads = bank_heads(leader, self.bank_of_run)
        cb = type(batch.c).from_buffer_copy(batch.c)          # full layout, static walk over the whole chip
        cb.tile_ticket = cb.cu_reserved = None
        cb.flags = 0
        if self.banks_fused:
            T = batch.total
            for s0, n_, g0, entries in info["plan"]:
                S = MocBankSet(n_banks=len(entries), C=bs.C, image=bs.image.data_ptr() + g0 * bs.tile_bytes)
                for i, (g, d) in enumerate(entries):
                    S.Ce[i] = bs.Ce[g]
                    if d is None:                             # nobody in this block trains under bank g
                        if self._bank_scratch is None:
                            self._bank_scratch = (torch.empty((2 * bs.C + 3, T), dtype=torch.float32, device=self.device),
                                                  torch.empty(T, dtype=torch.uint8, device=self.device))
                            for t_ in self._bank_scratch:
                                t_.record_stream(self.side)
                        S.stats[i], S.sel_flag[i] = ptr(self._bank_scratch[0]), ptr(self._bank_scratch[1])
                    else:
                        # the last slot written is the last slot of the run under bank g (bank_score_plan asserts the layout)
                        assert 0 <= d and batch.row_off_host[s0 + n_] + d <= T
                        S.stats[i], S.sel_flag[i] = ptr(batch.stats) + 4 * d, ptr(batch.sel_flag) + d
                check(lib().moc_scores_banks(C.byref(self._view(cb, s0, n_)), C.byref(S), st), "moc_scores_banks")
        else:
            for (_, g), h in heads.items():
                cb.Ce = bs.Ce[g]
                v = self._view(cb, self.run_slide0[h], self.run_n[h])
                check(lib().moc_scores(C.byref(v), ptr(self.banks_alone[g].image), st), "moc_scores")
        source = [heads[(leader[r], self.bank_of_run[r])] for r in range(R)]
        if any(source[r] != r for r in range(R)):             # same masks, same bank: topj / topk / discard / Adam values differ
            check(lib().moc_stats_share(C.byref(batch.c), ptr(self._leader_of_slide(source, "bank")), 0, batch.n_slides, st),
                  "moc_stats_share")

    def train_pass(self):
        """One pass (epoch) of every run: main_moc.train for each of them, in lockstep."""
        for m in self.models:
            if not m.training:
                m.train()
        ahead, self.ahead = self.ahead, None
        if ahead is not None:
            ahead["done"].wait(engine.stream_obj())
            self.turn = ahead["turn"]
            if ahead.get("head_only"):                        # its kept-row lists exist: score pass, selection, candidates now
                self._phase_a_tail(self.turn)
        else:
            self.turn = 1 - self.turn
            self._phase_a(self.turn)
        self.trained_phase_a = self.pass_info[self.turn]["report"]
        batch = self.batches[self.turn]
        t, ws0 = batch.meta_ws()
        batch.publish_n_sel()
        self.meta.refresh()
        for grp in self.groups:                               # the chain's own step count: its runs' optimizers hold it
            steps = {int(self.optimizers[r].state[self.models[r].model[0].weight]["step"])
                     for r in range(grp["r0"], grp["r0"] + grp["runs"].n_runs)}
            assert len(steps) == 1, "train_runs: the runs of a chain no longer agree on the Adam step count"
            grp["step"] = steps.pop()
            if self.per_run_adam:                             # re-read every pass, as MetaState.refresh does: a scheduler's or
                grp["hp"] = hp_records([adam_hp(self._adam_groups[r])    # a user's edit between two passes is seen
                                        for r in range(grp["r0"], grp["r0"] + grp["runs"].n_runs)])
        main = engine.stream_obj()
        ready = None
        if len(self.groups) > 1:
            ready = torch.cuda.Event()
            ready.record(main)                               # phase A of this pass is in front of it on the main stream
        joins = []

        def group_call(grp, raw_stream):
            ws = type(ws0).from_buffer_copy(ws0)
            ws.W2_alt = grp["w2alt"]
            bc = batch.c
            if len(batch._topk_slabs) or grp["cfg"] != (batch.c.topj, batch.c.topk, batch.c.discard_bits):
                # a grid: the chain's own topj / topk / discard_bits, and its K's slab of pooled positions
                bc = self._struct(batch.c, grp["cfg"])
                slab = batch._topk_slabs.get(grp["cfg"][1])
                if slab is not None:
                    ws.topk_idx = ptr(slab)
            mc = grp["meta"]
            mc.lr, mc.beta1, mc.beta2, mc.eps, mc.weight_decay = (self.meta.c.lr, self.meta.c.beta1, self.meta.c.beta2,
                                                                  self.meta.c.eps, self.meta.c.weight_decay)
            mc.step = grp["step"]
            if self.per_run_adam:                             # the records of THIS chain's runs: r0 ... (not run 0 ...)
                return lib().moc_train_steps_runs_hp(C.byref(bc), C.byref(mc), C.byref(grp["runs"]), C.byref(ws), ptr(self.labels),
                                                     grp["slide0"], grp["n"], grp["use"], grp["hp"], raw_stream)
            return lib().moc_train_steps_runs(C.byref(bc), C.byref(mc), C.byref(grp["runs"]), C.byref(ws), ptr(self.labels),
                                              grp["slide0"], grp["n"], grp["use"], raw_stream)
        main_raw = engine._stream()
        raw_of = lambda grp: main_raw if grp["stream"] is None else C.c_void_p(grp["stream"].cuda_stream)
        for grp in self.groups:
            if grp["stream"] is not None:
                grp["stream"].wait_event(ready)
        if self.mode == 2 and len(self.groups) > 1:
            # one chain of three launches per meta-step and run: the host's launch calls are what would hold the chains apart
            # (120 steps x 3 launches x ~4 us per run and pass), so every group's pass is issued from a thread of its own (the
            # library call releases the GIL; the stream is handed over as its raw handle)
            def threaded(grp):
                torch.cuda.set_device(self.device)             # (a new thread's current device is device 0)
                return group_call(grp, raw_of(grp))
            rcs = list(self.pool.map(threaded, self.groups))
        else:
            rcs = [group_call(grp, raw_of(grp)) for grp in self.groups]
        for rc in rcs:
            check(rc, "moc_train_steps_runs_hp" if self.per_run_adam else "moc_train_steps_runs")
        for grp in self.groups:
            if grp["stream"] is not None:
                ev = torch.cuda.Event()
                ev.record(grp["stream"])
                joins.append(ev)
        for ev in joins:
            main.wait_event(ev)
        for opt, n_ in zip(self.optimizers, self.run_n):      # n fused Adam steps in every optimizer's own counters
            for st in opt.state.values():
                if "step" in st:
                    st["step"] += n_
        self.last = (batch, self.labels)
        mark = torch.cuda.Event()
        mark.record(engine.stream_obj())
        self.steps_done[self.turn] = mark
        # The NEXT pass, on the side stream, into the other set (free once the pass before this one has run): its flags and
        # kept-row lists -- the compaction kernel reads the flags over PCIe, 77 us at eight runs, which costs the steps
        # nothing -- or (MOC_RUNS_LOOKAHEAD=1) all of its phase A (measured slower: the steps crawl under a score pass)
        other = 1 - self.turn
        if self.steps_done[other] is not None:
            self.steps_done[other].synchronize()
        with torch.cuda.stream(self.side):
            done = self._phase_a(other, head_only=not self.lookahead)
        self.ahead = {"turn": other, "done": done, "head_only": not self.lookahead}

    def losses(self):
        """[R, n] losses of the last pass (device); runs of different pass lengths: a list of R tensors [n_r]."""
        batch, _ = self.last
        loss = batch.meta_ws()[0]["loss"]
        if self.n is not None:
            return loss.view(self.R, self.n)
        return [loss[s0:s0 + n_] for s0, n_ in zip(self.run_slide0, self.run_n)]
