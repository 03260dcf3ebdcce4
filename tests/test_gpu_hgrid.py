"""A topj x topk x discard grid in one process (moc_amd.runs with a list of namespaces): every run is,
bit for bit, main_moc.train with that run's arguments; the configurations of one split share one mask draw and one score
pass per pass (moc_stats_share fills the followers' slots); chains of different topk keep their pooled positions apart.

Bags: D = 512, three slides per split of 517 / 700 / 1,030 rows (no multiple of 16 or 256) unless a test says otherwise.

Where the generator stands: TrainRuns draws the masks of the NEXT pass at the end of a pass (tests/test_gpu_grid.py), so
after e passes a run's generator is one pass of draws ahead of the default generator after e passes of main_moc.train --
the comparison of the final states accounts for that pass, as test_gpu_grid does, and a draw the caller makes from a run's
generator after pass p lands, in the run's mask stream, behind the masks of pass p + 1: that is where the run alone makes it."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import helpers as H
from moc_amd import synth

pytestmark = pytest.mark.gpu

SIZES = (517, 700, 1030)
CONFIGS = [(50, 5, ()), (100, 10, ()), (100, 10, ("delta_diff",)), (20, 3, ("topk", "bottomk"))]
EPOCHS = 3


@pytest.fixture(scope="module")
def dev(gpu_device):
    return gpu_device


def _bank(C_, D):
    return synth.make_bank(31 + C_, D, C_)


def _split(s, C_, D, dtype):
    W, We = _bank(C_, D)
    bags, labels = synth.make_slide_set(9000 + 37 * s, list(SIZES), D, We, C_)
    return [b.to(dtype) for b in bags], labels


def _rows():
    return sum(SIZES)


def _alone(dev, split, cfg, C_, D, dtype, model_seed, gen_seed, cache=False, extra_draw_after=None):
    """main_moc.train for EPOCHS passes with one run's arguments -> everything the grid must reproduce."""
    from moc_amd import main_moc as M
    W, We = _bank(C_, D)
    M.set_classifier_bank(W.to(dev), We.to(dev))
    bags, labels = _split(split, C_, D, dtype)
    torch.manual_seed(model_seed)
    model = M.senet(D, 4).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
    res = M.ResidentBags(bags, labels, dev, cache_scores=cache)
    args = H.make_args(C_, cfg[0], cfg[1], cfg[2])
    torch.manual_seed(gen_seed)
    losses, idx, cnt = [], None, None
    for e in range(EPOCHS):
        M.train(model, res, opt, dev, args)
        torch.cuda.synchronize()
        t = M.train.last[0].meta_ws()[0]
        losses.append(t["loss"].cpu().clone())
        idx, cnt = t["topk_idx"].cpu().clone(), t["topk_cnt"].cpu().clone()
        if extra_draw_after == e:
            torch.rand(1)
    steps = [int(float(opt.state[p]["step"])) for p in model.parameters()]
    return dict(p=torch.from_numpy(H.flat_params(model)), m=torch.from_numpy(H.flat_state(opt, "exp_avg")),
                v=torch.from_numpy(H.flat_state(opt, "exp_avg_sq")), steps=steps, losses=losses, idx=idx, cnt=cnt,
                rng=torch.get_rng_state().clone())


def _grid(dev, configs, n_splits, C_, D, dtype, cache=False, touch=None, on_pass=None):
    """The same runs through train_runs with a list of namespaces: configurations in the given order, splits inside."""
    from moc_amd import main_moc as M
    W, We = _bank(C_, D)
    M.set_classifier_bank(W.to(dev), We.to(dev))
    shared = []
    for s in range(n_splits):
        bags, labels = _split(s, C_, D, dtype)
        shared.append(M.ResidentBags(bags, labels, dev, cache_scores=cache))
    models, opts, splits, gens, args = [], [], [], [], []
    for ci, cfg in enumerate(configs):
        for s in range(n_splits):
            r = ci * n_splits + s
            torch.manual_seed(100 + r)
            model = M.senet(D, 4).to(dev)
            models.append(model)
            opts.append(torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4))
            splits.append(shared[s])                            # the same OBJECT for every configuration of a split
            g = torch.Generator()
            g.manual_seed(7000 + s)                             # one seed per split
            gens.append(g)
            args.append(H.make_args(C_, cfg[0], cfg[1], cfg[2]))
    losses, reports = [], []
    for e in range(EPOCHS):
        rs = M.train_runs(models, splits, opts, dev, args, generators=gens)
        torch.cuda.synchronize()
        losses.append(rs.losses().cpu().clone())
        reports.append((dict(rs.trained_phase_a), dict(rs.last_phase_a)))
        if on_pass is not None:
            on_pass(e, rs)
        if touch is not None and touch[1] == e:
            torch.rand(1, generator=gens[touch[0]])
    return dict(rs=rs, models=models, opts=opts, gens=gens, losses=losses, reports=reports)


def _same_next_draws(state_a, state_b):
    ga, gb = torch.Generator(), torch.Generator()
    ga.set_state(state_a)
    gb.set_state(state_b)
    return torch.equal(torch.rand(256, generator=ga), torch.rand(256, generator=gb))


def _assert_run(got, r, alone, what, ahead_draws=None):
    model, opt = got["models"][r], got["opts"][r]
    assert torch.equal(torch.from_numpy(H.flat_params(model)), alone["p"]), f"{what}: parameters"
    assert torch.equal(torch.from_numpy(H.flat_state(opt, "exp_avg")), alone["m"]), f"{what}: exp_avg"
    assert torch.equal(torch.from_numpy(H.flat_state(opt, "exp_avg_sq")), alone["v"]), f"{what}: exp_avg_sq"
    assert [int(float(opt.state[p]["step"])) for p in model.parameters()] == alone["steps"], f"{what}: step counts"
    for e in range(EPOCHS):
        assert torch.equal(got["losses"][e][r], alone["losses"][e]), f"{what}: losses of pass {e}"
    # the run's generator: the default generator after the run alone, plus the pass TrainRuns has drawn ahead
    g = torch.Generator()
    g.set_state(alone["rng"])
    torch.rand(_rows() if ahead_draws is None else ahead_draws, generator=g)
    assert _same_next_draws(g.get_state(), got["gens"][r].get_state()), f"{what}: generator state"


_alone_cache = {}


def _alone_grid(dev):
    """The eight runs of tests 1-3 alone, computed once."""
    if "grid" not in _alone_cache:
        _alone_cache["grid"] = [_alone(dev, r % 2, CONFIGS[r // 2], 2, 512, torch.float32, 100 + r, 7000 + r % 2) for r in range(8)]
    return _alone_cache["grid"]


def test_per_run_hyper_parameters_are_each_run_alone(dev, monkeypatch):
    monkeypatch.delenv("MOC_RUNS_SHARE", raising=False)
    alone = _alone_grid(dev)
    got = _grid(dev, CONFIGS, 2, 2, 512, torch.float32)
    for r in range(8):
        _assert_run(got, r, alone[r], f"run {r} {CONFIGS[r // 2]}")
    rs = got["rs"]
    assert rs.last_phase_a == {"slides": 24, "scored_slides": 6, "shared_slides": 18}
    assert all(tr == {"slides": 24, "scored_slides": 6, "shared_slides": 18} for tr, _ in got["reports"])
    # chains never mix configurations; the bags of a split shared by four runs are held once
    for g in rs.groups:
        assert len({rs.cfg[r] for r in range(g["r0"], g["r0"] + g["runs"].n_runs)}) == 1
    assert rs.X.size(0) == 2 * _rows()


def test_without_sharing_every_run_is_scored(dev, monkeypatch):
    monkeypatch.setenv("MOC_RUNS_SHARE", "0")
    alone = _alone_grid(dev)
    got = _grid(dev, CONFIGS, 2, 2, 512, torch.float32)
    for r in range(8):
        _assert_run(got, r, alone[r], f"run {r} {CONFIGS[r // 2]}")
    assert got["rs"].last_phase_a == {"slides": 24, "scored_slides": 24, "shared_slides": 0}


def test_a_generator_that_diverges_leaves_its_group(dev, monkeypatch):
    """After pass 1 the caller draws one number from run 3's generator.  The masks of pass 2 were drawn ahead, at the end of
    pass 1; the draw made during pass 2 finds run 3 apart from its group and scores it for itself.  In run 3's mask stream
    the extra number lies behind the masks of pass 2 -- where the run alone draws it.
    (A run is three slides, so a run that leaves its group adds three scored slides: 9, not the 7 the issue's text names --
    6 + 1 counts the run, the report counts slides, as its 6 / 18 of test 1 do.)"""
    monkeypatch.delenv("MOC_RUNS_SHARE", raising=False)
    alone = list(_alone_grid(dev))
    alone[3] = _alone(dev, 1, CONFIGS[1], 2, 512, torch.float32, 103, 7001, extra_draw_after=1)
    got = _grid(dev, CONFIGS, 2, 2, 512, torch.float32, touch=(3, 0))
    assert got["reports"][0][1]["scored_slides"] == 6            # drawn before the touch
    assert got["reports"][1][1] == {"slides": 24, "scored_slides": 9, "shared_slides": 15}, got["reports"]
    assert got["reports"][2][0]["scored_slides"] == 9            # ... and the pass trained from that draw
    for r in range(8):
        _assert_run(got, r, alone[r], f"run {r} {CONFIGS[r // 2]}")


@pytest.mark.parametrize("C_,D,dtype,configs,cache", [
    (2, 512, torch.bfloat16, CONFIGS[:3], False),
    (2, 512, torch.float16, CONFIGS[1:], False),
    (3, 512, torch.float32, CONFIGS[:3], False),
    (30, 1024, torch.bfloat16, [(40, 10, ()), (60, 5, ("bottomk",))], False),       # wide bank: mode 2, compact statistics
    (2, 512, torch.float32, CONFIGS[:3], True),                                   # cache_scores: no score pass at all
])
def test_other_storages_and_banks(dev, monkeypatch, C_, D, dtype, configs, cache):
    monkeypatch.delenv("MOC_RUNS_SHARE", raising=False)
    got = _grid(dev, configs, 2, C_, D, dtype, cache=cache)
    rs = got["rs"]
    assert rs.mode == (1 if C_ <= 16 else 2)
    assert rs.last_phase_a == {"slides": 6 * len(configs), "scored_slides": 6, "shared_slides": 6 * (len(configs) - 1)}
    for r in range(2 * len(configs)):
        alone = _alone(dev, r % 2, configs[r // 2], C_, D, dtype, 100 + r, 7000 + r % 2, cache=cache)
        _assert_run(got, r, alone, f"run {r} {configs[r // 2]}")


def test_mixed_topk_chains_keep_their_pooled_positions_apart(dev, monkeypatch):
    """K = 3, 5, 10 and 16 side by side, each chain on its own stream: [slide, C, K] regions with the batch's one K as the
    stride would overlap (slides 0-5 at K = 16 cover slides 6-11 at K = 3 ...)."""
    monkeypatch.delenv("MOC_RUNS_SHARE", raising=False)
    configs = [(100, K, ()) for K in (3, 5, 10, 16)]
    seen = {}

    def read(e, rs):
        if e == EPOCHS - 1:
            cnt = rs.last[0].meta_ws()[0]["topk_cnt"].cpu()
            for r in range(8):
                seen[r] = (rs.topk_idx(r).cpu().clone(), cnt[rs.run_slide0[r]:rs.run_slide0[r] + rs.run_n[r]].clone())
    got = _grid(dev, configs, 2, 2, 512, torch.float32, on_pass=read)
    rs = got["rs"]
    assert len(rs.groups) == 4 and len({id(g["stream"]) for g in rs.groups}) == 4
    for r in range(8):
        alone = _alone(dev, r % 2, configs[r // 2], 2, 512, torch.float32, 100 + r, 7000 + r % 2)
        _assert_run(got, r, alone, f"run {r} K={configs[r // 2][1]}")
        assert tuple(seen[r][0].shape) == (3, 2, configs[r // 2][1])
        assert torch.equal(seen[r][0], alone["idx"]), f"run {r}: topk_idx"
        assert torch.equal(seen[r][1], alone["cnt"]), f"run {r}: topk_cnt"


# ---- moc_stats_share alone
# eight visits: leaders 1 and 6 (leader 1 lies BEHIND its follower 0), followers {0, 2, 3} -> 1 and {7} -> 6, slides 4 and 5
# unrelated.  Layout "vec" (6,556 slots, a multiple of four): follower 3 takes the 16-byte path with a two-word head
# (first slot 3,090), follower 7 the 16-byte path without a head, followers 0 and 2 lie an odd number of 8-byte pairs from
# their leader and copy word by word.  519 is off the list of sizes above on purpose: it makes the slot count a multiple of
# four.  Layout "odd" (5,381 slots): no row of the arrays is 16-byte aligned with another -- everything word by word.
LAYOUTS = {"vec": (1030, 1030, 1030, 1030, 517, 519, 700, 700), "odd": (700, 700, 700, 700, 1030, 517, 517, 517)}
LEADER_OF = (1, -1, 1, 1, -1, -1, -1, 6)


@pytest.mark.parametrize("C_,dtype,layout,zero_slide", [
    (2, torch.float32, "vec", 5),
    (2, torch.float32, "odd", 6),
    (2, torch.bfloat16, "vec", 6),
    (2, torch.float16, "vec", 5),
    (30, torch.bfloat16, "vec", 5),                             # compact statistics (C + 5 rows)
    (30, torch.bfloat16, "odd", 6),
])
def test_stats_share_alone(dev, C_, dtype, layout, zero_slide):
    """Arm A: today's moc_phase_a over all eight slides.  Arm B: compaction and scores over the leaders and the unrelated
    slides, the share, selection and candidates over all slides.  (The issue's arm B clears the followers' sel_flag by hand
    after the share; moc_stats_share does that itself -- the arrays are pre-filled with ones, so a flag left standing shows.)"""
    from moc_amd import engine, main_moc as M
    from moc_amd._lib import check, lib, ptr
    from moc_amd.runs import TrainRuns
    D, topj = 512, 60
    sizes = LAYOUTS[layout]
    W, We = _bank(C_, D)
    # the underlying bags: one per leader / unrelated slide; the followers' visits point at their leader's rows
    own = [b for b in range(8) if LEADER_OF[b] < 0]
    bags, _ = synth.make_slide_set(4242, [sizes[b] for b in own], D, We, C_)
    X = torch.cat([b.to(dtype) for b in bags], 0).to(dev)
    first, o = {}, 0
    for b, bag in zip(own, bags):
        first[b] = o
        o += bag.size(0)
    starts = [first[b if LEADER_OF[b] < 0 else LEADER_OF[b]] for b in range(8)]
    g = torch.Generator()
    g.manual_seed(77)
    own_mask = {b: (torch.rand(sizes[b], generator=g) > 0.5).to(torch.uint8) for b in own}
    own_mask[zero_slide].zero_()                                # one slide keeps no row at all
    mask = torch.cat([own_mask[b if LEADER_OF[b] < 0 else LEADER_OF[b]] for b in range(8)])
    bank = engine.Bank.get(W.to(dev), We.to(dev), dtype, dev)
    nan_i = 0x7FC00000

    def fresh():
        b = engine.SlideBatch(X, sizes, C_, We.size(1), topj, 10, (), mask=mask, x_starts=starts)
        b.stats.fill_(float("nan"))
        b.cand.fill_(float("nan"))
        b.kept.fill_(nan_i)
        b.sel_idx.fill_(nan_i)
        b.sel_row.fill_(nan_i)
        b.n_kept.zero_()                                        # (counts size loops: a missing one must not send a kernel astray)
        b.n_sel.zero_()
        b.sel_flag.fill_(1)
        return b
    A = fresh()
    A.phase_a(bank)
    Bb = fresh()
    Bb._layout(engine.COMPACT_STATS and Bb.Ce > 16)
    assert Bb.c.flags == A.c.flags and bool(A.c.flags & 1) == (C_ == 30)
    st = engine._stream()
    for s0, n in ((1, 1), (4, 3)):                              # the leaders and the unrelated slides
        v = TrainRuns._view(Bb.c, s0, n)
        check(lib().moc_mask_compact(C.byref(v), st), "moc_mask_compact")
        check(lib().moc_scores(C.byref(v), ptr(bank.image), st), "moc_scores")
    lead = torch.tensor(LEADER_OF, dtype=torch.int32).to(dev)
    check(lib().moc_stats_share(C.byref(Bb.c), ptr(lead), 0, 8, st), "moc_stats_share")
    Bb.select()
    Bb.gather_candidates()
    torch.cuda.synchronize()
    NS = C_ + 5 if C_ == 30 else 2 * C_ + 3
    nk_a, nk_b = A.n_kept.cpu(), Bb.n_kept.cpu()
    assert torch.equal(nk_a, nk_b), (nk_a, nk_b)
    assert int(nk_a[zero_slide]) == 0 and (zero_slide != 6 or int(nk_a[7]) == 0)
    ns_a, ns_b = A.n_sel.cpu(), Bb.n_sel.cpu()
    assert torch.equal(ns_a, ns_b), (ns_a, ns_b)
    off = A.row_off_host
    bits = lambda t: t.view(torch.int32)
    for b in range(8):
        k, s_ = int(nk_a[b]), int(ns_a[b])
        lo = off[b]
        assert torch.equal(A.kept[lo:lo + k], Bb.kept[lo:lo + k]), f"slide {b}: kept"
        assert torch.equal(bits(A.stats[:NS, lo:lo + k]), bits(Bb.stats[:NS, lo:lo + k])), f"slide {b}: statistics"
        assert not torch.isnan(Bb.stats[:NS, lo:lo + k]).any(), f"slide {b}: a statistic was never written"
        assert torch.equal(A.sel_flag[lo:lo + k], Bb.sel_flag[lo:lo + k]), f"slide {b}: sel_flag"
        assert torch.equal(A.sel_idx[lo:lo + s_], Bb.sel_idx[lo:lo + s_]), f"slide {b}: sel_idx"
        assert torch.equal(A.sel_row[lo:lo + s_], Bb.sel_row[lo:lo + s_]), f"slide {b}: sel_row"
        assert torch.equal(bits(A.cand[:, lo:lo + s_]), bits(Bb.cand[:, lo:lo + s_])), f"slide {b}: cand"
        assert s_ == 0 or not torch.isnan(Bb.cand[:, lo:lo + s_]).any()
    # nothing behind a follower's kept rows was touched (the copy stops at n_kept[leader])
    for b in (0, 2, 3, 7):
        k = int(nk_a[b])
        assert torch.isnan(Bb.stats[:NS, off[b] + k:off[b + 1]]).all() and bool((Bb.kept[off[b] + k:off[b + 1]] == nan_i).all())
    # a bad leader index is clamped into the batch: nothing outside the arrays is read (slide 4 then copies from slide 7,
    # clipped to the shorter of the two)
    bad = torch.tensor((-1, -1, -1, -1, 1000, -1, -1, -1), dtype=torch.int32).to(dev)
    check(lib().moc_stats_share(C.byref(Bb.c), ptr(bad), 4, 1, st), "moc_stats_share")
    torch.cuda.synchronize()
    assert int(Bb.n_kept[4]) == min(int(nk_a[7]), sizes[4])


def test_driver_grid_reproduces_every_single_configuration(dev, tmp_path):
    """`run_moc --topjs 50,100 --topks 5,10 --discard_sets none topk+bottomk --folds 0,1`: every configuration directory
    holds what the single-configuration `--folds 0,1` run writes into it, the best checkpoints the same bits; --summary
    reads one of them."""
    from moc_amd import run_moc
    common = ["--synthetic", "24", "--shot", "4", "--folds", "0,1", "--seed", "1", "--disable_tqdm", "--epochs", "1"]
    grid = run_moc.cli(common + ["--topjs", "50,100", "--topks", "5,10", "--discard_sets", "none", "topk+bottomk",
                                 "--result_dir", str(tmp_path / "grid")])
    assert len(grid) == 16
    for J in (50, 100):
        for K in (5, 10):
            for name, flag in (("none", []), ("topk+bottomk", ["--discard_classifiers", "topk", "bottomk"])):
                sub = f"topj{J}_topk{K}_{name}"
                run_moc.cli(common + ["--topj", str(J), "--topk", str(K)] + flag + ["--result_dir", str(tmp_path / "alone" / sub)])
                for fold in (0, 1):
                    for stem in (f"zs_results_shot_4_fold_{fold}.json", f"best_results_shot_4_fold_{fold}.json"):
                        a = json.load(open(tmp_path / "alone" / sub / stem))
                        b = json.load(open(tmp_path / "grid" / sub / stem))
                        a.pop("best_model_path", None)
                        assert b.pop("best_model_path", None) in (None, str(tmp_path / "grid" / sub / f"best_model_shot_4_fold_{fold}.pt"))
                        assert a == b, (sub, fold, stem, a, b)
                    sa = torch.load(tmp_path / "alone" / sub / f"best_model_shot_4_fold_{fold}.pt", map_location="cpu")
                    sb = torch.load(tmp_path / "grid" / sub / f"best_model_shot_4_fold_{fold}.pt", map_location="cpu")
                    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa), (sub, fold)
    # --summary reads a configuration directory like any --result_dir: give it the three other folds of one configuration
    run_moc.cli(common[:5] + ["2,3,4"] + common[6:] + ["--topjs", "50", "--topks", "5", "--discard_sets", "none",
                                                       "--result_dir", str(tmp_path / "grid")])
    one = tmp_path / "grid" / "topj50_topk5_none"
    run_moc.cli(["--summary", "--summary_dir", str(one)])
    table = open(one / "summary_4.csv").read().splitlines()
    assert table[0].startswith("fold,test_auc") and len(table) == 7
