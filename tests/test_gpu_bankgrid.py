"""A bank grid in one process (moc_amd.runs with `banks` / `bank_of_run`): the runs of one fold and seed
under several narrow prompt banks share one mask draw and one multi-bank score pass per pass, and every run is, bit for
bit, that run trained alone by train_runs after set_classifier_bank of its bank.  Everything is exact.

Folds: slides of (1, 600, 17, 255) rows, and of (16, 15, 256, 2) rows visited five times per pass (repeat_num: the first
slide twice).  topj = 20 exceeds what most of them keep.  A slide whose every row a mask drops has no meta-step to compare
(its top-k pools nothing), so the generators' seeds are the first under which the one- and two-row slides keep a row in each
of the passes trained; `_seed_keeping` replays the draws on the host to find them."""
import ctypes as C
import json
import os

import pytest
import torch

import helpers as H
from moc_amd import synth

pytestmark = pytest.mark.gpu

FOLDS = (((1, 600, 17, 255), None), ((16, 15, 256, 2), 5))
EPOCHS = 3
TOPJ, TOPK = 20, 5


@pytest.fixture(scope="module")
def dev(gpu_device):
    return gpu_device


def _visits(sizes, repeat):
    return [sizes[i % len(sizes)] for i in range(repeat or len(sizes))]


def _seed_keeping(visits, passes, first=1):
    """The first seed >= `first` whose generator keeps a row of every visited slide in each of `passes` passes
    (torch.rand(N) > 0.5 per visit, in order: main_moc.train's draws)."""
    for seed in range(first, first + 100000):
        g = torch.Generator()
        g.manual_seed(seed)
        if all(bool((torch.rand(n, generator=g) > 0.5).any()) for _ in range(passes) for n in visits):
            return seed
    raise AssertionError("no seed found")


_seeds = {}


def _fold_seed(f):
    if f not in _seeds:
        _seeds[f] = _seed_keeping(_visits(*FOLDS[f]), EPOCHS + 1, first=1 + 1000 * f)
    return _seeds[f]


def _banks(C_, D, ces, dev):
    return [tuple(t.to(dev) for t in synth.make_bank(700 + 13 * g + ce, D, C_, n_bg=ce - C_)) for g, ce in enumerate(ces)]


def _fold_bags(f, C_, D, dtype, folds=FOLDS):
    _, We = synth.make_bank(700, D, C_)
    bags, labels = synth.make_slide_set(4100 + 91 * f, list(folds[f][0]), D, We, C_)
    return [b.to(dtype) for b in bags], labels


def _snapshot(model, opt):
    return (torch.from_numpy(H.flat_params(model)), torch.from_numpy(H.flat_state(opt, "exp_avg")),
            torch.from_numpy(H.flat_state(opt, "exp_avg_sq")))


def _alone(dev, split, bank, C_, D, model_seed, gen_seed, cfg=(TOPJ, TOPK, ()), lr=1e-3, touch_after=None):
    """The existing train_runs with ONE run after set_classifier_bank of its bank -> per pass (params, m, v, losses)."""
    from moc_amd import main_moc as M
    M.set_classifier_bank(*bank)
    torch.manual_seed(model_seed)
    model = M.senet(D, 4).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=1e-4)
    g = torch.Generator()
    g.manual_seed(gen_seed)
    out = []
    for e in range(EPOCHS):
        rs = M.train_runs([model], [split], [opt], dev, H.make_args(C_, *cfg), generators=[g])
        torch.cuda.synchronize()
        out.append(_snapshot(model, opt) + (rs.losses().cpu().clone().reshape(-1),))
        if touch_after == e:
            torch.rand(1, generator=g)
    return out


def _assert_pass(got, alone, what):
    for name, a, b in zip(("parameters", "exp_avg", "exp_avg_sq", "losses"), got, alone):
        assert torch.equal(a, b), f"{what}: {name}"


# ------------------------------------------------------------------ 1. moc_kept_share alone
SHARE_SIZES = (1, 2, 15, 16, 17, 255, 600)
SENTINEL = -0x5A5A5A5B


@pytest.mark.parametrize("pad", [None, 2, 1, 3])      # slots between a leader and its follower: 906 + pad = 2, 0, 3, 1 mod 4
def test_kept_share_copies_the_lists_and_nothing_else(dev, pad):
    from moc_amd import engine as E
    from moc_amd._lib import lib, ptr
    group = list(SHARE_SIZES) + ([pad] if pad else [])
    n = len(group)
    sizes = group * 3                                  # groups A, B, C: B leads A (a leader behind its follower) and C
    T = sum(sizes)
    assert (sum(group) % 4) == {None: 2, 2: 0, 1: 3, 3: 1}[pad]
    g = torch.Generator()
    g.manual_seed(11)
    m = (torch.rand(sum(group), generator=g) > 0.5).to(torch.uint8)
    m[0] = 1
    X = torch.randn((T, 256), generator=torch.Generator().manual_seed(1)).to(dev)
    b = E.SlideBatch(X, sizes, 2, 6, TOPJ, TOPK, (), mask=torch.cat([m, m, m]))
    E.check(lib().moc_mask_compact(C.byref(b.c), E._stream()), "moc_mask_compact")
    torch.cuda.synchronize()
    ref_kept, ref_nk = b.kept.clone(), b.n_kept.clone()
    off = b.row_off_host
    # followers: sentinel lists; statistics and flags: patterns the call must leave
    expect = ref_kept.clone()
    for s in list(range(0, n)) + list(range(2 * n, 3 * n)):
        b.kept[off[s]:off[s + 1]] = SENTINEL
        b.n_kept[s] = SENTINEL
        expect[off[s]:off[s + 1]] = SENTINEL
        nk = int(ref_nk[s])
        expect[off[s]:off[s] + nk] = ref_kept[off[s]:off[s] + nk]
    b.stats.fill_(float("nan"))
    b.sel_flag.fill_(0xA5)
    lead = torch.tensor([n + s for s in range(n)] + [-1] * n + [n + s for s in range(n)], dtype=torch.int32).to(dev)
    E.check(lib().moc_kept_share(C.byref(b.c), ptr(lead), 0, 3 * n, E._stream()), "moc_kept_share")
    torch.cuda.synchronize()
    assert torch.equal(b.n_kept, ref_nk)
    assert torch.equal(b.kept, expect)                 # (the 16 words behind the last slot included)
    assert bool(torch.isnan(b.stats).all()) and bool((b.sel_flag == 0xA5).all())


def test_kept_share_on_an_unmasked_batch_changes_nothing(dev):
    from moc_amd import engine as E
    from moc_amd._lib import lib, ptr
    sizes = [17, 600, 17, 600]
    X = torch.randn((sum(sizes), 256), generator=torch.Generator().manual_seed(2)).to(dev)
    b = E.SlideBatch(X, sizes, 2, 6, TOPJ, TOPK, ())
    b.stats.fill_(float("nan"))
    b.sel_flag.fill_(0xA5)
    lead = torch.tensor([2, 3, -1, -1], dtype=torch.int32).to(dev)
    assert lib().moc_kept_share(C.byref(b.c), ptr(lead), 0, 4, E._stream()) == 0
    torch.cuda.synchronize()
    assert b.kept is None and bool(torch.isnan(b.stats).all()) and bool((b.sel_flag == 0xA5).all())


# ------------------------------------------------------------------ 2. training, exact against each run alone
CASES = [
    # C, D, storage, Ce of every bank
    (2, 256, torch.float32, (3, 6)),
    (2, 512, torch.float32, (3, 6, 16, 6, 4)),               # passes 4 + 1
    (2, 512, torch.bfloat16, (16, 3, 6, 5, 6)),              # passes 3 + 2
    (3, 512, torch.float16, (4, 7)),
    (3, 256, torch.bfloat16, (7, 4, 7, 5, 4)),
]
_alone_cache = {}


def _alone_case(dev, ci):
    if ci not in _alone_cache:
        C_, D, dtype, ces = CASES[ci]
        from moc_amd import main_moc as M
        banks = _banks(C_, D, ces, dev)
        out = {}
        for f in range(2):
            bags, labels = _fold_bags(f, C_, D, dtype)
            split = M.ResidentBags(bags, labels, dev, repeat_num=FOLDS[f][1])
            for g in range(len(ces)):
                out[(g, f)] = _alone(dev, split, banks[g], C_, D, 100 + 2 * g + f, _fold_seed(f))
        _alone_cache[ci] = out
    return _alone_cache[ci]


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_bank_grid_is_each_run_alone(dev, monkeypatch, ci, fused):
    from moc_amd import engine as E, main_moc as M, runs
    monkeypatch.setenv("MOC_RUNS_BANKS_FUSED", fused)
    monkeypatch.delenv("MOC_RUNS_SHARE", raising=False)
    C_, D, dtype, ces = CASES[ci]
    G = len(ces)
    alone = _alone_case(dev, ci)
    banks = _banks(C_, D, ces, dev)
    keep = (M.zeroshot_weights, M.zeroshot_weights_ext)
    shared = []
    for f in range(2):
        bags, labels = _fold_bags(f, C_, D, dtype)
        shared.append(M.ResidentBags(bags, labels, dev, repeat_num=FOLDS[f][1]))
    models, opts, splits, gens, of_run = [], [], [], [], []
    for g in range(G):                                       # bank-major
        for f in range(2):
            torch.manual_seed(100 + 2 * g + f)
            model = M.senet(D, 4).to(dev)
            models.append(model)
            opts.append(torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4))
            splits.append(shared[f])
            gen = torch.Generator()
            gen.manual_seed(_fold_seed(f))
            gens.append(gen)
            of_run.append(g)
    args = H.make_args(C_, TOPJ, TOPK)
    for e in range(EPOCHS):
        rs = M.train_runs(models, splits, opts, dev, args, generators=gens, banks=banks, bank_of_run=of_run)
        torch.cuda.synchronize()
        losses = rs.losses()
        for r in range(2 * G):
            g, f = r // 2, r % 2
            _assert_pass(_snapshot(models[r], opts[r]) + (losses[r].cpu().reshape(-1),), alone[(g, f)][e],
                         f"pass {e}, bank {g} (Ce={ces[g]}), fold {f}")
        plan = runs.bank_score_plan([0, 1] * G, of_run, rs.run_slide0, rs.run_n, rs.batches[0].row_off_host,
                                    E.plan_bank_passes(D, dtype, G))
        assert len(plan) == (1 if G <= 3 else 2)             # both folds' leaders in one launch per pass of the set
        want = {"slides": 9 * G, "scored_slides": 9, "shared_slides": 9 * (G - 1), "bank_passes": len(plan) if fused == "1" else 0}
        assert rs.last_phase_a == want and rs.trained_phase_a == want
    assert M.zeroshot_weights is keep[0] and M.zeroshot_weights_ext is keep[1]      # the module's bank is not touched


# ------------------------------------------------------------------ 3. the other grids' axes, in the same TrainRuns
SIZES3 = (((37, 300, 64), None),)


def _grid3(dev, banks, cells, touch=None, per_run_adam=False):
    """cells: [(bank, cfg, lr)] over one fold -> per pass the snapshots of every run, and the reports."""
    from moc_amd import main_moc as M
    bags, labels = _fold_bags(0, 2, 512, torch.float32, SIZES3)
    split = M.ResidentBags(bags, labels, dev)
    models, opts, gens, args = [], [], [], []
    for r, (g, cfg, lr) in enumerate(cells):
        torch.manual_seed(300 + r)
        model = M.senet(512, 4).to(dev)
        models.append(model)
        opts.append(torch.optim.Adam(model.parameters(), lr=lr, weight_decay=1e-4))
        gen = torch.Generator()
        gen.manual_seed(77)
        gens.append(gen)
        args.append(H.make_args(2, *cfg))
    out, reports = [], []
    for e in range(EPOCHS):
        rs = M.train_runs(models, [split] * len(cells), opts, dev, args, generators=gens, per_run_adam=per_run_adam,
                          banks=banks, bank_of_run=[g for g, _, _ in cells])
        torch.cuda.synchronize()
        losses = rs.losses()
        out.append([_snapshot(models[r], opts[r]) + (losses[r].cpu().reshape(-1),) for r in range(len(cells))])
        reports.append(dict(rs.last_phase_a))
        if touch is not None and touch[1] == e:
            torch.rand(1, generator=gens[touch[0]])
    return out, reports, split


def _check3(dev, banks, cells, out, touch=None):
    from moc_amd import main_moc as M
    bags, labels = _fold_bags(0, 2, 512, torch.float32, SIZES3)
    split = M.ResidentBags(bags, labels, dev)
    for r, (g, cfg, lr) in enumerate(cells):
        alone = _alone(dev, split, banks[g], 2, 512, 300 + r, 77, cfg=cfg, lr=lr,
                       touch_after=touch[1] if touch is not None and touch[0] == r else None)
        for e in range(EPOCHS):
            _assert_pass(out[e][r], alone[e], f"pass {e}, run {r}: bank {g}, {cfg}, lr {lr}")


def test_banks_times_selection_configurations(dev, monkeypatch):
    monkeypatch.delenv("MOC_RUNS_BANKS_FUSED", raising=False)
    banks = _banks(2, 512, (6, 4), dev)
    cfgs = [(TOPJ, TOPK, ()), (10, 3, ("delta_diff",))]
    cells = [(g, cfg, 1e-3) for cfg in cfgs for g in range(2)]          # configuration-major: chains of one configuration
    out, reports, _ = _grid3(dev, banks, cells)
    # one draw, one launch over the leader's three slides; the second configuration's runs are filled by moc_stats_share
    assert all(rp == {"slides": 12, "scored_slides": 3, "shared_slides": 9, "bank_passes": 1} for rp in reports)
    _check3(dev, banks, cells, out)


def test_banks_times_learning_rates(dev, monkeypatch):
    monkeypatch.delenv("MOC_RUNS_BANKS_FUSED", raising=False)
    banks = _banks(2, 512, (6, 4), dev)
    cells = [(g, (TOPJ, TOPK, ()), lr) for g in range(2) for lr in (1e-3, 3e-4)]
    out, reports, _ = _grid3(dev, banks, cells, per_run_adam=True)
    assert all(rp["bank_passes"] == 1 and rp["scored_slides"] == 3 for rp in reports)
    _check3(dev, banks, cells, out)


def test_a_run_that_leaves_its_mask_group_is_scored_for_itself(dev, monkeypatch):
    monkeypatch.delenv("MOC_RUNS_BANKS_FUSED", raising=False)
    banks = _banks(2, 512, (6, 4, 5), dev)
    cells = [(g, (TOPJ, TOPK, ()), 1e-3) for g in range(3)]
    out, reports, _ = _grid3(dev, banks, cells, touch=(1, 0))
    assert reports[0] == {"slides": 9, "scored_slides": 3, "shared_slides": 6, "bank_passes": 1}       # drawn before the touch
    # run 1 is its own leader from the next draw on: its launch carries its bank alone
    assert reports[1] == {"slides": 9, "scored_slides": 6, "shared_slides": 3, "bank_passes": 2}, reports
    _check3(dev, banks, cells, out, touch=(1, 0))


# ------------------------------------------------------------------ 4. the driver
def test_driver_writes_what_every_bank_and_fold_writes_alone(dev, tmp_path, monkeypatch, capsys):
    import pandas as pd
    import shutil
    from moc_amd import main_moc as M, run_moc
    monkeypatch.delenv("MOC_RUNS_BANKS_FUSED", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    names, spec, banks = ("a", "b", "c"), [], {}
    for name, n_bg in zip(names, (4, 1, 9)):
        W, We = synth.make_bank(900 + n_bg, 512, 2, n_bg=n_bg)
        fw, fe = str(tmp_path / f"{name}_w.pt"), str(tmp_path / f"{name}_we.pt")
        torch.save(W, fw)
        torch.save(We, fe)
        spec.append(f"{name}={fw},{fe}")
        banks[name] = (W, We)
    common = ["--synthetic", "6", "--shot", "2", "--epochs", "2", "--seed", "1", "--disable_tqdm"]
    out = str(tmp_path / "grid")
    res = run_moc.cli(common + ["--folds", "0,1", "--result_dir", out, "--banks"] + spec)
    printed = capsys.readouterr().out
    assert len(res) == 6 and all(f"[bank {n}] [fold {f}] Best Val" in printed for n in names for f in (0, 1))
    n_ckpt = 0
    for name in names:
        for fold in (0, 1):
            alone_dir = str(tmp_path / f"alone_{name}")
            a = run_moc.get_args(common + ["--fold", str(fold), "--result_dir", alone_dir])
            loaders = run_moc.prepare(a, dev)
            M.set_classifier_bank(banks[name][0].to(dev), banks[name][1].to(dev))
            torch.manual_seed(1)
            model = M.senet(512, 4).to(dev)
            opt = torch.optim.Adam(model.parameters(), lr=a.lr, weight_decay=a.weight_decay)
            want = run_moc.main(a, model, opt, *loaders, dev)
            d = run_moc.bankgrid_dir(out, name)
            for stem in ("best_results", "zs_results"):
                got_j = json.load(open(os.path.join(d, f"{stem}_shot_2_fold_{fold}.json")))
                want_j = json.load(open(os.path.join(alone_dir, f"{stem}_shot_2_fold_{fold}.json")))
                got_j.pop("best_model_path", None)
                want_j.pop("best_model_path", None)
                assert got_j == want_j, (name, fold, stem)
            # (a checkpoint is written when the validation AUC first exceeds 0: a run whose AUC stays 0 writes none, in either way)
            got_pt = os.path.join(d, f"best_model_shot_2_fold_{fold}.pt")
            assert os.path.exists(got_pt) == os.path.exists(want["best_model_path"]), (name, fold)
            if os.path.exists(got_pt):
                n_ckpt += 1
                got_sd, want_sd = torch.load(got_pt, map_location="cpu"), torch.load(want["best_model_path"], map_location="cpu")
                assert got_sd.keys() == want_sd.keys() and all(torch.equal(got_sd[k], want_sd[k]) for k in got_sd), (name, fold)
    capsys.readouterr()
    assert n_ckpt >= 1                                        # (most runs do improve: the comparison is not empty)
    # bank_grid_summary.csv: the JSONs' numbers
    t = pd.read_csv(os.path.join(out, "bank_grid_summary.csv"), float_precision="round_trip")
    assert list(t["bank"]) == list(names) and list(t["runs"]) == [2, 2, 2]
    for i, name in enumerate(names):
        js = [json.load(open(os.path.join(run_moc.bankgrid_dir(out, name), f"best_results_shot_2_fold_{f}.json"))) for f in (0, 1)]
        bv, ta = [j["best_val"] for j in js], [j["test_at_best_val"] for j in js]
        assert t["best_val_mean"][i] == (bv[0] + bv[1]) / 2 and t["best_val_std"][i] == abs(bv[0] - bv[1]) / 2
        assert t["test_auc_mean"][i] == (ta[0] + ta[1]) / 2 and t["test_auc_std"][i] == abs(ta[0] - ta[1]) / 2
    # --summary reads a bank's directory (it wants five folds: folds 2-4 here are copies of fold 0's file)
    d = run_moc.bankgrid_dir(out, "b")
    for f in (2, 3, 4):
        shutil.copy(os.path.join(d, "best_results_shot_2_fold_0.json"), os.path.join(d, f"best_results_shot_2_fold_{f}.json"))
    run_moc.cli(["--summary", "--summary_dir", d])
    table = pd.read_csv(os.path.join(d, "summary_2.csv"))
    js = [json.load(open(os.path.join(d, f"best_results_shot_2_fold_{f}.json"))) for f in (0, 1)]
    assert list(table["test_auc"][:2]) == [j["test_at_best_val"] for j in js]
