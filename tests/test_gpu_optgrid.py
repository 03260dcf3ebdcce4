"""A seeds x lr x weight-decay grid in one process: runs that share a split, their initial parameters
and their mask stream and differ in Adam's hyper-parameters step in ONE lockstep chain (moc_train_steps_runs_hp: run r's
coefficients by value in the step launch), and every run is, bit for bit, main_moc.train with that run's optimizer.

Bags: D = 512, three slides of 617 / 1,030 / 1,411 rows (no multiple of 16 or 256), two passes, topj 100, topk 5."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import helpers as H
from moc_amd import synth
from oracle import moc_oracle as O

pytestmark = pytest.mark.gpu

SIZES = (617, 1030, 1411)
EPOCHS = 2
GRID = [(1e-3, 1e-4), (3e-3, 0.0), (3e-4, 1e-2), (1e-3, 1e-4)]
NINE = [(1e-4 * (k + 1), 1e-4) for k in range(9)]            # nine distinct learning rates
MODEL_SEED, GEN_SEED = 100, 7000


@pytest.fixture(scope="module")
def dev(gpu_device):
    return gpu_device


def _bank(C_, D=512):
    return synth.make_bank(31 + C_, D, C_)


def _bags(C_, dtype, D=512):
    W, We = _bank(C_, D)
    bags, labels = synth.make_slide_set(9000, list(SIZES), D, We, C_)
    return [b.to(dtype) for b in bags], labels


_alone_cache = {}


def _adam(params, hp):
    """hp: (lr, weight_decay), or the full (lr, (beta1, beta2), eps, weight_decay)"""
    if len(hp) == 2:
        return torch.optim.Adam(params, lr=hp[0], weight_decay=hp[1])
    lr, betas, eps, wd = hp
    return torch.optim.Adam(params, lr=lr, betas=betas, eps=eps, weight_decay=wd)


def _alone(dev, lr, wd, C_=2, dtype=torch.float32, j=100, K=5, betas=None, eps=None):
    """main_moc.train for EPOCHS passes with Adam(lr, weight_decay) -- and, where given, betas and eps -> what a cell of the
    grid must reproduce (computed once per cell and shared by the tests; never modified)."""
    key = (lr, wd, C_, dtype, j, K, betas, eps)
    if key not in _alone_cache:
        from moc_amd import main_moc as M
        W, We = _bank(C_)
        M.set_classifier_bank(W.to(dev), We.to(dev))
        bags, labels = _bags(C_, dtype)
        torch.manual_seed(MODEL_SEED)
        model = M.senet(512, 4).to(dev)
        opt = _adam(model.parameters(), (lr, wd) if betas is None else (lr, betas, eps, wd))
        res = M.ResidentBags(bags, labels, dev)
        args = H.make_args(C_, j, K)
        torch.manual_seed(GEN_SEED)
        losses = []
        for _ in range(EPOCHS):
            M.train(model, res, opt, dev, args)
            torch.cuda.synchronize()
            losses.append(M.train.last[0].meta_ws()[0]["loss"].cpu().numpy().copy())
        _alone_cache[key] = dict(p=H.flat_params(model), m=H.flat_state(opt, "exp_avg"), v=H.flat_state(opt, "exp_avg_sq"),
                                 losses=losses)
    return _alone_cache[key]


def _grid(dev, hps, C_=2, dtype=torch.float32, j=100, K=5, per_run_adam=True, epochs=EPOCHS):
    """The cells through train_runs: ONE split object, equal initial parameters, equal generator states."""
    from moc_amd import main_moc as M
    W, We = _bank(C_)
    M.set_classifier_bank(W.to(dev), We.to(dev))
    bags, labels = _bags(C_, dtype)
    split = M.ResidentBags(bags, labels, dev)
    models, opts, gens = [], [], []
    for hp in hps:
        torch.manual_seed(MODEL_SEED)
        model = M.senet(512, 4).to(dev)
        models.append(model)
        opts.append(_adam(model.parameters(), hp))
        g = torch.Generator()
        g.manual_seed(GEN_SEED)
        gens.append(g)
    args = H.make_args(C_, j, K)
    losses = []
    for _ in range(epochs):
        rs = M.train_runs(models, [split] * len(hps), opts, dev, args, generators=gens, per_run_adam=per_run_adam)
        torch.cuda.synchronize()
        losses.append(rs.losses().cpu().numpy().copy())
    return dict(rs=rs, models=models, opts=opts, losses=losses)


def _bits(got, r):
    return (H.flat_params(got["models"][r]), H.flat_state(got["opts"][r], "exp_avg"), H.flat_state(got["opts"][r], "exp_avg_sq"))


def _assert_run(got, r, alone, what):
    p, m, v = _bits(got, r)
    np.testing.assert_array_equal(p, alone["p"], err_msg=f"{what}: parameters")
    np.testing.assert_array_equal(m, alone["m"], err_msg=f"{what}: exp_avg")
    np.testing.assert_array_equal(v, alone["v"], err_msg=f"{what}: exp_avg_sq")
    for e in range(EPOCHS):
        np.testing.assert_array_equal(got["losses"][e][r], alone["losses"][e], err_msg=f"{what}: losses of pass {e}")
    assert all(int(float(got["opts"][r].state[q]["step"])) == EPOCHS * len(SIZES) for q in got["models"][r].parameters())


def test_every_cell_of_a_lockstep_chain_is_its_run_alone(dev, monkeypatch):
    monkeypatch.delenv("MOC_RUNS_GROUPS", raising=False)
    monkeypatch.delenv("MOC_RUNS_SHARE", raising=False)
    got = _grid(dev, GRID)
    rs = got["rs"]
    assert rs.mode == 1 and len(rs.groups) == 1 and rs.groups[0]["runs"].n_runs == 4       # one launch pair per step
    assert rs.trained_phase_a == {"slides": 12, "scored_slides": 3, "shared_slides": 9}     # one mask group
    for r, (lr, wd) in enumerate(GRID):
        _assert_run(got, r, _alone(dev, lr, wd), f"run {r} lr {lr} wd {wd}")
    for a, b in zip(_bits(got, 0), _bits(got, 3)):                                         # the two equal cells
        np.testing.assert_array_equal(a, b)
    for r, s in ((0, 1), (0, 2), (1, 2)):                                                  # ... and cells that differ, differ
        assert not np.array_equal(_bits(got, r)[0], _bits(got, s)[0]), (r, s)
        assert not np.array_equal(_bits(got, r)[2], _bits(got, s)[2]), (r, s)


FULL = [(1e-3, (0.9, 0.999), 1e-8, 1e-4), (3e-4, (0.8, 0.99), 1e-6, 1e-2), (3e-3, (0.95, 0.9999), 1e-7, 0.0)]


def test_runs_with_their_own_betas_and_eps_are_their_runs_alone(dev, monkeypatch):
    """Three runs in one lockstep chain whose records differ in every field -- betas and eps too, which no other GPU test
    moves off torch's defaults: run r > 0 must read ITS beta1 / beta2 / eps (test_gpu_adam.py anchors the run alone to the
    update's arithmetic)."""
    monkeypatch.delenv("MOC_RUNS_GROUPS", raising=False)
    monkeypatch.delenv("MOC_RUNS_SHARE", raising=False)
    got = _grid(dev, FULL)
    rs = got["rs"]
    assert rs.mode == 1 and rs.per_run_adam and len(rs.groups) == 1 and rs.groups[0]["runs"].n_runs == 3
    for r, (lr, betas, eps, wd) in enumerate(FULL):
        _assert_run(got, r, _alone(dev, lr, wd, betas=betas, eps=eps), f"run {r} lr {lr} betas {betas} eps {eps} wd {wd}")
    for r, s in ((0, 1), (0, 2), (1, 2)):
        for a, b in zip(_bits(got, r), _bits(got, s)):
            assert not np.array_equal(a, b), (r, s)


@pytest.mark.parametrize("groups_env,n_groups", [(None, 2), ("1", 1)])
def test_a_chain_cut_in_two_keeps_every_run_s_own_record(dev, monkeypatch, groups_env, n_groups):
    """Nine cells: two chains of 5 + 4 (the second chain's records start at run 5, not at run 0); with MOC_RUNS_GROUPS=1 one
    call of nine runs, whose step the library issues as launches of 5 + 4 runs (eight coefficient entries per launch)."""
    monkeypatch.delenv("MOC_RUNS_SHARE", raising=False)
    if groups_env is None:
        monkeypatch.delenv("MOC_RUNS_GROUPS", raising=False)
    else:
        monkeypatch.setenv("MOC_RUNS_GROUPS", groups_env)
    got = _grid(dev, NINE)
    rs = got["rs"]
    assert rs.mode == 1 and [g["runs"].n_runs for g in rs.groups] == ([5, 4] if n_groups == 2 else [9])
    assert [g["r0"] for g in rs.groups] == ([0, 5] if n_groups == 2 else [0])
    for r, (lr, wd) in enumerate(NINE):
        _assert_run(got, r, _alone(dev, lr, wd), f"run {r} lr {lr}")


def test_wide_bank_runs_take_their_own_record(dev, monkeypatch):
    monkeypatch.delenv("MOC_RUNS_GROUPS", raising=False)
    monkeypatch.delenv("MOC_RUNS_SHARE", raising=False)
    hps = [(1e-3, 1e-4), (3e-3, 0.0), (3e-4, 1e-2)]
    got = _grid(dev, hps, C_=30, dtype=torch.bfloat16, j=40)
    rs = got["rs"]
    assert rs.mode == 2 and len(rs.groups) == 3
    for r, (lr, wd) in enumerate(hps):
        _assert_run(got, r, _alone(dev, lr, wd, C_=30, dtype=torch.bfloat16, j=40), f"run {r} lr {lr} wd {wd}")
    assert not np.array_equal(_bits(got, 0)[0], _bits(got, 1)[0])


def test_the_old_entry_and_the_new_one_agree_on_equal_hyper_parameters(dev, monkeypatch):
    monkeypatch.delenv("MOC_RUNS_GROUPS", raising=False)
    monkeypatch.delenv("MOC_RUNS_SHARE", raising=False)
    hps = [(1e-3, 1e-4)] * 4
    old = _grid(dev, hps, per_run_adam=False)
    new = _grid(dev, hps, per_run_adam=True)
    assert not old["rs"].per_run_adam and new["rs"].per_run_adam and len(old["rs"].groups) == len(new["rs"].groups) == 1
    alone = _alone(dev, 1e-3, 1e-4)
    for r in range(4):
        for a, b in zip(_bits(old, r), _bits(new, r)):
            np.testing.assert_array_equal(a, b)
        for e in range(EPOCHS):
            np.testing.assert_array_equal(old["losses"][e][r], new["losses"][e][r])
        _assert_run(old, r, alone, f"old entry, run {r}")


def test_a_hyper_parameter_edit_between_passes_is_seen(dev, monkeypatch):
    """The param groups are read at every train_pass: halving run 1's learning rate after pass 0 is what the run alone
    does when its caller halves it there."""
    monkeypatch.delenv("MOC_RUNS_GROUPS", raising=False)
    from moc_amd import main_moc as M
    W, We = _bank(2)
    M.set_classifier_bank(W.to(dev), We.to(dev))
    bags, labels = _bags(2, torch.float32)
    torch.manual_seed(MODEL_SEED)
    model = M.senet(512, 4).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=3e-3, weight_decay=0.0)
    res = M.ResidentBags(bags, labels, dev)
    torch.manual_seed(GEN_SEED)
    for e in range(EPOCHS):
        M.train(model, res, opt, dev, H.make_args(2, 100, 5))
        opt.param_groups[0]["lr"] = 1.5e-3
    torch.cuda.synchronize()
    split = M.ResidentBags(bags, labels, dev)
    models, opts, gens = [], [], []
    for lr, wd in GRID[:2]:
        torch.manual_seed(MODEL_SEED)
        models.append(M.senet(512, 4).to(dev))
        opts.append(torch.optim.Adam(models[-1].parameters(), lr=lr, weight_decay=wd))
        gens.append(torch.Generator().manual_seed(GEN_SEED))
    for e in range(EPOCHS):
        M.train_runs(models, [split, split], opts, dev, H.make_args(2, 100, 5), generators=gens, per_run_adam=True)
        opts[1].param_groups[0]["lr"] = 1.5e-3
    torch.cuda.synchronize()
    np.testing.assert_array_equal(H.flat_params(models[1]), H.flat_params(model))
    np.testing.assert_array_equal(H.flat_state(opts[1], "exp_avg_sq"), H.flat_state(opt, "exp_avg_sq"))
    np.testing.assert_array_equal(H.flat_params(models[0]), _alone(dev, *GRID[0])["p"])


def test_weight_decay_zero_and_another_learning_rate_against_the_cpu_oracle(dev, monkeypatch):
    """Three steps of the run at (3e-3, 0) -- run 1 of two, so that its record is not the first -- against the oracle's
    train_step with torch.optim.Adam on the CPU, from the same initial parameters and the same masks.  The tolerances are
    test_gpu_parity.test_train_steps_match_reference_fixtures' for train.npz: assert_adam_params_close with grad_noise 1e-6
    (its `lr` is the run's learning rate: an element whose gradient is within the noise moves by up to lr per step),
    exp_avg to 1e-6 x steps, exp_avg_sq to 1e-8, the losses to helpers.ATOL."""
    monkeypatch.delenv("MOC_RUNS_GROUPS", raising=False)
    lr, wd = 3e-3, 0.0
    W, We = _bank(2)
    bags, labels = _bags(2, torch.float32)
    torch.manual_seed(MODEL_SEED)
    ref = O.Senet(512, 4)
    ref_opt = torch.optim.Adam(ref.parameters(), lr=lr, weight_decay=wd)
    torch.manual_seed(GEN_SEED)                                 # (the oracle draws its masks from the default generator)
    ref_losses = O.train_epoch(ref, ref_opt, bags, labels, W, We, 2, 100, 5)
    got = _grid(dev, [(1e-3, 1e-4), (lr, wd)], epochs=1)
    steps = len(SIZES)
    p, m, v = _bits(got, 1)
    d = np.abs(p.astype(np.float64) - H.flat_params(ref))
    print(f"worst parameter difference after {steps} steps: {d.max():.3e}; exp_avg {np.abs(m - H.flat_state(ref_opt, 'exp_avg')).max():.3e}; "
          f"exp_avg_sq {np.abs(v - H.flat_state(ref_opt, 'exp_avg_sq')).max():.3e}; "
          f"loss {np.abs(got['losses'][0][1] - np.asarray(ref_losses)).max():.3e}")
    H.assert_adam_params_close(p, H.flat_params(ref), H.flat_state(ref_opt, "exp_avg_sq"), step=steps, grad_noise=1e-6, lr=lr,
                               what="(3e-3, 0) after three steps")
    np.testing.assert_allclose(m, H.flat_state(ref_opt, "exp_avg"), atol=1e-6 * steps)
    np.testing.assert_allclose(v, H.flat_state(ref_opt, "exp_avg_sq"), atol=1e-8)
    np.testing.assert_allclose(got["losses"][0][1], np.asarray(ref_losses), atol=H.ATOL)
    # without weight decay a parameter whose gradient was zero in all three steps has not moved at all
    init = H.flat_params(H.seeded_senet(O, MODEL_SEED))
    still = v == 0
    assert np.array_equal(p[still], init[still])


def test_bad_records_are_runtime_errors_and_launch_nothing(dev, monkeypatch):
    monkeypatch.delenv("MOC_RUNS_GROUPS", raising=False)
    from moc_amd import runs
    got = _grid(dev, GRID[:2], epochs=1)
    rs = got["rs"]
    grp, batch = rs.groups[0], rs.last[0]
    ws0 = batch.meta_ws()[1]
    ws = type(ws0).from_buffer_copy(ws0)
    ws.W2_alt = grp["w2alt"]
    before = [b.copy() for r in range(2) for b in _bits(got, r)]
    good = (1e-3, 0.9, 0.999, 1e-8, 1e-4)

    def call(records):
        runs.steps_runs_hp(batch.c, grp["meta"], grp["runs"], ws, rs.labels.data_ptr(), grp["slide0"], grp["n"], grp["use"],
                           records, None)
    with pytest.raises(RuntimeError, match="moc_train_steps_runs_hp: null hyper-parameter records"):
        call(None)
    with pytest.raises(RuntimeError, match=r"run 1: lr = nan \(finite, >= 0\)"):
        call(runs.hp_records([good, (float("nan"),) + good[1:]]))
    with pytest.raises(RuntimeError, match=r"run 0: beta1 = 1 \(0 <= beta < 1\)"):
        call(runs.hp_records([good[:1] + (1.0,) + good[2:], good]))
    with pytest.raises(RuntimeError, match=r"run 1: weight_decay = -0.0001 \(finite, >= 0\)"):
        call(runs.hp_records([good, good[:4] + (-1e-4,)]))
    torch.cuda.synchronize()
    after = [b for r in range(2) for b in _bits(got, r)]
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


def test_driver_grid_reproduces_every_cell_s_own_command(dev, tmp_path, monkeypatch):
    """`run_moc --seeds 3,4 --lrs 1e-3,3e-3 --wds 0,1e-4 --folds 0,1`: eight cell directories; two cells that differ in all
    three axes hold what their own single command writes, the best checkpoints the same bits; the summary has a line per
    (lr, wd); the (lr, wd) cells of a (seed, fold) are scored once."""
    monkeypatch.delenv("MOC_RUNS_GROUPS", raising=False)
    monkeypatch.delenv("MOC_RUNS_SHARE", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    from moc_amd import main_moc as M, run_moc
    common = ["--synthetic", "6", "--shot", "2", "--epochs", "3", "--topj", "100", "--topk", "10", "--disable_tqdm"]
    grid = run_moc.cli(common + ["--folds", "0,1", "--seeds", "3,4", "--lrs", "1e-3,3e-3", "--wds", "0,1e-4",
                                 "--result_dir", str(tmp_path / "grid")])
    assert len(grid) == 16
    # 16 runs x 4 visits; a mask group per (seed, fold): 2 x 2 x 4 slides are scored, a quarter of all
    assert M.train_runs.last.trained_phase_a == {"slides": 64, "scored_slides": 16, "shared_slides": 48}
    assert M.train_runs.last.per_run_adam and all(g["runs"].n_runs == 8 for g in M.train_runs.last.groups)
    dirs = sorted(p.name for p in (tmp_path / "grid").iterdir() if p.is_dir())
    assert dirs == sorted(f"seed{s}_lr{lr}_wd{wd}" for s in (3, 4) for lr in ("0.001", "0.003") for wd in ("0", "0.0001"))
    for seed, lr, wd, fold in ((3, "1e-3", "0", 0), (4, "3e-3", "1e-4", 1)):
        sub = f"seed{seed}_lr{format(float(lr), 'g')}_wd{format(float(wd), 'g')}"
        run_moc.cli(common + ["--fold", str(fold), "--seed", str(seed), "--lr", lr, "--weight_decay", wd,
                              "--result_dir", str(tmp_path / "alone" / sub)])
        for stem in (f"zs_results_shot_2_fold_{fold}.json", f"best_results_shot_2_fold_{fold}.json"):
            a = json.load(open(tmp_path / "alone" / sub / stem))
            b = json.load(open(tmp_path / "grid" / sub / stem))
            a.pop("best_model_path", None)
            assert b.pop("best_model_path", None) in (None, str(tmp_path / "grid" / sub / f"best_model_shot_2_fold_{fold}.pt"))
            assert a == b, (sub, fold, stem, a, b)
        sa = torch.load(tmp_path / "alone" / sub / f"best_model_shot_2_fold_{fold}.pt", map_location="cpu")
        sb = torch.load(tmp_path / "grid" / sub / f"best_model_shot_2_fold_{fold}.pt", map_location="cpu")
        assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa), (sub, fold)
        assert sorted(p.name for p in (tmp_path / "grid" / sub).iterdir()) == sorted(
            f"{stem}_shot_2_fold_{f}.{ext}" for stem, ext in (("zs_results", "json"), ("best_results", "json"), ("best_model", "pt"))
            for f in (0, 1))
    table = open(tmp_path / "grid" / "opt_grid_summary.csv").read().splitlines()
    assert table[0].startswith("lr,weight_decay,runs,") and len(table) == 5
    assert [ln.split(",")[:3] for ln in table[1:]] == [["0.001", "0", "4"], ["0.001", "0.0001", "4"], ["0.003", "0", "4"], ["0.003", "0.0001", "4"]]
    for ln in table[1:]:
        lr, wd = ln.split(",")[:2]
        vals = [json.load(open(tmp_path / "grid" / f"seed{s}_lr{lr}_wd{wd}" / f"best_results_shot_2_fold_{f}.json"))
                for s in (3, 4) for f in (0, 1)]
        np.testing.assert_allclose([float(x) for x in ln.split(",")[3:]],
                                   [np.mean([v["best_val"] for v in vals]), np.std([v["best_val"] for v in vals]),
                                    np.mean([v["test_at_best_val"] for v in vals]), np.std([v["test_at_best_val"] for v in vals])],
                                   rtol=1e-12, atol=0)
