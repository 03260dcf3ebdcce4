"""A shots x folds grid in one process: runs of unequal pass length trained in lockstep chains (moc_amd.runs), all runs
evaluated in one pass (main_moc.evaluation_runs), and `run_moc --shots a,b --folds c,d` against the single commands.
Per run everything is BIT-identical to the run alone (main_moc.train / main_moc.evaluation)."""
import json
import os

import numpy as np
import pytest
import torch

import helpers as H
from moc_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(gpu_device):
    return gpu_device


def _task(run, n, C, D, dtype, lo=1200, hi=3000):
    W, We = synth.make_bank(31 + C, D, C)                       # the runs share the classifier bank
    g = np.random.default_rng(500 + run)
    sizes = [int(v) for v in g.integers(lo, hi, size=n)]
    bags, labels = synth.make_slide_set(9000 + 37 * run, sizes, D, We, C)
    return W, We, [b.to(dtype) for b in bags], labels


def _alone(dev, run, n, C, D, dtype, j, K, epochs):
    from moc_amd import main_moc as M
    W, We, bags, labels = _task(run, n, C, D, dtype)
    M.set_classifier_bank(W.to(dev), We.to(dev))
    torch.manual_seed(100 + run)
    model = M.senet(D, 4).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
    res = M.ResidentBags(bags, labels, dev)
    args = H.make_args(C, j, K, ())
    torch.manual_seed(7000 + run)                               # the run's mask stream
    losses = []
    for _ in range(epochs):
        M.train(model, res, opt, dev, args)
        torch.cuda.synchronize()
        losses.append(M.train.last[0].meta_ws()[0]["loss"].cpu().numpy().copy())
    return (H.flat_params(model), H.flat_state(opt, "exp_avg"), H.flat_state(opt, "exp_avg_sq"), losses,
            torch.get_rng_state().clone())


@pytest.mark.parametrize("lengths,C,D,dtype,j,K", [
    ((2, 4, 8, 4, 2, 8), 2, 512, torch.float32, 300, 10),       # three pass lengths, not sorted: six chains of one run
    ((2, 2, 2, 4, 4, 8), 2, 512, torch.float32, 300, 10),       # sorted, as the driver orders them: chains of 3, 2 and 1
    ((2, 2, 4, 4, 8), 3, 512, torch.bfloat16, 200, 10),
    ((2, 3, 2), 30, 512, torch.bfloat16, 40, 10),               # wide bank (mode 2): every run a chain of its own
])
def test_unequal_runs_are_each_the_run_alone_bit_for_bit(dev, lengths, C, D, dtype, j, K):
    from moc_amd import main_moc as M
    R, epochs = len(lengths), 3
    alone = [_alone(dev, r, lengths[r], C, D, dtype, j, K, epochs) for r in range(R)]
    models, opts, splits, gens = [], [], [], []
    for r in range(R):
        W, We, bags, labels = _task(r, lengths[r], C, D, dtype)
        M.set_classifier_bank(W.to(dev), We.to(dev))
        torch.manual_seed(100 + r)
        model = M.senet(D, 4).to(dev)
        models.append(model)
        opts.append(torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4))
        splits.append(M.ResidentBags(bags, labels, dev))
        g = torch.Generator()
        g.manual_seed(7000 + r)
        gens.append(g)
    args = H.make_args(C, j, K, ())
    losses = []
    for _ in range(epochs):
        rs = M.train_runs(models, splits, opts, dev, args, generators=gens)
        torch.cuda.synchronize()
        losses.append([t.cpu().numpy().copy() for t in rs.losses()])
    assert rs.mode == (1 if C <= 16 else 2)
    assert sorted(r for g in rs.groups for r in range(g["r0"], g["r0"] + g["runs"].n_runs)) == list(range(R))
    assert all(lengths[r] == g["n"] for g in rs.groups for r in range(g["r0"], g["r0"] + g["runs"].n_runs))
    if C <= 16 and list(lengths) == sorted(lengths):            # one chain per pass length, several runs in lockstep
        assert sorted(g["runs"].n_runs for g in rs.groups) == sorted(lengths.count(n_) for n_ in set(lengths))
    for r in range(R):
        p, m, v, ls, rng = alone[r]
        np.testing.assert_array_equal(H.flat_params(models[r]), p, err_msg=f"run {r}: parameters")
        np.testing.assert_array_equal(H.flat_state(opts[r], "exp_avg"), m, err_msg=f"run {r}: exp_avg")
        np.testing.assert_array_equal(H.flat_state(opts[r], "exp_avg_sq"), v, err_msg=f"run {r}: exp_avg_sq")
        for e in range(epochs):
            np.testing.assert_array_equal(losses[e][r], ls[e], err_msg=f"run {r} pass {e}: losses")
        assert all(int(float(opts[r].state[q]["step"])) == epochs * lengths[r] for q in models[r].parameters())
        # the run's generator continues the stream where the default generator stands after the run alone (TrainRuns has
        # drawn the flags of one more pass ahead, from the same stream): compare what each would draw next with a replay
        # of `torch.rand(N) > 0.5` from the run's seed
        rows = sum(splits[r].sizes[k] for k in splits[r].visit_order())
        g = torch.Generator()
        g.manual_seed(7000 + r)
        torch.rand(epochs * rows, generator=g)
        after_alone = torch.Generator()
        after_alone.set_state(rng)
        g1 = torch.Generator()
        g1.set_state(g.get_state())
        assert torch.equal(torch.rand(256, generator=after_alone), torch.rand(256, generator=g1)), f"run {r}: the run alone"
        torch.rand(rows, generator=g)
        g2 = torch.Generator()
        g2.set_state(gens[r].get_state())
        assert torch.equal(torch.rand(256, generator=g2), torch.rand(256, generator=g)), f"run {r}: generator state"


def _pooled_alone(M, model, loader, dev, args):
    ev = M.evaluation(model, loader, dev, args)
    keep, loader.repeat_num = loader.repeat_num, loader.real_len()          # (the pass evaluation() made: every slide once)
    try:
        plan = loader.eval_plan(args.n_classes, M.zeroshot_weights_ext.size(1), args.topj, args.topk, args.discard_classifiers)
    finally:
        loader.repeat_num = keep
    return ev, plan["batch"].meta_ws()[0]["pooled"].cpu().clone()


@pytest.mark.parametrize("dtype,C", [(torch.float32, 2), (torch.bfloat16, 3)])
def test_evaluation_runs_is_evaluation_per_run(dev, dtype, C, monkeypatch):
    from moc_amd import main_moc as M
    D, j, K = 512, 200, 10
    lengths = (4, 7, 5)                                         # splits of different sizes
    R = len(lengths)
    args = H.make_args(C, j, K, ())
    models, opts, trains, evals = [], [], [], []
    for r in range(R):
        W, We, bags, labels = _task(r, lengths[r], C, D, dtype)
        M.set_classifier_bank(W.to(dev), We.to(dev))
        torch.manual_seed(100 + r)
        model = M.senet(D, 4).to(dev)
        models.append(model)
        opts.append(torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4))
        trains.append(M.ResidentBags(bags, labels, dev, repeat_num=lengths[r] + 1))
        _, _, vb, vl = _task(40 + r, lengths[r] + 3, C, D, dtype)
        evals.append(M.ResidentBags(vb, vl, dev))

    def compare(ms, lds, want=None):
        want = want or [_pooled_alone(M, m, ld, dev, args) for m, ld in zip(ms, lds)]
        reps = [ld.repeat_num for ld in lds]
        got = M.evaluation_runs(ms, lds, dev, args)
        assert [ld.repeat_num for ld in lds] == reps            # restored as evaluation restores it
        for r, (ev, pooled) in enumerate(want):
            assert got[r] == ev, (r, got[r], ev)                 # loss, acc, auc: the same Python floats
            assert torch.equal(M.evaluation_runs.last_pooled[r].view(torch.int32), pooled.view(torch.int32)), f"run {r}: pooled logits"

    compare(models, evals)                                      # fresh models: a scratch arena
    compare(models + models, trains + evals)                    # a model named twice; visits that wrap around (repeat_num)
    gens = []
    for r in range(R):
        g = torch.Generator()
        g.manual_seed(7000 + r)
        gens.append(g)
    for _ in range(2):                                          # after some training: the parameters lie in TrainRuns' arena
        M.train_runs(models, trains, opts, dev, args, generators=gens)
    from moc_amd import engine
    assert engine.ModelArena.of_models(models).P is None        # (used in place)
    compare(models + models, trains + evals)
    # a batch limit small enough to force several chunks, each of which may hold slides of several runs
    want = [_pooled_alone(M, m, ld, dev, args) for m, ld in zip(models, evals)]
    monkeypatch.setattr(M, "MAX_BATCH_BYTES", 3 * 3000 * D * torch.empty((), dtype=dtype).element_size())
    compare(models, evals, want)
    assert [M.evaluation(m, ld, dev, args) for m, ld in zip(models, evals)] == [w[0] for w in want]
    plan = [p for k, p in M._eval_run_plans.items() if k[-3] == M.MAX_BATCH_BYTES][-1]
    assert len(plan["chunks"]) > 1
    monkeypatch.undo()
    # refusals
    loud = M.ResidentBags(vb, vl, dev, loader_seed_draw=True)
    with pytest.raises(AssertionError, match="loader_seed_draw"):
        M.evaluation_runs(models[:1], [loud], dev, args)
    with pytest.raises(AssertionError, match="resident"):
        M.evaluation_runs(models[:1], [[1, 2]], dev, args)
    with pytest.raises(AssertionError, match="width"):
        M.evaluation_runs([models[0], M.senet(1024, 4).to(dev)], evals[:2], dev, args)


def test_a_grid_in_one_process_reproduces_every_single_command(dev, tmp_path):
    """`run_moc --shots 1,4 --folds 0,1`: every run's files are those of `--fold F --shot S --result_dir <dir>/<S>_shot`
    alone, the best checkpoints the same bits, and --summary reads the tree."""
    from moc_amd import run_moc
    common = ["--synthetic", "6", "--seed", "1", "--epochs", "4", "--topj", "100", "--topk", "10", "--disable_tqdm"]
    grid = run_moc.cli(common + ["--shots", "1,4", "--folds", "0,1", "--result_dir", str(tmp_path / "grid")])
    assert len(grid) == 4
    for shot in (1, 4):
        for fold in (0, 1):
            alone = run_moc.cli(common + ["--fold", str(fold), "--shot", str(shot), "--result_dir", str(tmp_path / "alone" / f"{shot}_shot")])
            for name in (f"zs_results_shot_{shot}_fold_{fold}.json", f"best_results_shot_{shot}_fold_{fold}.json"):
                a = json.load(open(tmp_path / "alone" / f"{shot}_shot" / name))
                b = json.load(open(tmp_path / "grid" / f"{shot}_shot" / name))
                a.pop("best_model_path", None)
                assert b.pop("best_model_path", None) in (None, str(tmp_path / "grid" / f"{shot}_shot" / f"best_model_shot_{shot}_fold_{fold}.pt"))
                assert a == b, (shot, fold, name, a, b)
            assert alone["best_val"] == json.load(open(tmp_path / "grid" / f"{shot}_shot" / f"best_results_shot_{shot}_fold_{fold}.json"))["best_val"]
            sa = torch.load(tmp_path / "alone" / f"{shot}_shot" / f"best_model_shot_{shot}_fold_{fold}.pt", map_location="cpu")
            sb = torch.load(tmp_path / "grid" / f"{shot}_shot" / f"best_model_shot_{shot}_fold_{fold}.pt", map_location="cpu")
            assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)
    # --summary reads <dir>/<shot>_shot/best_results_shot_<shot>_fold_<0..4>.json: give it the three other folds of shot 1
    run_moc.cli(common + ["--shots", "1", "--folds", "2,3,4", "--result_dir", str(tmp_path / "grid")])
    run_moc.cli(["--summary", "--summary_dir", str(tmp_path / "grid")])
    table = open(tmp_path / "grid" / "summary_1.csv").read().splitlines()
    assert table[0].startswith("fold,test_auc") and len(table) == 7
