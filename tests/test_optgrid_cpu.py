"""Optimizer grids without a GPU: the driver's --lr / --weight_decay / --seeds / --lrs / --wds flags,
the cell order, the directories, the refusals, opt_grid_summary.csv, and the declaration, export and binding of
moc_train_steps_runs_hp with its argument checks."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(*argv):
    from moc_amd import run_moc
    return run_moc.get_args(list(argv))


def test_entry_is_declared_exported_and_bound_and_the_abi_stays_20():
    from moc_amd import _lib
    src = open(os.path.join(ROOT, "include", "moc_hip.h")).read()
    assert re.search(r"int\s+moc_train_steps_runs_hp\s*\(", src) and "#define MOC_ABI_VERSION 20" in src
    assert re.search(r"double\s+lr,\s*beta1,\s*beta2,\s*eps,\s*weight_decay;\s*\}\s*moc_adam_hp_t", src)
    assert "moc_train_steps_runs_hp" in _lib.SIGNATURES and _lib.ABI_VERSION == 20
    assert "moc_train_steps_runs_hp" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    h = _lib.lib()
    assert hasattr(h, "moc_train_steps_runs_hp") and h.moc_version() == 20
    # the record: five doubles, in the header's order
    assert ctypes.sizeof(_lib.MocAdamHp) == 40
    assert [n for n, _ in _lib.MocAdamHp._fields_] == ["lr", "beta1", "beta2", "eps", "weight_decay"]


def test_hp_records_are_what_the_library_reads():
    from moc_amd import runs
    recs = runs.hp_records([(1e-3, 0.9, 0.999, 1e-8, 1e-4), (3e-3, 0.8, 0.99, 1e-6, 0.0)])
    assert len(recs) == 2 and (recs[1].lr, recs[1].beta1, recs[1].beta2, recs[1].eps, recs[1].weight_decay) == (3e-3, 0.8, 0.99, 1e-6, 0.0)
    assert runs.adam_hp({"lr": 3e-4, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0}) == (3e-4, 0.9, 0.999, 1e-8, 0.0)


def test_bad_records_are_refused_before_any_launch():
    """The record checks come first: nothing else of the call is looked at, nothing is launched (no GPU here)."""
    from moc_amd import _lib, runs
    h = _lib.lib()
    b, m, w = _lib.MocBatch(), _lib.MocMeta(), _lib.MocMetaWs()
    R = _lib.MocRuns(n_runs=2, slide_stride=3, par_stride=1 << 16, image_stride=1 << 20)
    good = (1e-3, 0.9, 0.999, 1e-8, 1e-4)

    def call(records, runs_c=R):
        return h.moc_train_steps_runs_hp(ctypes.byref(b), ctypes.byref(m), ctypes.byref(runs_c), ctypes.byref(w), None, 0, 3, 15,
                                         records, None)
    assert call(None) == 1 and b"moc_train_steps_runs_hp: null hyper-parameter records" in h.moc_last_error()
    for bad, text in (((float("nan"),) + good[1:], b"run 1: lr"), ((float("inf"),) + good[1:], b"run 1: lr"),
                      ((-1e-3,) + good[1:], b"run 1: lr"), (good[:1] + (1.0,) + good[2:], b"run 1: beta1"),
                      (good[:2] + (-0.1,) + good[3:], b"run 1: beta2"), (good[:3] + (float("nan"),) + good[4:], b"run 1: eps"),
                      (good[:4] + (-1e-4,), b"run 1: weight_decay"), (good[:4] + (float("inf"),), b"run 1: weight_decay")):
        assert call(runs.hp_records([good, bad])) == 1 and text in h.moc_last_error(), (bad, h.moc_last_error())
    # records past n_runs are not read; good records get as far as the checks moc_train_steps_runs makes
    one = _lib.MocRuns(n_runs=1, slide_stride=3, par_stride=1 << 16, image_stride=1 << 20)
    assert call(runs.hp_records([good, (float("nan"),) * 5]), one) == 1 and b"moc_train_steps_runs_hp: null X/row_off" in h.moc_last_error()
    assert call(runs.hp_records([good]), _lib.MocRuns(n_runs=17)) == 1 and b"1 .. 16 runs" in h.moc_last_error()
    with pytest.raises(RuntimeError, match="null hyper-parameter records"):
        runs.steps_runs_hp(b, m, R, w, None, 0, 3, 15, None, None)
    # the old entry's refusals keep their text
    assert h.moc_train_steps_runs(ctypes.byref(b), ctypes.byref(m), ctypes.byref(R), ctypes.byref(w), None, 0, 3, 15, None) == 1
    assert b"moc_train_steps_runs: null X/row_off" in h.moc_last_error()


def test_single_run_flags_default_to_the_reference_constants():
    a = _args()
    assert a.lr == 1e-3 and a.weight_decay == 1e-4 and a.seeds is None and a.lrs is None and a.wds is None
    b = _args("--lr", "3e-3", "--weight_decay", "0")
    assert b.lr == 3e-3 and b.weight_decay == 0.0
    from moc_amd import run_moc
    assert not run_moc.optgrid_requested(a) and not run_moc.optgrid_requested(b)
    run_moc.check_optgrid_args(_args("--shots", "1,2", "--patch_maps", "test"))      # not a grid: not this function's business
    # the constants are gone from where the driver builds Adam
    src = open(os.path.join(ROOT, "moc_amd", "run_moc.py")).read()
    assert "lr=1e-3, weight_decay=1e-4" not in src and src.count("lr=args.lr, weight_decay=args.weight_decay") == 3


def test_cells_are_seed_major_then_lr_then_wd():
    from moc_amd import run_moc
    a = _args("--seeds", "1,2,3", "--lrs", "3e-4,1e-3,3e-3", "--wds", "0,1e-4", "--folds", "0,1", "--result_dir", "out")
    assert run_moc.optgrid_requested(a)
    cells = run_moc.optgrid_cells(a)
    assert len(cells) == 18
    assert cells[:7] == [(1, 3e-4, 0.0), (1, 3e-4, 1e-4), (1, 1e-3, 0.0), (1, 1e-3, 1e-4), (1, 3e-3, 0.0), (1, 3e-3, 1e-4), (2, 3e-4, 0.0)]
    assert cells[-1] == (3, 3e-3, 1e-4)
    # a list that is not given is the single flag's value
    b = _args("--lrs", "1e-3,3e-3", "--seed", "7", "--weight_decay", "1e-2")
    assert run_moc.optgrid_cells(b) == [(7, 1e-3, 1e-2), (7, 3e-3, 1e-2)]
    c = _args("--seeds", "4,5")
    assert run_moc.optgrid_cells(c) == [(4, 1e-3, 1e-4), (5, 1e-3, 1e-4)]
    assert run_moc.optgrid_cells(_args("--wds", "0", "--seed", "1", "--lr", "2e-3")) == [(1, 2e-3, 0.0)]
    run_moc.check_optgrid_args(a)                                # nothing to refuse
    # the runs: cells in order, fold-major inside one; every run carries its cell's seed / lr / weight_decay and directory
    runs = run_moc.optgrid_runs(a, cells[:2], [0, 1])
    assert [(r.seed, r.lr, r.weight_decay, r.fold) for r in runs] == [(1, 3e-4, 0.0, 0), (1, 3e-4, 0.0, 1), (1, 3e-4, 1e-4, 0), (1, 3e-4, 1e-4, 1)]
    assert runs[2].result_dir == os.path.join("out", "seed1_lr0.0003_wd0.0001") and a.result_dir == "out" and a.seed is None


def test_directory_names():
    from moc_amd import run_moc
    assert run_moc.optgrid_dir("out", (1, 3e-5, 0.0)) == os.path.join("out", "seed1_lr3e-05_wd0")
    assert run_moc.optgrid_dir("out", (12, 1e-3, 1e-4)) == os.path.join("out", "seed12_lr0.001_wd0.0001")
    assert run_moc.optgrid_dir("out", (3, 3e-3, 1e-2)) == os.path.join("out", "seed3_lr0.003_wd0.01")
    assert run_moc.optgrid_dir("r", (0, 1.0, 0)) == os.path.join("r", "seed0_lr1_wd0")


@pytest.mark.parametrize("argv,message", [
    (["--lrs", "1e-3,3e-3", "--seed", "1", "--shots", "1,2"], "do not combine with --shots"),
    (["--seeds", "1,2", "--topjs", "50,100"], "do not combine with --topjs / --topks / --discard_sets"),
    (["--seeds", "1,2", "--topks", "5,10"], "do not combine with --topjs / --topks / --discard_sets"),
    (["--wds", "0,1e-4", "--seed", "1", "--discard_sets", "none", "topk"], "do not combine with --topjs / --topks / --discard_sets"),
    (["--seeds", "1,2", "--patch_maps", "test"], "do not combine with --patch_maps"),
    (["--seeds", "1,2", "--patch_maps_from", "best.pt"], "do not combine with --patch_maps"),
    (["--lrs", "1e-3", "--seed", "1", "--loader_seed_draw", "1"], "do not combine with --loader_seed_draw"),
    (["--wds", "0", "--seed", "1", "--ablation_study", "avg"], "do not combine with --ablation_study"),
    (["--lrs", "1e-3,3e-3"], "--lrs / --wds need --seed or --seeds"),
    (["--seeds", ""], "--seeds: a non-empty list"),
    (["--seeds", "1,x"], "--seeds: not a comma-separated list"),
    (["--seeds", "1.5"], "--seeds: not a comma-separated list"),
    (["--lrs", ",", "--seed", "1"], "--lrs: a non-empty list"),
    (["--lrs", "1e-3,fast", "--seed", "1"], "--lrs: not a comma-separated list"),
    (["--lrs", "1e-3,1e-3", "--seed", "1"], "--lrs: a value named twice"),
    (["--lrs", "1e-3,-1e-3", "--seed", "1"], "--lrs: finite values >= 0"),
    (["--wds", "0,nan", "--seed", "1"], "--wds: finite values >= 0"),
    (["--seeds", "2,2"], "--seeds: a value named twice"),
])
def test_refusals_come_before_any_bag_is_loaded(argv, message, monkeypatch):
    from moc_amd import run_moc
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit, match=message):
        run_moc.check_optgrid_args(_args(*argv))
    with pytest.raises(SystemExit, match=message):               # cli() refuses the same way, before it looks for a GPU
        run_moc.cli(argv)


def test_a_launcher_is_refused(monkeypatch):
    from moc_amd import run_moc
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match=r"--seeds / --lrs / --wds are one-GPU options \(WORLD_SIZE > 1\)"):
        run_moc.check_optgrid_args(_args("--seeds", "1,2"))
    with pytest.raises(SystemExit, match="WORLD_SIZE > 1"):
        run_moc.cli(["--lrs", "1e-3,3e-3", "--seed", "1"])
    run_moc.check_optgrid_args(_args("--seed", "1", "--lr", "3e-3"))                 # single-run flags: no grid, no refusal


def test_more_than_32_runs_train_in_blocks_of_whole_cells():
    from moc_amd import run_moc
    from moc_amd.runs import MAX_RUNS
    a = _args("--seeds", "1,2,3", "--lrs", "3e-4,1e-3,3e-3", "--wds", "0,1e-4")
    blocks = run_moc.hgrid_blocks(len(run_moc.optgrid_cells(a)), 5, MAX_RUNS)        # 18 cells x 5 folds
    assert blocks == [[0, 1, 2, 3, 4, 5], [6, 7, 8, 9, 10, 11], [12, 13, 14, 15, 16, 17]]


def test_chains_hold_the_cells_of_a_fold_and_keep_their_own_records():
    """The chain key has no (lr, wd) in it: nine cells of one fold are ONE group of runs, cut by the cap into 5 + 4 -- and
    the second chain's records must be those of runs 5 ... 8."""
    from moc_amd.runs import group_runs, hp_records
    keys = [(4, 0, (100, 5, 0))] * 9
    chains = group_runs(keys, 8)
    assert chains == [[0, 1, 2, 3, 4], [5, 6, 7, 8]]
    hps = [(1e-4 * (r + 1), 0.9, 0.999, 1e-8, 1e-4) for r in range(9)]
    second = hp_records([hps[r] for r in chains[1]])
    assert [rec.lr for rec in second] == [hps[r][0] for r in (5, 6, 7, 8)]


def test_summary_table_from_result_files(tmp_path):
    from moc_amd import run_moc
    cells = [(s, lr, wd) for s in (3, 4) for lr in (1e-3, 3e-5) for wd in (0.0, 1e-4)]
    folds, shot = [0, 2], 2
    rng = np.random.default_rng(5)
    vals = {}
    for cell in cells:
        d = run_moc.optgrid_dir(str(tmp_path), cell)
        os.makedirs(d)
        for fold in folds:
            vals[cell, fold] = (float(rng.uniform(0.5, 1)), float(rng.uniform(0.5, 1)))
            json.dump({"best_val": vals[cell, fold][0], "test_at_best_val": vals[cell, fold][1], "test_acc_at_best_val": 0.5,
                       "best_epoch": 1, "zero_shot_test": {"auc": 0.6, "acc": 0.5}},
                      open(os.path.join(d, f"best_results_shot_{shot}_fold_{fold}.json"), "w"))
    path = run_moc.write_optgrid_summary(str(tmp_path), cells, folds, shot)
    assert path == os.path.join(str(tmp_path), "opt_grid_summary.csv")
    lines = open(path).read().splitlines()
    assert lines[0] == "lr,weight_decay,runs,best_val_mean,best_val_std,test_auc_mean,test_auc_std" and len(lines) == 5
    for line, (lr, wd) in zip(lines[1:], [(1e-3, 0.0), (1e-3, 1e-4), (3e-5, 0.0), (3e-5, 1e-4)]):
        f = line.split(",")
        assert f[0] == format(lr, "g") and f[1] == format(wd, "g") and int(f[2]) == 4
        v = np.array([vals[(s, lr, wd), fold] for s in (3, 4) for fold in folds])
        np.testing.assert_allclose([float(x) for x in f[3:]], [v[:, 0].mean(), v[:, 0].std(), v[:, 1].mean(), v[:, 1].std()],
                                   rtol=1e-12, atol=0)
    assert lines[3].startswith("3e-05,0,4,")
