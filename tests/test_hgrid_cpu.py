"""Hyper-parameter grids without a GPU: the chain grouping with configurations in its keys, the mask groups, the driver's
flags, directories, refusals and blocks, and moc_stats_share's argument checks."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_declared_and_bound_and_the_abi_stays_20():
    from moc_amd import _lib
    src = open(os.path.join(ROOT, "include", "moc_hip.h")).read()
    assert re.search(r"int\s+moc_stats_share\s*\(", src) and "#define MOC_ABI_VERSION 20" in src
    assert "moc_stats_share" in _lib.SIGNATURES and _lib.ABI_VERSION == 20
    assert "moc_stats_share" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    h = _lib.lib()
    assert hasattr(h, "moc_stats_share") and h.moc_version() == 20
    assert "moc_share.hip" in open(os.path.join(ROOT, "moc_amd", "csrc", "Makefile")).read()


def test_stats_share_refuses_bad_arguments_before_any_launch():
    from moc_amd import _lib
    h = _lib.lib()
    b = _lib.MocBatch()
    lead = (ctypes.c_int32 * 4)(-1, 0, -1, -1)
    lp = ctypes.cast(lead, ctypes.c_void_p)
    assert h.moc_stats_share(None, lp, 0, 1, None) == 1 and b"null pointer" in h.moc_last_error()
    assert h.moc_stats_share(ctypes.byref(b), None, 0, 1, None) == 1 and b"null pointer" in h.moc_last_error()
    assert h.moc_stats_share(ctypes.byref(b), lp, 0, 1, None) == 1 and b"moc_stats_share: null X/row_off" in h.moc_last_error()
    # a batch that passes the common checks (the pointers are never followed on the host) but has no statistics
    off = (ctypes.c_int64 * 5)(0, 16, 32, 48, 64)
    b = _lib.MocBatch(X=4096, dtype=_lib.MOC_F32, D=512, total_rows=64, n_slides=4, max_rows=16,
                      row_off=ctypes.cast(off, ctypes.c_void_p), C=2, Ce=6, topj=10, topk=5)
    assert h.moc_stats_share(ctypes.byref(b), lp, 0, 4, None) == 1 and b"no stats" in h.moc_last_error()
    b.stats, b.sel_flag = 4096, 4096
    for s0, n in ((-1, 2), (0, 0), (0, 5), (3, 2), (4, 1)):
        assert h.moc_stats_share(ctypes.byref(b), lp, s0, n, None) == 1 and b"bad slide range" in h.moc_last_error(), (s0, n)
    with pytest.raises(AssertionError, match="bad slide range"):
        _lib.check(1, "moc_stats_share")


def test_chains_never_mix_configurations():
    from moc_amd.runs import group_runs
    cfgs = [(50, 5, 0), (100, 10, 0), (100, 10, 4), (20, 3, 9)]
    # five folds per configuration, fold-major inside one: what the driver hands over
    keys = [(8, 0, c) for c in cfgs for _ in range(5)]
    chains = group_runs(keys, 8)
    assert sorted(r for ch in chains for r in ch) == list(range(20))
    for ch in chains:
        assert len({keys[r][2] for r in ch}) == 1               # one configuration
        assert ch == list(range(ch[0], ch[0] + len(ch)))        # consecutive runs
        assert len(ch) <= 8
    assert [len(ch) for ch in chains] == [5, 5, 5, 5]
    # the cap still cuts a configuration of many folds into even chains; unequal pass lengths still part the runs
    keys = [(8, 0, cfgs[0])] * 9 + [(8, 0, cfgs[1])] * 3 + [(4, 0, cfgs[1])] * 2
    chains = group_runs(keys, 8)
    assert [len(ch) for ch in chains] == [5, 4, 3, 2] and all(len({keys[r] for r in ch}) == 1 for ch in chains)
    assert max(len(ch) for ch in group_runs([(8, 0, cfgs[0])] * 32, 16)) == 16
    # interleaved configurations: still one chain per configuration, the runs in their given order
    assert group_runs([(8, 0, cfgs[i % 2]) for i in range(6)], 8) == [[0, 2, 4], [1, 3, 5]]


def test_mask_groups():
    from moc_amd.runs import consecutive_blocks, mask_groups
    A, B = 1001, 1002                                           # split ids
    s0, s1, s2 = b"state-0", b"state-1", b"state-2"
    # four configurations x two folds, every fold's generators in step
    keys = [(A, s0), (B, s1)] * 4
    assert mask_groups(keys) == [0, 1, 0, 1, 0, 1, 0, 1]
    # run 3 has diverged: it leaves its group, the others stay with their leader
    keys[3] = (B, s2)
    assert mask_groups(keys) == [0, 1, 0, 3, 0, 1, 0, 1]
    # equal states on DIFFERENT splits share nothing; equal splits with different states neither
    assert mask_groups([(A, s0), (B, s0), (A, s1)]) == [0, 1, 2]
    # singletons, a run that takes no part, a leader that is not the first run
    assert mask_groups([(A, s0)]) == [0]
    assert mask_groups([None, (A, s0), None, (A, s0)]) == [0, 1, 2, 1]
    assert mask_groups([]) == []
    # two diverged runs that agree with each other form a group of their own
    assert mask_groups([(A, s0), (A, s1), (A, s0), (A, s1)]) == [0, 1, 0, 1]
    assert consecutive_blocks([0, 1, 3, 4, 5, 9]) == [(0, 2), (3, 3), (9, 1)] and consecutive_blocks([]) == []


def _args(*argv):
    from moc_amd import run_moc
    return run_moc.get_args(list(argv))


def test_flags_configurations_and_result_directories():
    from moc_amd import run_moc
    a = _args("--topjs", "50,100", "--topks", "5,10", "--discard_sets", "none", "topk+bottomk", "--folds", "0,1",
              "--result_dir", "out")
    assert run_moc.hgrid_requested(a)
    cfgs = run_moc.hgrid_configs(a)
    assert cfgs == [(50, 5, ()), (50, 5, ("topk", "bottomk")), (50, 10, ()), (50, 10, ("topk", "bottomk")),
                    (100, 5, ()), (100, 5, ("topk", "bottomk")), (100, 10, ()), (100, 10, ("topk", "bottomk"))]
    assert run_moc.hgrid_dir("out", cfgs[0]) == os.path.join("out", "topj50_topk5_none")
    assert run_moc.hgrid_dir("out", cfgs[7]) == os.path.join("out", "topj100_topk10_topk+bottomk")
    runs = run_moc.hgrid_runs(a, cfgs, [0, 1])
    assert [(r.topj, r.topk, tuple(r.discard_classifiers), r.fold) for r in runs[:4]] == \
        [(50, 5, (), 0), (50, 5, (), 1), (50, 5, ("topk", "bottomk"), 0), (50, 5, ("topk", "bottomk"), 1)]
    assert runs[2].result_dir == os.path.join("out", "topj50_topk5_topk+bottomk") and a.result_dir == "out"
    # a list that is not given is the single flag's value
    b = _args("--topks", "3,5", "--topj", "77", "--discard_classifiers", "delta_diff")
    assert run_moc.hgrid_configs(b) == [(77, 3, ("delta_diff",)), (77, 5, ("delta_diff",))]
    assert not run_moc.hgrid_requested(_args("--folds", "0,1"))
    run_moc.check_hgrid_args(a)                                 # nothing to refuse
    run_moc.check_hgrid_args(_args("--shots", "1,2", "--patch_maps", "test"))       # not a grid: not this function's business


@pytest.mark.parametrize("argv,message", [
    (["--topjs", "50,100", "--shots", "1,2"], "do not combine with --shots"),
    (["--topks", "5,10", "--patch_maps", "test"], "do not combine with --patch_maps"),
    (["--topks", "5,10", "--patch_maps_from", "best.pt"], "do not combine with --patch_maps"),
    (["--discard_sets", "none", "topk", "--loader_seed_draw", "1"], "do not combine with --loader_seed_draw"),
    (["--topjs", ""], "--topjs: a non-empty list"),
    (["--topks", ","], "--topks: a non-empty list"),
    (["--topks", "5,x"], "--topks: not a comma-separated list"),
    (["--discard_sets"], "--discard_sets: an empty list"),
    (["--discard_sets", "topk+nonsense"], "--discard_sets: discard set 'topk\\+nonsense'"),
    (["--topjs", "50,50"], "--topjs: a value named twice"),
    (["--topjs", "50,100", "--ablation_study", "avg"], "the ablation study trains none"),
])
def test_refusals_come_before_any_bag_is_loaded(argv, message, monkeypatch):
    from moc_amd import run_moc
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit, match=message):
        run_moc.check_hgrid_args(_args(*argv))
    # cli() refuses the same way, before it looks for a GPU
    with pytest.raises(SystemExit, match=message):
        run_moc.cli(argv)


def test_a_launcher_needs_a_seed(monkeypatch):
    from moc_amd import run_moc
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="under a launcher need --seed"):
        run_moc.check_hgrid_args(_args("--topjs", "50,100"))
    run_moc.check_hgrid_args(_args("--topjs", "50,100", "--seed", "1"))


def test_more_than_32_runs_train_in_blocks_of_whole_configurations():
    from moc_amd import run_moc
    from moc_amd.runs import MAX_RUNS
    assert MAX_RUNS == 32
    # fifteen discard sets x five folds = 75 runs: six configurations (30 runs) per block
    blocks = run_moc.hgrid_blocks(15, 5, MAX_RUNS)
    assert blocks == [[0, 1, 2, 3, 4, 5], [6, 7, 8, 9, 10, 11], [12, 13, 14]]
    assert run_moc.hgrid_blocks(20, 5, MAX_RUNS)[-1] == [18, 19] and len(run_moc.hgrid_blocks(20, 5, MAX_RUNS)) == 4
    assert run_moc.hgrid_blocks(8, 2, MAX_RUNS) == [list(range(8))]
    assert run_moc.hgrid_blocks(3, 32, MAX_RUNS) == [[0], [1], [2]]
    assert run_moc.hgrid_blocks(4, 20, MAX_RUNS) == [[0], [1], [2], [3]]            # never part of a configuration
    with pytest.raises(SystemExit, match="at most 32"):
        run_moc.hgrid_blocks(2, 33, MAX_RUNS)


def test_grid_footprint_counts_the_splits_of_a_fold_once():
    from moc_amd import run_moc
    fold0 = [(("t", 0), 10_000), (("v", 0), 50_000), (("e", 0), 60_000)]
    fold1 = [(("t", 1), 12_000), (("v", 1), 50_000), (("e", 1), 60_000)]
    one = run_moc.grid_bytes([fold0], 512, 4, 2)
    four = run_moc.grid_bytes([fold0] * 4, 512, 4, 2)
    # three more configurations of the same fold add their work arrays and nothing else: no bag, no second copy of the
    # train split, no packing copy (C = 2: 73 bytes per evaluated row, 353 per trained row and set)
    per_run = (10_000 + 50_000 + 2 * 60_000) * 73 + 10_000 * 2 * 353
    assert four - one == 3 * per_run
    both = run_moc.grid_bytes([fold0, fold1] * 2, 512, 4, 2)
    assert both > four


def test_summary_reads_a_directory_that_holds_the_result_files_itself(tmp_path):
    import json
    from moc_amd import run_moc
    for fold in range(5):
        json.dump({"test_at_best_val": 0.5 + fold / 10, "test_acc_at_best_val": 0.5, "zero_shot_test": {"auc": 0.6, "acc": 0.5}},
                  open(tmp_path / f"best_results_shot_4_fold_{fold}.json", "w"))
    run_moc.cli(["--summary", "--summary_dir", str(tmp_path)])
    table = open(tmp_path / "summary_4.csv").read().splitlines()
    assert table[0].startswith("fold,test_auc") and len(table) == 7 and not os.path.exists(tmp_path / "summary_1.csv")
