"""The shots x folds grid in one process, host side (no GPU): the C entry is declared and bound, the driver parses `--shots`,
maps (shot, fold) to the launcher's result directories and deals the pairs to the ranks, and runs of unequal pass length
are grouped into lockstep chains (moc_amd.runs.group_runs)."""
import os
import re

import pytest

from moc_amd import _lib, run_moc, runs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_declared_and_bound_and_the_abi_stays_20():
    header = open(os.path.join(ROOT, "include", "moc_hip.h")).read()
    assert re.search(r"#define\s+MOC_ABI_VERSION\s+20\b", header)
    assert re.search(r"int\s+moc_meta_forward_by_slide\s*\(", header)
    assert "moc_meta_forward_by_slide" in _lib.SIGNATURES and _lib.ABI_VERSION == 20
    res, argtypes = _lib.SIGNATURES["moc_meta_forward_by_slide"]
    assert len(argtypes) == 9                       # B, M, R, model_of_slide, ws, slide0, n, use_bits, stream
    assert [n for n, _ in _lib.MocRuns._fields_] == ["n_runs", "slide_stride", "par_stride", "image_stride"]
    declared = set(re.findall(r"\b(moc_[a-z0-9_]+)\s*\(", header))
    assert set(_lib.SIGNATURES) <= declared


def test_shots_flag_and_result_directories():
    a = run_moc.get_args(["--shots", "1,4", "--folds", "0,1", "--result_dir", "out"])
    assert a.shots == "1,4"
    pairs = run_moc.pairs_of_rank(a.shots, a.folds, a.shot, a.fold, 0, 1)
    assert pairs == [(1, 0), (1, 1), (4, 0), (4, 1)]            # shot-major: runs of one pass length side by side
    assert [run_moc.run_result_dir(a, s) for s, _ in pairs] == [os.path.join("out", "1_shot")] * 2 + [os.path.join("out", "4_shot")] * 2
    # --shots without --folds: the one --fold; --folds alone keeps writing into --result_dir itself
    b = run_moc.get_args(["--shots", "2,8", "--fold", "3", "--result_dir", "out"])
    assert run_moc.pairs_of_rank(b.shots, b.folds, b.shot, b.fold, 0, 1) == [(2, 3), (8, 3)]
    c = run_moc.get_args(["--folds", "0,1", "--shot", "16", "--result_dir", "out"])
    assert run_moc.pairs_of_rank(c.shots, c.folds, c.shot, c.fold, 0, 1) == [(16, 0), (16, 1)]
    assert run_moc.run_result_dir(c, 16) == "out"
    with pytest.raises(AssertionError, match="twice"):
        run_moc.pairs_of_rank("1,1", "0", 1, 0, 0, 1)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_every_pair_is_trained_exactly_once_over_the_ranks(world):
    shots, folds = "1,2,4,8,16", "0,1,2,3,4"
    dealt = [run_moc.pairs_of_rank(shots, folds, 1, 0, rank, world) for rank in range(world)]
    flat = [p for d in dealt for p in d]
    assert sorted(flat) == sorted((s, f) for s in (1, 2, 4, 8, 16) for f in range(5)) and len(set(flat)) == 25
    assert max(len(d) for d in dealt) - min(len(d) for d in dealt) <= 1


def test_shots_do_not_combine_with_patch_maps():
    a = run_moc.get_args(["--shots", "1,2", "--patch_maps", "test"])
    with pytest.raises(SystemExit, match="--shots"):
        run_moc.check_patch_map_args(a)
    run_moc.check_patch_map_args(run_moc.get_args(["--shots", "1,2"]))       # (alone it is fine)


def test_runs_are_grouped_by_pass_length():
    lengths = [n for n in (2, 4, 8, 16, 32) for _ in range(5)]
    chains = runs.group_runs(lengths, cap=8)
    assert sorted(r for c in chains for r in c) == list(range(25))           # every run in exactly one chain
    assert all(len({lengths[r] for r in c}) == 1 for c in chains)            # a chain's runs make the same visits
    assert len(chains) == 5 and all(len(c) == 5 for c in chains)
    # interleaved order, long groups, keys that carry a step count too
    inter = [2, 32, 2, 32, 4]
    assert runs.group_runs(inter, cap=8) == [[0, 2], [1, 3], [4]]
    many = runs.group_runs([7] * 40, cap=16)
    assert all(len(c) <= 16 for c in many) and sorted(r for c in many for r in c) == list(range(40))
    assert [len(c) for c in runs.group_runs([3] * 9, cap=8)] == [5, 4]
    assert runs.group_runs([(4, 0), (4, 8), (4, 0)], cap=8) == [[0, 2], [1]]
    assert runs.group_runs([5, 5, 5], cap=1) == [[0], [1], [2]]
    with pytest.raises(AssertionError):
        runs.group_runs([1, 2], cap=17)
    assert runs.MAX_RUNS >= 25


def test_grid_footprint_counts_a_shared_split_once():
    a = run_moc.get_args(["--synthetic", "6", "--shots", "1,4", "--folds", "0,1"])
    fps = []
    for shot, fold in run_moc.pairs_of_rank(a.shots, a.folds, a.shot, a.fold, 0, 1):
        a.shot, a.fold = shot, fold
        fps.append(run_moc.split_footprints(a))
    # the generated validation / test slides of a fold do not depend on the shot count: the same key, held once
    assert fps[0][1][0] == fps[2][1][0] and fps[0][2][0] == fps[2][2][0] and fps[0][1][0] != fps[1][1][0]
    assert fps[0][0][0] != fps[2][0][0]
    whole = run_moc.grid_bytes(fps, 512, 4, 2)
    assert whole < sum(run_moc.grid_bytes([fp], 512, 4, 2) for fp in fps)
    assert run_moc.largest_grid(fps, 512, 4, 2, whole) == 4
    assert run_moc.largest_grid(fps, 512, 4, 2, whole - 1) == 3
    assert run_moc.largest_grid(fps, 512, 4, 2, 0) == 0
    # a shared split's work arrays count per visit: two runs that share everything but the train split need more than one
    one = run_moc.grid_bytes([fps[0]], 512, 4, 2)
    two = run_moc.grid_bytes([fps[0], fps[2]], 512, 4, 2)
    ws_eval = 4 * 7 + 4 * 6 + 13 + 4 * 2
    assert two - one >= (fps[2][1][1] + 2 * fps[2][2][1]) * ws_eval + fps[2][0][1] * 512 * 4
    assert run_moc.FEATURE_DIM == 512
