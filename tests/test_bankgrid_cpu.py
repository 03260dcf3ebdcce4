"""Bank grids without a GPU: the plan of the multi-bank score launches, moc_kept_share's argument checks and
a host model of its kernel's index arithmetic, and the driver's flags, refusals, directories, blocks and summary."""
import ctypes
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_declared_and_bound_and_the_abi_stays_20():
    from moc_amd import _lib
    src = open(os.path.join(ROOT, "include", "moc_hip.h")).read()
    assert re.search(r"int\s+moc_kept_share\s*\(", src) and "#define MOC_ABI_VERSION 20" in src
    assert "moc_kept_share" in _lib.SIGNATURES and _lib.ABI_VERSION == 20
    assert "moc_kept_share" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    h = _lib.lib()
    assert hasattr(h, "moc_kept_share") and h.moc_version() == 20
    assert "kept_share_kernel" in open(os.path.join(ROOT, "moc_amd", "csrc", "moc_share.hip")).read()


# ------------------------------------------------------------------ the plan
def _layout(run_sizes):
    """run_sizes[r]: the slide sizes of run r -> (run_slide0, run_n, row_off_host)."""
    slide0, n, off = [], [], [0]
    for sizes in run_sizes:
        slide0.append(len(off) - 1)
        n.append(len(sizes))
        for s in sizes:
            off.append(off[-1] + s)
    return slide0, n, off


FOLD_A, FOLD_B = [1, 600, 17, 255], [16, 15, 256, 2, 16]


@pytest.mark.parametrize("dtype,cuts", [(torch.float32, [(0, 4), (4, 1)]), (torch.bfloat16, [(0, 3), (3, 2)]),
                                        (torch.float16, [(0, 3), (3, 2)])])
def test_five_banks_at_512_are_two_passes(dtype, cuts):
    from moc_amd import engine
    from moc_amd.runs import bank_score_plan
    passes = engine.plan_bank_passes(512, dtype, 5)
    assert passes == cuts
    # bank-major, two folds: both leaders are consecutive runs and their followers lie the same distance behind them
    slide0, n, off = _layout([FOLD_A, FOLD_B] * 5)
    rows = sum(FOLD_A) + sum(FOLD_B)
    plan = bank_score_plan([0, 1] * 5, [g for g in range(5) for _ in range(2)], slide0, n, off, passes)
    assert plan == [(0, 9, g0, [(g, g * rows) for g in range(g0, g0 + k)]) for g0, k in cuts]
    assert plan == bank_score_plan([0, 1] * 5, [g for g in range(5) for _ in range(2)], slide0, n, off, passes)     # deterministic


def test_two_folds_that_are_not_neighbours_are_two_leader_blocks():
    from moc_amd.runs import bank_score_plan
    # fold-major: runs (fold 0: banks 0, 1, 2), (fold 1: banks 0, 1, 2)
    slide0, n, off = _layout([FOLD_A] * 3 + [FOLD_B] * 3)
    a, b = sum(FOLD_A), sum(FOLD_B)
    plan = bank_score_plan([0, 0, 0, 3, 3, 3], [0, 1, 2, 0, 1, 2], slide0, n, off, [(0, 3)])
    assert plan == [(0, 4, 0, [(0, 0), (1, a), (2, 2 * a)]), (12, 5, 0, [(0, 0), (1, b), (2, 2 * b)])]
    # neighbours whose followers lie at different distances do not share a launch either
    slide0, n, off = _layout([FOLD_A, FOLD_B, FOLD_B, FOLD_A])
    plan = bank_score_plan([0, 1, 1, 0], [0, 0, 1, 1], slide0, n, off, [(0, 2)])
    assert plan == [(0, 4, 0, [(0, 0), (1, a + 2 * b)]), (4, 5, 0, [(0, 0), (1, b)])]


def test_a_bank_absent_from_a_group_and_a_run_that_left_its_group():
    from moc_amd.runs import bank_heads, bank_score_plan
    a = sum(FOLD_A)
    slide0, n, off = _layout([FOLD_A] * 3)
    # run 1 (bank 1) has left the group: it is its own leader, its launch carries its bank alone; the group of run 0 has no
    # run under bank 1 any more -- its window of the launch goes to scratch (None)
    plan = bank_score_plan([0, 1, 0], [0, 1, 2], slide0, n, off, [(0, 3)])
    assert plan == [(0, 4, 0, [(0, 0), (1, None), (2, 2 * a)]), (4, 4, 1, [(1, 0)])]
    # five banks in passes 3 + 2 with the diverged run under bank 4: its group launches the second pass only, trimmed to it
    slide0, n, off = _layout([FOLD_A] * 5)
    plan = bank_score_plan([0, 0, 0, 0, 4], [0, 1, 2, 3, 4], slide0, n, off, [(0, 3), (3, 2)])
    assert plan == [(0, 4, 0, [(0, 0), (1, a), (2, 2 * a)]), (0, 4, 3, [(3, 3 * a)]), (16, 4, 4, [(4, 0)])]
    # two runs of one (group, bank) -- configurations of a hyper-parameter grid: the first is scored, the second is not in the plan
    slide0, n, off = _layout([FOLD_A] * 4)
    assert bank_heads([0, 0, 0, 0], [0, 1, 0, 1]) == {(0, 0): 0, (0, 1): 1}
    assert bank_score_plan([0, 0, 0, 0], [0, 1, 0, 1], slide0, n, off, [(0, 2)]) == [(0, 4, 0, [(0, 0), (1, a)])]
    # the leader trains under a later bank than its follower: the distance is that of the FOLLOWER's slots all the same
    assert bank_score_plan([0, 0], [1, 0], *_layout([FOLD_A] * 2), [(0, 2)]) == [(0, 4, 0, [(0, a), (1, 0)])]


def test_the_plan_asserts_the_constant_distance():
    from moc_amd.runs import bank_score_plan
    slide0, n, off = _layout([[16, 32, 48], [16, 48, 32]])          # the same rows, another order
    with pytest.raises(AssertionError, match="same sizes in the same order"):
        bank_score_plan([0, 0], [0, 1], slide0, n, off, [(0, 2)])
    slide0, n, off = _layout([[16, 32, 48], [16, 32]])
    with pytest.raises(AssertionError, match="number of visits"):
        bank_score_plan([0, 0], [0, 1], slide0, n, off, [(0, 2)])


def test_train_runs_refuses_wide_and_mixed_banks_before_it_allocates():
    """On the host: the refusals come before the first device array (a split packed on the CPU gets that far and no further)."""
    import types
    from moc_amd import main_moc as M, runs
    args = types.SimpleNamespace(n_classes=2, topj=10, topk=5, discard_classifiers=[])
    W2, W3, E6, E17 = torch.zeros((512, 2)), torch.zeros((512, 3)), torch.zeros((512, 6)), torch.zeros((512, 17))

    def build(banks, of_run, cache=False):
        sp = M.ResidentBags([torch.zeros((4, 512))], [0], "cpu", cache_scores=cache)
        return runs.TrainRuns([None], [None], [sp], "cpu", args, generators=[torch.Generator()], banks=banks, bank_of_run=of_run)
    with pytest.raises(AssertionError, match="wider than 16 columns"):
        build([(W2, E6), (W2, E17)], [0])
    with pytest.raises(AssertionError, match="different C"):
        build([(W2, E6), (W3, E6)], [0])
    with pytest.raises(AssertionError, match="bank_of_run names one of the banks"):
        build([(W2, E6)], [1])
    with pytest.raises(AssertionError, match="score cache belongs to one bank"):
        build([(W2, E6)], [0], cache=True)
    with pytest.raises(AssertionError, match="bank_of_run without banks"):
        build(None, [0])


# ------------------------------------------------------------------ moc_kept_share: the host checks
def test_kept_share_refuses_bad_arguments_before_any_launch():
    from moc_amd import _lib
    h = _lib.lib()
    b = _lib.MocBatch()
    lead = (ctypes.c_int32 * 4)(-1, 0, -1, -1)
    lp = ctypes.cast(lead, ctypes.c_void_p)
    assert h.moc_kept_share(None, lp, 0, 1, None) == 1 and b"moc_kept_share: null pointer" in h.moc_last_error()
    assert h.moc_kept_share(ctypes.byref(b), None, 0, 1, None) == 1 and b"moc_kept_share: null pointer" in h.moc_last_error()
    assert h.moc_kept_share(ctypes.byref(b), lp, 0, 1, None) == 1 and b"moc_kept_share: null X/row_off" in h.moc_last_error()
    off = (ctypes.c_int64 * 5)(0, 16, 32, 48, 64)
    # an UNMASKED batch that passes the common checks (no pointer is followed on the host): a bad range is refused, a good
    # one is MOC_OK without a launch -- stats / sel_flag may be null, the entry never reads them
    b = _lib.MocBatch(X=4096, dtype=_lib.MOC_F32, D=512, total_rows=64, n_slides=4, max_rows=16,
                      row_off=ctypes.cast(off, ctypes.c_void_p), C=2, Ce=6, topj=10, topk=5)
    for s0, n in ((-1, 2), (0, 0), (0, 5), (3, 2), (4, 1)):
        assert h.moc_kept_share(ctypes.byref(b), lp, s0, n, None) == 1 and b"moc_kept_share: bad slide range" in h.moc_last_error(), (s0, n)
    assert h.moc_kept_share(ctypes.byref(b), lp, 0, 4, None) == 0
    # a masked batch without its lists
    b.mask = 4096
    assert h.moc_kept_share(ctypes.byref(b), lp, 0, 4, None) == 1
    assert b"moc_kept_share" in h.moc_last_error() and b"kept" in h.moc_last_error() and b"n_kept" in h.moc_last_error()
    b.kept = 4096
    assert h.moc_kept_share(ctypes.byref(b), lp, 0, 4, None) == 1 and b"moc_kept_share" in h.moc_last_error()
    b.n_kept = 4096
    for s0, n in ((-1, 2), (0, 0), (0, 5), (3, 2), (4, 1)):        # the range is refused on a masked batch too, before the launch
        assert h.moc_kept_share(ctypes.byref(b), lp, s0, n, None) == 1 and b"bad slide range" in h.moc_last_error(), (s0, n)


# ------------------------------------------------------------------ kept_share_kernel: a host model of its lanes
SH_THREADS, SH_CHUNK = 256, 1024


def _kept_share_lanes(src0, dst0, cap_l, cap_b, n_kept_l, grid_x, vec_ok=1):
    """The stores of one follower slide, lane by lane, as moc_share.hip's kept_share_kernel forms them ->
    [(destination word, source word, words of the store)] in absolute slots of `kept`."""
    nk = max(0, min(n_kept_l, cap_l, cap_b))
    out = []
    if nk == 0:
        return nk, out
    vec = bool(vec_ok) and ((src0 - dst0) & 3) == 0
    for bx in range(grid_x):
        for t in range(SH_THREADS):
            if vec:
                head = (4 - (dst0 & 3)) & 3
                h = min(head, nk)
                nvec = (nk - h) >> 2
                tail0 = h + 4 * nvec
                v = bx * SH_THREADS + t
                while v < nvec:
                    out.append((dst0 + h + 4 * v, src0 + h + 4 * v, 4))
                    v += grid_x * SH_THREADS
                if bx == 0 and t < 8:
                    i = t if t < 4 else tail0 + (t - 4)
                    ok = t < h if t < 4 else (t - 4) < nk - tail0
                    if ok:
                        out.append((dst0 + i, src0 + i, 1))
            else:
                i0 = bx * SH_CHUNK
                while i0 < nk:
                    for u in range(4):
                        i = i0 + u * SH_THREADS + t
                        if i < nk:
                            out.append((dst0 + i, src0 + i, 1))
                    i0 += grid_x * SH_CHUNK
    return nk, out


@pytest.mark.parametrize("size", [1, 3, 4, 5, 255, 256, 257, 1023, 1025, 2600])
@pytest.mark.parametrize("dist", [0, 1, 2, 3])
def test_every_word_of_a_followers_list_is_written_once_and_nothing_else(size, dist):
    for dst_phase in range(4):
        for follower_first in (False, True):
            # slots between the two slides: a multiple of four plus `dist`
            gap = size + 4 * 7 + dist + (-size % 4)
            lo, hi = 100 + dst_phase, 100 + dst_phase + gap
            dst0, src0 = (lo, hi) if follower_first else (hi, lo)
            assert abs(src0 - dst0) % 4 == dist
            for nk_l in sorted({size, max(0, size - 1), size // 2, 0, size + 5}):      # (more than the slide: clamped)
                for grid_x in sorted({1, (size + SH_CHUNK - 1) // SH_CHUNK}):
                    for vec_ok in (1, 0):
                        nk, stores = _kept_share_lanes(src0, dst0, size, size, nk_l, grid_x, vec_ok)
                        assert nk == min(nk_l, size)
                        written = []
                        for d, s, w in stores:
                            assert s - src0 == d - dst0
                            if w == 4:                             # 16-byte accesses on both sides
                                assert d % 4 == 0 and s % 4 == 0 and dist == 0 and vec_ok
                            written += range(d, d + w)
                        assert sorted(written) == list(range(dst0, dst0 + nk)), (size, dist, dst_phase, nk_l, grid_x, vec_ok)
                        if dist == 0 and vec_ok and nk >= 8:
                            assert any(w == 4 for _, _, w in stores)


def test_a_follower_of_another_size_is_clamped_to_both():
    nk, stores = _kept_share_lanes(0, 400, 300, 17, 290, 1)
    assert nk == 17 and sorted(x for d, _, w in stores for x in range(d, d + w)) == list(range(400, 417))
    nk, stores = _kept_share_lanes(0, 400, 9, 300, 290, 1)
    assert nk == 9 and max(s + w for _, s, w in stores) <= 9


# ------------------------------------------------------------------ the driver
def _args(*argv):
    from moc_amd import run_moc
    return run_moc.get_args(list(argv))


def _save_bank(tmp_path, name, C_=2, ce=6, D=512):
    from moc_amd import synth
    W, We = synth.make_bank(50 + ce, D, C_, n_bg=ce - C_)
    fw, fe = str(tmp_path / f"{name}_w.pt"), str(tmp_path / f"{name}_we.pt")
    torch.save(W, fw)
    torch.save(We, fe)
    return f"{name}={fw},{fe}"


def test_flags_directories_runs_and_blocks(tmp_path):
    from moc_amd import run_moc
    from moc_amd.runs import MAX_RUNS
    a = _args("--banks", _save_bank(tmp_path, "plain"), _save_bank(tmp_path, "long", ce=16), "--folds", "0,1,2", "--seed", "3",
              "--result_dir", "out")
    assert run_moc.bankgrid_requested(a) and not run_moc.bankgrid_requested(_args("--folds", "0,1"))
    banks = run_moc.check_bankgrid_args(a)
    assert [(n, tuple(W.shape), tuple(We.shape)) for n, W, We in banks] == [("plain", (512, 2), (512, 6)), ("long", (512, 2), (512, 16))]
    assert run_moc.check_bankgrid_args(_args("--folds", "0,1")) is None
    assert run_moc.bankgrid_dir("out", "plain") == os.path.join("out", "bank_plain")
    runs = run_moc.bankgrid_runs(a, ["plain", "long"], [0, 1, 2])
    assert [(r.bank, r.fold) for r in runs] == [("plain", 0), ("plain", 1), ("plain", 2), ("long", 0), ("long", 1), ("long", 2)]
    assert runs[4].result_dir == os.path.join("out", "bank_long") and a.result_dir == "out"
    # more than 32 runs: blocks of whole folds, a fold's banks together
    assert run_moc.bankgrid_blocks(4, 5, MAX_RUNS) == [[0, 1, 2, 3, 4]]
    assert run_moc.bankgrid_blocks(7, 5, MAX_RUNS) == [[0, 1, 2, 3], [4]]
    assert run_moc.bankgrid_blocks(20, 3, MAX_RUNS) == [[0], [1], [2]]
    with pytest.raises(SystemExit, match="at most 32"):
        run_moc.bankgrid_blocks(33, 1, MAX_RUNS)


def test_grid_footprint_counts_a_folds_splits_once_and_the_work_arrays_per_bank():
    from moc_amd import engine, run_moc
    fold0 = [(("t", 0), 10_000), (("v", 0), 50_000), (("e", 0), 60_000)]
    fold1 = [(("t", 1), 12_000), (("v", 1), 50_000), (("e", 1), 60_000)]
    one = run_moc.bankgrid_bytes([fold0, fold1], 512, 4, 2, 1)
    four = run_moc.bankgrid_bytes([fold0, fold1], 512, 4, 2, 4)
    ws = engine.bank_work_row_bytes(2)
    per_bank = sum((tr + va + 2 * te) * ws + tr * 2 * (ws + 4 * 64 + 16 + 8) for (_, tr), (_, va), (_, te) in (fold0, fold1))
    assert four - one == 3 * per_bank                       # three more banks: their work arrays and not one bag
    assert one == run_moc.grid_bytes([fold0, fold1], 512, 4, 2)


@pytest.mark.parametrize("extra,message", [
    (["--shots", "1,2"], "does not combine with --shots"),
    (["--topjs", "50,100"], "does not combine with --topjs"),
    (["--topks", "5,10"], "does not combine with --topjs"),
    (["--discard_sets", "none", "topk"], "does not combine with --topjs"),
    (["--seeds", "1,2"], "does not combine with --seeds / --lrs / --wds"),
    (["--lrs", "1e-3,1e-4"], "does not combine with --seeds / --lrs / --wds"),
    (["--wds", "0,1e-4"], "does not combine with --seeds / --lrs / --wds"),
    (["--patch_maps", "test"], "does not combine with --patch_maps"),
    (["--patch_maps_from", "best.pt"], "does not combine with --patch_maps"),
    (["--loader_seed_draw", "1"], "does not combine with --loader_seed_draw"),
    (["--cache_scores", "1"], "does not combine with --cache_scores"),
    (["--ablation_study", "avg"], "the ablation study trains none"),
])
def test_flags_that_do_not_combine_are_refused_before_any_bag_is_loaded(tmp_path, monkeypatch, extra, message):
    from moc_amd import run_moc
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    argv = ["--banks", _save_bank(tmp_path, "a"), _save_bank(tmp_path, "b", ce=5), "--seed", "1"] + extra
    with pytest.raises(SystemExit, match=message):
        run_moc.check_bankgrid_args(_args(*argv))
    with pytest.raises(SystemExit, match=message):                 # cli() refuses the same way, before it looks for a GPU
        run_moc.cli(argv)


def test_bank_files_are_checked_before_any_bag_is_loaded(tmp_path, monkeypatch):
    from moc_amd import run_moc
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    a, b = _save_bank(tmp_path, "a"), _save_bank(tmp_path, "b", ce=5)

    def refused(argv, message):
        with pytest.raises(SystemExit, match=message):
            run_moc.check_bankgrid_args(_args(*argv))
        with pytest.raises(SystemExit, match=message):
            run_moc.cli(argv)
    refused(["--banks", a, b], "--banks needs --seed")
    refused(["--banks", a, a, "--seed", "1"], "duplicate bank name 'a'")
    refused(["--banks", a, "c=" + str(tmp_path / "no_w.pt") + "," + str(tmp_path / "no_we.pt"), "--seed", "1"], "no_w.pt: no such file")
    refused(["--banks", a, _save_bank(tmp_path, "three", C_=3, ce=7), "--seed", "1"], r"banks of different C \(\[2, 3\]\)")
    refused(["--banks", a, _save_bank(tmp_path, "wide", ce=17), "--seed", "1"], "wide: Ce=17 columns; a bank grid takes banks of at most 16")
    torch.save({"not": "a tensor"}, str(tmp_path / "bad_w.pt"))
    refused(["--banks", f"bad={tmp_path / 'bad_w.pt'},{tmp_path / 'a_we.pt'}", "--seed", "1"], "bad: need saved tensors")
    monkeypatch.setenv("WORLD_SIZE", "2")
    refused(["--banks", a, b, "--seed", "1"], "one-GPU option")
    # a malformed NAME=W,W_ext is argparse's refusal
    with pytest.raises(SystemExit):
        _args("--banks", "nofiles", "--seed", "1")


def test_without_banks_the_command_is_as_it_was():
    from moc_amd import run_moc
    a = _args("--folds", "0,1", "--seed", "1")
    assert a.banks is None and run_moc.check_bankgrid_args(a) is None


def test_summary_arithmetic_and_the_summary_of_a_banks_directory(tmp_path):
    import numpy as np
    import pandas as pd
    from moc_amd import run_moc
    vals = {"plain": [(0.5, 0.6), (0.7, 0.4), (0.9, 0.8), (0.6, 0.6), (0.8, 0.7)],
            "long": [(1.0, 0.5), (0.5, 1.0), (0.75, 0.75), (0.25, 0.5), (0.5, 0.25)]}
    for name, vs in vals.items():
        d = run_moc.bankgrid_dir(str(tmp_path), name)
        os.makedirs(d)
        for fold, (bv, ta) in enumerate(vs):
            json.dump({"best_val": bv, "test_at_best_val": ta, "test_acc_at_best_val": 0.5, "zero_shot_test": {"auc": 0.6, "acc": 0.5}},
                      open(os.path.join(d, f"best_results_shot_4_fold_{fold}.json"), "w"))
    path = run_moc.write_bankgrid_summary(str(tmp_path), ["plain", "long"], [0, 1, 2, 3, 4], 4)
    assert path == os.path.join(str(tmp_path), "bank_grid_summary.csv")
    t = pd.read_csv(path, float_precision="round_trip")
    assert list(t.columns) == ["bank", "runs", "best_val_mean", "best_val_std", "test_auc_mean", "test_auc_std"]
    assert list(t["bank"]) == ["plain", "long"] and list(t["runs"]) == [5, 5]
    for i, name in enumerate(["plain", "long"]):
        v = np.asarray(vals[name], dtype=np.float64)
        assert t["best_val_mean"][i] == v[:, 0].mean() and t["best_val_std"][i] == v[:, 0].std()         # population: ddof = 0
        assert t["test_auc_mean"][i] == v[:, 1].mean() and t["test_auc_std"][i] == v[:, 1].std()
    assert t["best_val_std"][0] == pytest.approx(np.sqrt(0.02))
    # a subset of the folds is what was asked for, not what lies in the directory
    t2 = pd.read_csv(run_moc.write_bankgrid_summary(str(tmp_path), ["long"], [0, 1], 4), float_precision="round_trip")
    assert list(t2["runs"]) == [2] and t2["best_val_mean"][0] == 0.75 and t2["best_val_std"][0] == 0.25
    # --summary reads a bank's directory as it reads any directory that holds the result files itself
    d = run_moc.bankgrid_dir(str(tmp_path), "plain")
    run_moc.cli(["--summary", "--summary_dir", d])
    table = open(os.path.join(d, "summary_4.csv")).read().splitlines()
    assert table[0].startswith("fold,test_auc") and len(table) == 7 and table[1].startswith("0,0.6")
