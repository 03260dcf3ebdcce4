"""Bank sweeps, the parts that need no GPU: moc_scores_banks refuses bad arguments before anything is launched (the
library's checks are host code), the planner's cuts for (D, storage, number of banks), the chunk sizes, the command
line's argument checks and the summary writer."""
import ctypes

import pandas as pd
import pytest
import torch


# ------------------------------------------------------------------ the entry's refusals
def _valid(D=512, dtype=0, n_banks=2, C=2, Ce=(3, 16, 6, 6)):
    """A batch and a bank set that pass every check (host buffers stand in for device memory: nothing here is launched,
    every case below breaks exactly one rule)."""
    from moc_amd import _lib
    keep = [ctypes.create_string_buffer(4096 + 16) for _ in range(12)]
    addr = [(ctypes.addressof(b) + 15) & ~15 for b in keep]
    B = _lib.MocBatch(X=addr[0], dtype=dtype, D=D, total_rows=8, n_slides=1, max_rows=8, row_off=addr[1], C=0, Ce=0, topj=0, topk=0)
    S = _lib.MocBankSet(n_banks=n_banks, C=C, image=addr[2])
    for g in range(4):
        S.Ce[g], S.stats[g], S.sel_flag[g] = Ce[g], addr[3 + g], addr[7 + g]
    return B, S, keep, addr


def _refused(B, S, code, text):
    from moc_amd import _lib
    h = _lib.lib()
    rc = h.moc_scores_banks(ctypes.byref(B) if B is not None else None, ctypes.byref(S) if S is not None else None, None)
    msg = h.moc_last_error().decode()
    assert rc == code and text in msg, (rc, msg)


def test_limits_and_sizes():
    from moc_amd import _lib
    h = _lib.lib()
    F32, BF16, F16 = _lib.MOC_F32, _lib.MOC_BF16, _lib.MOC_F16
    # the streaming kernel's n-tile limits (four on fp32 bags, three on 16-bit bags), then 160 KiB of LDS
    assert [h.moc_scores_banks_max(D, F32) for D in (256, 512, 1024, 1536, 2048, 2560)] == [4, 4, 2, 1, 1, 0]
    assert [h.moc_scores_banks_max(D, BF16) for D in (256, 512, 1024, 1536, 1792)] == [3, 3, 1, 1, 0]
    assert h.moc_scores_banks_max(512, F16) == 3 and h.moc_scores_banks_max(500, F32) == 0 and h.moc_scores_banks_max(512, 7) == 0
    for dt in (F32, BF16, F16):
        for n in (1, 2, 4):
            assert h.moc_bank_set_bytes(512, n, dt) == n * h.moc_bank_bytes(512, 16, dt) == n * h.moc_bank_bytes(512, 3, dt)
    assert h.moc_bank_set_bytes(512, 0, F32) == 0


def test_scores_banks_refuses_before_any_launch():
    from moc_amd import _lib
    B, S, keep, _ = _valid()
    _refused(None, S, 1, "null pointer")
    _refused(B, None, 1, "null pointer")
    B, S, keep, _ = _valid(); S.image = None
    _refused(B, S, 1, "null pointer")
    B, S, keep, _ = _valid(); S.stats[1] = None
    _refused(B, S, 1, "null pointer (stats / sel_flag of bank 1)")
    B, S, keep, _ = _valid(); S.sel_flag[0] = None
    _refused(B, S, 1, "null pointer")
    B, S, keep, _ = _valid(); S.stats[3] = None; S.Ce[3] = 99          # (beyond n_banks: not looked at) ... but X is:
    B.X = None
    _refused(B, S, 1, "null X/row_off")
    for n in (0, -1, 5):
        B, S, keep, _ = _valid(n_banks=n)
        _refused(B, S, 1, "outside 1 .. 4")
    for ce in (2, 1, 17, 0):                                            # C < Ce <= 16
        B, S, keep, _ = _valid(Ce=(3, ce, 6, 6))
        _refused(B, S, 1, "bank 1: need C < Ce <= 16")
    B, S, keep, _ = _valid(dtype=_lib.MOC_BF16, n_banks=4)
    _refused(B, S, 1, "at most 3")
    B, S, keep, _ = _valid(D=1024, n_banks=3)
    _refused(B, S, 1, "at most 2")
    B, S, keep, addr = _valid(); B.tile_ticket = addr[11]
    _refused(B, S, 1, "static walk")
    B, S, keep, addr = _valid(); B.cu_reserved = addr[11]
    _refused(B, S, 1, "static walk")
    B, S, keep, _ = _valid(); B.flags = _lib.MOC_STATS_COMPACT
    _refused(B, S, 1, "full statistics layout")
    B, S, keep, _ = _valid(D=2560, n_banks=1)
    _refused(B, S, 2, "160 KiB")
    B, S, keep, _ = _valid(D=1792, dtype=_lib.MOC_F16, n_banks=1)
    _refused(B, S, 2, "160 KiB")
    with pytest.raises(RuntimeError, match="code 2"):
        _lib.check(2, "moc_scores_banks")
    # nothing was written through any of the pointers
    assert all(b.raw == bytes(len(b)) for b in keep)


# ------------------------------------------------------------------ the planner and the chunks
def test_planner_cuts():
    from moc_amd import engine
    P = engine.plan_bank_passes
    assert P(512, torch.float32, 5) == [(0, 4), (4, 1)]
    assert P(512, torch.float32, 4) == [(0, 4)] and P(512, torch.float32, 1) == [(0, 1)]
    assert P(512, torch.bfloat16, 5) == [(0, 3), (3, 2)] and P(512, torch.float16, 7) == [(0, 3), (3, 3), (6, 1)]
    assert P(1024, torch.float32, 5) == [(0, 2), (2, 2), (4, 1)]
    assert P(1024, torch.bfloat16, 2) == [(0, 1), (1, 1)]
    assert P(256, torch.float32, 8) == [(0, 4), (4, 4)]
    with pytest.raises(AssertionError, match="does not fit"):
        P(2560, torch.float32, 2)
    with pytest.raises(AssertionError, match="no bank"):
        P(512, torch.float32, 0)


def test_chunks_count_the_bags_once_and_the_work_arrays_per_bank(monkeypatch):
    from moc_amd import engine, main_moc as M
    assert engine.bank_work_row_bytes(2) == 4 * 7 + 1 + 4 + 8 + 4 * 6 + 4 * 2
    sizes = [100] * 8
    monkeypatch.setattr(M, "MAX_BATCH_BYTES", 100 * 512 * 4 * 4)                   # four slides' bags
    assert M._chunks_banks(sizes, 512, 4, 1, 2) == [[0, 1, 2, 3], [4, 5, 6, 7]] == M._chunks(sizes, 512, 4)
    # work arrays: 73 B a row and bank at two classes; 2048 B of bag a row -- 60 banks' arrays outweigh the bags
    assert M._chunks_banks(sizes, 512, 4, 28, 2) == [[0, 1, 2, 3], [4, 5, 6, 7]]
    assert M._chunks_banks(sizes, 512, 4, 60, 2) == [[0], [1], [2], [3], [4], [5], [6], [7]]
    per = engine.bank_work_row_bytes(2)
    assert 100 * 60 * per * 2 > M.MAX_BATCH_BYTES >= 100 * 60 * per


# ------------------------------------------------------------------ the command line
def _bank_files(tmp_path, name, C=2, Ce=6, D=512):
    fw, fe = tmp_path / f"{name}_W.pt", tmp_path / f"{name}_We.pt"
    torch.save(torch.zeros(D, C), fw)
    torch.save(torch.zeros(D, Ce), fe)
    return f"{name}={fw},{fe}"


def _args(S, tmp_path, banks, extra=()):
    return S.get_args(["--zs", "--topks", "1,10", "--synthetic", "4", "--split", "test", "--out", str(tmp_path / "o"), "--banks"]
                      + list(banks) + list(extra))


def test_cli_bank_argument_checks(tmp_path):
    from moc_amd import sweep as S
    a = _args(S, tmp_path, [_bank_files(tmp_path, "a"), _bank_files(tmp_path, "b", Ce=16)])
    assert [b[0] for b in a.banks] == ["a", "b"] and a.ckpt is None
    banks, sds = S.check_bank_args(a)
    assert [(n, tuple(W.shape), tuple(We.shape)) for n, W, We in banks] == [("a", (512, 2), (512, 6)), ("b", (512, 2), (512, 16))]
    assert sds == []
    for bad in ("a", "=x.pt,y.pt", "a=x.pt", "a=x.pt,y.pt,z.pt", "a/b=x.pt,y.pt"):
        with pytest.raises(SystemExit):
            _args(S, tmp_path, [bad])
    with pytest.raises(SystemExit, match="duplicate bank name 'a'"):
        S.check_bank_args(_args(S, tmp_path, [_bank_files(tmp_path, "a"), _bank_files(tmp_path, "a")]))
    with pytest.raises(SystemExit, match="no such file"):
        S.check_bank_args(_args(S, tmp_path, [_bank_files(tmp_path, "a"), f"c={tmp_path / 'none.pt'},{tmp_path / 'a_We.pt'}"]))
    three = [_bank_files(tmp_path, n) for n in ("a", "b", "c")]
    with pytest.raises(SystemExit, match=r"one per bank \(3\); got 2"):
        S.check_bank_args(_args(S, tmp_path, three, ["--ckpt", "m0.pt", "m1.pt", "--topjs", "5"]))
    with pytest.raises(SystemExit, match="different C"):
        S.check_bank_args(_args(S, tmp_path, [_bank_files(tmp_path, "a"), _bank_files(tmp_path, "d", C=3)]))
    with pytest.raises(SystemExit, match="at most 16"):
        S.check_bank_args(_args(S, tmp_path, [_bank_files(tmp_path, "a"), _bank_files(tmp_path, "w", Ce=17)]))
    # without --banks: one checkpoint, a string, as before
    with pytest.raises(SystemExit):
        S.get_args(["--ckpt", "a.pt", "b.pt", "--topjs", "5", "--topks", "1", "--synthetic", "4", "--split", "test", "--out", "o"])
    a = S.get_args(["--ckpt", "a.pt", "--topjs", "5", "--topks", "1", "--synthetic", "4", "--split", "test", "--out", "o"])
    assert a.ckpt == "a.pt" and a.banks is None


def test_bank_summary_writer(tmp_path):
    from moc_amd import sweep as S
    m = lambda v: {"loss": v, "acc": 0.5, "auc": 1.0 / 3.0}         # noqa: E731
    ev = [{(5, 1, ()): m(0.1), (5, 10, ("topk", "bottomk")): m(0.2)}, {(5, 1, ()): m(0.3), (5, 10, ("topk", "bottomk")): m(0.4)}]
    zs = [{("topj_pooling", 1): m(0.5)}, {("topj_pooling", 1): m(0.6)}]
    rows = S.write_bank_summary(tmp_path, ["a", "b"], ev, zs)
    assert len(rows) == 6
    df = pd.read_csv(tmp_path / "bank_summary.csv", float_precision="round_trip")
    assert list(df.columns) == ["bank", "kind", "topj", "topk", "discard", "loss", "acc", "auc"]
    assert list(df["bank"]) == ["a"] * 3 + ["b"] * 3 and list(df["loss"]) == [0.1, 0.2, 0.5, 0.3, 0.4, 0.6]
    assert list(df["kind"][:3]) == ["eval", "eval", "zs:topj_pooling"] and df["discard"][1] == "topk+bottomk"
    assert df["auc"][0] == 1.0 / 3.0 and pd.isna(df["topj"][2])
    # per bank the rows are those of the bank's own sensitivity.csv
    S.write_sensitivity(tmp_path / "a", ev[0], zs[0])
    one = pd.read_csv(tmp_path / "a" / "sensitivity.csv", float_precision="round_trip")
    pd.testing.assert_frame_equal(df[df["bank"] == "a"].drop(columns="bank").reset_index(drop=True), one, check_exact=True)
    # a zero-shot table alone
    assert len(S.write_bank_summary(tmp_path / "z", ["a", "b"], None, zs)) == 2
