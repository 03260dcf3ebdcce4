"""Prediction without a GPU: the R-model entry is declared, bound, named in INTEGRATION.md and the ABI is still 20; its
host-side refusals come before any launch; the CLI parses and refuses before any GPU work; the output files round-trip."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_models_entry_declared_bound_documented_abi_20():
    from moc_amd import _lib
    src = open(os.path.join(ROOT, "include", "moc_hip.h")).read()
    assert re.search(r"int\s+moc_meta_forward_models\s*\(", src)
    assert int(re.search(r"#define MOC_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION == 20
    assert "moc_meta_forward_models" in _lib.SIGNATURES
    assert "moc_meta_forward_models" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    h = _lib.lib()
    assert hasattr(h, "moc_meta_forward_models") and h.moc_version() == 20


def _fakes(R=2):
    from moc_amd import _lib
    h = _lib.lib()
    b = _lib.MocBatch(X=16, dtype=_lib.MOC_BF16, D=512, total_rows=100, n_slides=1, max_rows=100, row_off=16,
                      C=2, Ce=6, topj=10, topk=5, mask=None, stats=16, sel_flag=16, sel_idx=16, sel_row=16, n_sel=16, cand=16)
    m = _lib.MocMeta(W1=16, b1=16, W2=16, b2=16, W1_image=16, H=64, D=512)
    img = h.moc_w1_image_bytes(512, _lib.MOC_BF16)
    runs = _lib.MocRuns(n_runs=R, slide_stride=0, par_stride=64 * 512 + 64 + 256 + 4, image_stride=img)
    return h, b, m, runs, ctypes.c_void_p(16)


def _call(h, b, m, runs, mixed, slide0=0, n=1):
    return h.moc_meta_forward_models(ctypes.byref(b), ctypes.byref(m), ctypes.byref(runs), mixed, slide0, n, 15, None)


@pytest.mark.parametrize("what, fix, msg", [
    ("mask", lambda b, m, r: setattr(b, "mask", 16), b"mask"),
    ("kept", lambda b, m, r: (setattr(b, "mask", 16), setattr(b, "kept", 16), setattr(b, "n_kept", 16)), b"masked"),
    ("stats", lambda b, m, r: setattr(b, "stats", None), b"phase-A"),
    ("n_sel", lambda b, m, r: setattr(b, "n_sel", None), b"phase-A"),
    ("runs0", lambda b, m, r: setattr(r, "n_runs", 0), b"n_runs=0"),
    ("runs17", lambda b, m, r: setattr(r, "n_runs", 17), b"n_runs=17"),
    ("image", lambda b, m, r: setattr(r, "image_stride", r.image_stride - 16), b"image_stride"),
    ("slide_stride", lambda b, m, r: setattr(r, "slide_stride", 1), b"slide_stride"),
    ("par_stride", lambda b, m, r: setattr(r, "par_stride", 100), b"par_stride"),
    ("D", lambda b, m, r: setattr(m, "D", 1024), b"meta D"),
])
def test_models_entry_refuses_on_the_host(what, fix, msg):
    """Errors, not faults: every refusal returns rc 1 with a message (the fake device pointers are never touched --
    a launch would fault on them)."""
    h, b, m, runs, mixed = _fakes()
    fix(b, m, runs)
    assert _call(h, b, m, runs, mixed) == 1
    assert msg in h.moc_last_error(), h.moc_last_error()


def test_models_entry_refuses_null_mixed_and_bad_range():
    h, b, m, runs, mixed = _fakes()
    assert _call(h, b, m, runs, None) == 1 and b"null mixed" in h.moc_last_error()
    assert _call(h, b, m, runs, mixed, 0, 2) == 1 and b"slide range" in h.moc_last_error()
    assert h.moc_meta_forward_models(ctypes.byref(b), ctypes.byref(m), None, mixed, 0, 1, 15, None) == 1


def test_cli_parses():
    from moc_amd import predict as P
    a = P.get_args(["--ckpt", "a.pt", "b.pt", "--out", "o", "--synthetic", "24", "--shot", "4", "--split", "test"])
    assert a.ckpt == ["a.pt", "b.pt"] and a.synthetic == 24 and a.split == "test" and a.topj == 10 and a.topk == 10
    a = P.get_args(["--ckpt", "a.pt", "--out", "o", "--slides", "s.csv", "--data_dir", "d", "--bag_dtype", "bf16",
                    "--discard_classifiers", "delta_diff", "--topj", "400"])
    assert a.slides == "s.csv" and a.bag_dtype == "bf16" and a.discard_classifiers == ["delta_diff"] and a.topj == 400
    with pytest.raises(SystemExit):
        P.get_args(["--out", "o"])
    with pytest.raises(SystemExit):
        P.get_args(["--ckpt", "a.pt", "--out", "o", "--split", "holdout"])


def _ckpt(path, D=512, bad=False):
    from moc_amd.main_moc import senet
    sd = senet(D, 4).state_dict() if not bad else {"weight": torch.zeros(3)}
    torch.save(sd, path)
    return str(path)


def test_cli_refusals_come_before_the_gpu(monkeypatch, tmp_path):
    from moc_amd import predict as P

    def no_gpu(*a, **k):
        raise AssertionError("touched the GPU")
    monkeypatch.setattr(torch.cuda, "is_available", no_gpu)
    monkeypatch.setattr(P, "predict", no_gpu)
    good = _ckpt(tmp_path / "a.pt")
    base = ["--out", str(tmp_path / "o"), "--synthetic", "8", "--split", "test"]
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one-GPU"):
        P.cli(["--ckpt", good] + base)
    monkeypatch.setenv("WORLD_SIZE", "1")
    with pytest.raises(SystemExit, match="senet"):
        P.cli(["--ckpt", good, _ckpt(tmp_path / "bad.pt", bad=True)] + base)
    with pytest.raises(SystemExit, match="disagree"):
        P.cli(["--ckpt", good, _ckpt(tmp_path / "d1024.pt", D=1024)] + base)
    with pytest.raises(SystemExit, match="1 .. 16"):
        P.cli(["--ckpt"] + [good] * 17 + base)
    with pytest.raises(SystemExit, match="exactly one"):
        P.cli(["--ckpt", good, "--slides", "x.csv", "--data_dir", "d"] + base)
    with pytest.raises(SystemExit, match="--split"):
        P.cli(["--ckpt", good, "--out", "o", "--synthetic", "8"])
    csv = tmp_path / "s.csv"
    csv.write_text("slide_id,label\nA,0\nB,1\nA,1\n")
    with pytest.raises(SystemExit, match="more than once"):
        P.cli(["--ckpt", good, "--out", "o", "--slides", str(csv), "--data_dir", str(tmp_path)])
    with pytest.raises(SystemExit, match="--data_dir"):
        P.cli(["--ckpt", good, "--out", "o", "--slides", str(csv)])


@pytest.mark.parametrize("labeled", [True, False])
def test_write_and_load_round_trip(tmp_path, labeled):
    from moc_amd import predict as P
    rng = np.random.default_rng(5)
    R, N, C = 3, 7, 3
    pooled = rng.standard_normal((R, N, C)).astype(np.float32) * 0.05
    probs = P._probs(pooled)
    ens = probs.mean(axis=0, dtype=np.float64).astype(np.float32)
    p = P.Predictions(slide_ids=[f"s{i:02d}" for i in range(N)], paths=[f"/d/pt_files/s{i:02d}.pt" for i in range(N)],
                      classes=["KICH", "KIRC", "KIRP"], pooled=pooled, probs=probs, ensemble=ens,
                      pred=ens.argmax(1).astype(np.int64), labels=rng.integers(0, C, N).astype(np.int64) if labeled else None)
    info = {"args": {"topj": 10}, "checkpoints": ["a.pt", "b.pt", "c.pt"]}
    doc = P.write_predictions(p, str(tmp_path / "out"), info, {"ensemble": {"auc": 0.5}} if labeled else None)
    assert sorted(os.listdir(tmp_path / "out")) == ["predictions.csv", "predictions.json"]
    import json
    on_disk = json.load(open(tmp_path / "out" / "predictions.json"))
    assert on_disk == doc and on_disk["checkpoints"] == info["checkpoints"] and on_disk["n_models"] == R
    assert ("metrics" in on_disk) == labeled
    import pandas as pd
    cols = list(pd.read_csv(tmp_path / "out" / "predictions.csv").columns)
    assert cols[:6] == ["slide_id", "path", "pred", "prob_KICH", "prob_KIRC", "prob_KIRP"]
    assert "m2_prob_KIRP" in cols and ("label" in cols) == labeled
    q = P.load_predictions(str(tmp_path / "out"))
    assert q.slide_ids == p.slide_ids and q.paths == p.paths and q.classes == p.classes
    for f in ("pooled", "probs", "ensemble", "pred", "labels"):
        a, b = getattr(p, f), getattr(q, f)
        if a is None:
            assert b is None
        else:
            assert a.dtype == b.dtype and np.array_equal(a, b), f


def test_ensemble_metrics_on_hand_made_predictions():
    import types
    from moc_amd import predict as P
    pooled = np.array([[[0.0, 0.1], [0.1, 0.0], [0.0, 0.2]], [[0.0, 0.05], [0.0, 0.01], [0.3, 0.0]]], dtype=np.float32)
    probs = P._probs(pooled)
    ens = probs.mean(0).astype(np.float32)
    p = P.Predictions(slide_ids=["a", "b", "c"], paths=["a", "b", "c"], classes=["0", "1"], pooled=pooled, probs=probs,
                      ensemble=ens, pred=ens.argmax(1), labels=np.array([1, 0, 1]))
    m = P.metrics(p, types.SimpleNamespace(pretrain="conch"))
    assert len(m["models"]) == 2 and m["models"][0]["acc"] == 1.0
    assert m["ensemble"]["acc"] == float((ens.argmax(1) == p.labels).mean())
    np.testing.assert_allclose(m["ensemble"]["loss"], -np.mean(np.log(ens[np.arange(3), p.labels].astype(np.float64))), rtol=1e-12)
