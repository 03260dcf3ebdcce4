"""Ensemble patch maps without a GPU: the dense R-model entry is declared, bound, named in INTEGRATION.md and the ABI is
still 20; every host-side refusal comes before any launch; predict parses --patch_maps and still refuses before any GPU
work; an ensemble map written from hand-made arrays loads back unchanged."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dense_models_entry_declared_bound_documented_abi_20():
    from moc_amd import _lib
    src = open(os.path.join(ROOT, "include", "moc_hip.h")).read()
    assert re.search(r"int\s+moc_meta_forward_dense_models\s*\(", src)
    assert int(re.search(r"#define MOC_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION == 20
    assert "moc_meta_forward_dense_models" in _lib.SIGNATURES
    assert "moc_meta_forward_dense_models" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    h = _lib.lib()
    assert hasattr(h, "moc_meta_forward_dense_models") and h.moc_version() == 20


def _fakes(R=2):
    from moc_amd import _lib
    h = _lib.lib()
    b = _lib.MocBatch(X=16, dtype=_lib.MOC_BF16, D=512, total_rows=100, n_slides=1, max_rows=100, row_off=16,
                      C=2, Ce=6, topj=10, topk=5, mask=None, stats=16, sel_flag=16, sel_idx=16, sel_row=16, n_sel=16, cand=16)
    m = _lib.MocMeta(W1=16, b1=16, W2=16, b2=16, W1_image=16, H=64, D=512)
    img = h.moc_w1_image_bytes(512, _lib.MOC_BF16)
    runs = _lib.MocRuns(n_runs=R, slide_stride=0, par_stride=64 * 512 + 64 + 256 + 4, image_stride=img)
    return h, b, m, runs, ctypes.c_void_p(16)


def _call(h, b, m, runs, mean, scale=56.3477, slide0=0, n=1, std=16, gates=16):
    return h.moc_meta_forward_dense_models(ctypes.byref(b), ctypes.byref(m), ctypes.byref(runs), scale, mean, std, gates,
                                           slide0, n, 15, None)


@pytest.mark.parametrize("what, fix, msg", [
    ("mask", lambda b, m, r: setattr(b, "mask", 16), b"mask"),
    ("stats", lambda b, m, r: setattr(b, "stats", None), b"statistics"),
    ("runs0", lambda b, m, r: setattr(r, "n_runs", 0), b"n_runs=0"),
    ("runs17", lambda b, m, r: setattr(r, "n_runs", 17), b"n_runs=17"),
    ("slide_stride", lambda b, m, r: setattr(r, "slide_stride", 1), b"slide_stride"),
    ("par_stride", lambda b, m, r: setattr(r, "par_stride", 100), b"par_stride"),
    ("image", lambda b, m, r: setattr(r, "image_stride", r.image_stride - 16), b"image_stride"),
    ("D", lambda b, m, r: setattr(m, "D", 1024), b"meta D"),
    ("C", lambda b, m, r: (setattr(b, "C", 65), setattr(b, "Ce", 70)), b"C=65"),
])
def test_dense_models_entry_refuses_on_the_host(what, fix, msg):
    """Errors, not faults: every refusal returns rc 1 with a message (the fake device pointers are never touched --
    a launch would fault on them)."""
    h, b, m, runs, mean = _fakes()
    fix(b, m, runs)
    assert _call(h, b, m, runs, mean) == 1
    assert msg in h.moc_last_error(), h.moc_last_error()


def test_dense_models_entry_refuses_null_mean_bad_range_and_scale():
    h, b, m, runs, mean = _fakes()
    assert _call(h, b, m, runs, None) == 1 and b"null prob_mean" in h.moc_last_error()
    assert _call(h, b, m, runs, mean, slide0=0, n=2) == 1 and b"slide range" in h.moc_last_error()
    assert _call(h, b, m, runs, mean, slide0=-1) == 1 and b"slide range" in h.moc_last_error()
    assert _call(h, b, m, runs, mean, n=0) == 1 and b"slide range" in h.moc_last_error()
    for bad in (math.inf, -math.inf, math.nan):
        assert _call(h, b, m, runs, mean, scale=bad) == 1 and b"not finite" in h.moc_last_error()
    assert h.moc_meta_forward_dense_models(ctypes.byref(b), ctypes.byref(m), None, 56.3477, mean, None, None,
                                           0, 1, 15, None) == 1


def test_cli_parses_patch_maps():
    from moc_amd import predict as P
    a = P.get_args(["--ckpt", "a.pt", "b.pt", "--out", "o", "--synthetic", "24", "--shot", "4", "--split", "test",
                    "--patch_maps"])
    assert a.patch_maps is True and a.ckpt == ["a.pt", "b.pt"]
    assert P.get_args(["--ckpt", "a.pt", "--out", "o", "--synthetic", "8", "--split", "test"]).patch_maps is False


def test_patch_maps_refusals_come_before_the_gpu(monkeypatch, tmp_path):
    from moc_amd import predict as P
    from moc_amd.main_moc import senet

    def no_gpu(*a, **k):
        raise AssertionError("touched the GPU")
    monkeypatch.setattr(torch.cuda, "is_available", no_gpu)
    monkeypatch.setattr(P, "predict", no_gpu)
    good = str(tmp_path / "a.pt")
    torch.save(senet(512, 4).state_dict(), good)
    base = ["--out", str(tmp_path / "o"), "--synthetic", "8", "--split", "test", "--patch_maps"]
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one-GPU"):
        P.cli(["--ckpt", good] + base)
    monkeypatch.setenv("WORLD_SIZE", "1")
    with pytest.raises(SystemExit, match="1 .. 16"):
        P.cli(["--ckpt"] + [good] * 17 + base)
    with pytest.raises(SystemExit, match="--split"):
        P.cli(["--ckpt", good, "--out", "o", "--synthetic", "8", "--patch_maps"])
    with pytest.raises(SystemExit, match="exactly one"):
        P.cli(["--ckpt", good, "--slides", "x.csv", "--data_dir", "d"] + base)


def _map(rng, R, C, N, K, label):
    from moc_amd.patch_maps import EnsembleMap
    k = min(K, N)
    pm = rng.random((N, C)).astype(np.float32)
    probs = rng.random(C).astype(np.float32)
    return EnsembleMap(path=f"/d/pt_files/s{N}.pt", label=label, pred=int(probs.argmax()), probabilities=probs,
                       pooled=rng.standard_normal((R, C)).astype(np.float32),
                       coords=rng.integers(0, 90000, (N, 2)).astype(np.int64),
                       logits=rng.standard_normal((N, C)).astype(np.float32), selected=rng.random(N) < 0.3,
                       zs_evidence=rng.integers(0, N, (C, k)).astype(np.int64), prob_mean=pm,
                       prob_std=(pm * 0.1).astype(np.float32), gates_mean=rng.random((N, 4)).astype(np.float32),
                       evidence=rng.integers(0, N, (R, C, k)).astype(np.int64))


def test_ensemble_maps_round_trip(tmp_path):
    from dataclasses import fields
    from moc_amd.patch_maps import EnsembleMap, load_ensemble_map, write_ensemble_maps
    rng = np.random.default_rng(3)
    maps = [_map(rng, 3, 2, 40, 10, 1), _map(rng, 3, 2, 7, 10, -1), _map(rng, 1, 30, 300, 5, 0)]
    ids = ["lab", "unlab", "c30"]
    out = tmp_path / "maps"
    index = write_ensemble_maps(maps, str(out), ids)
    assert sorted(os.listdir(out)) == ["c30.npz", "index.json", "lab.npz", "unlab.npz"]
    assert json.load(open(out / "index.json")) == index
    for sid, m in zip(ids, maps):
        e = index[sid]
        assert e["label"] == m.label and e["pred"] == m.pred and e["file"] == f"{sid}.npz"
        assert np.array_equal(np.asarray(e["probabilities"], dtype=np.float32), m.probabilities)
        q = load_ensemble_map(str(out / e["file"]))
        for f in fields(EnsembleMap):
            a, b = getattr(m, f.name), getattr(q, f.name)
            if isinstance(a, np.ndarray):
                assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (sid, f.name)
            else:
                assert a == b and type(a) is type(b), (sid, f.name)
        with np.load(out / e["file"]) as z:
            assert np.array_equal(z["evidence_coords"], m.coords[m.evidence])
            assert z["evidence_coords"].shape == m.evidence.shape + (2,)
            assert np.array_equal(z["zs_evidence_coords"], m.coords[m.zs_evidence])
