"""Patch maps without a GPU: the new C entry is declared, bound and versioned; the driver's flags parse and its refusals
come before any GPU work; write_patch_maps / load_patch_map round-trip a hand-made map."""
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dense_entry_declared_bound_and_versioned():
    from moc_amd import _lib
    src = open(os.path.join(ROOT, "include", "moc_hip.h")).read()
    assert re.search(r"int\s+moc_meta_forward_dense\s*\(", src)
    assert int(re.search(r"#define MOC_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION == 20
    assert "moc_meta_forward_dense" in _lib.SIGNATURES
    h = _lib.lib()
    assert hasattr(h, "moc_meta_forward_dense") and h.moc_version() == 20


def test_dense_entry_refuses_bad_batches_on_the_host():
    """Errors, not faults: a masked batch or one without statistics is refused before anything is launched."""
    import ctypes
    from moc_amd import _lib
    h = _lib.lib()
    b = _lib.MocBatch(X=16, dtype=_lib.MOC_BF16, D=512, total_rows=100, n_slides=1, max_rows=100, row_off=16,
                      C=2, Ce=6, topj=10, topk=5, mask=16, kept=16, n_kept=16, stats=16)
    m = _lib.MocMeta(W1=16, b1=16, W2=16, b2=16, W1_image=16, H=64, D=512)
    mixed = ctypes.c_void_p(16)
    rc = h.moc_meta_forward_dense(ctypes.byref(b), ctypes.byref(m), None, mixed, 0, 1, 15, None)
    assert rc == 1 and b"masked" in h.moc_last_error()
    b.mask = None
    b.stats = None
    rc = h.moc_meta_forward_dense(ctypes.byref(b), ctypes.byref(m), None, mixed, 0, 1, 15, None)
    assert rc == 1 and b"statistics" in h.moc_last_error()
    b.stats = 16
    rc = h.moc_meta_forward_dense(ctypes.byref(b), ctypes.byref(m), None, None, 0, 1, 15, None)
    assert rc == 1 and b"null mixed" in h.moc_last_error()
    rc = h.moc_meta_forward_dense(ctypes.byref(b), ctypes.byref(m), None, mixed, 0, 2, 15, None)
    assert rc == 1 and b"slide range" in h.moc_last_error()


def test_patch_map_flags_parse():
    from moc_amd import run_moc as R
    a = R.get_args([])
    assert a.patch_maps is None and a.patch_maps_from is None and R.patch_map_splits(a) == []
    assert R.patch_map_splits(R.get_args(["--patch_maps", "none"])) == []
    assert R.patch_map_splits(R.get_args(["--patch_maps", "val"])) == ["val"]
    assert R.patch_map_splits(R.get_args(["--patch_maps", "all"])) == ["train", "val", "test"]
    a = R.get_args(["--patch_maps_from", "best.pt"])
    assert a.patch_maps_from == "best.pt" and R.patch_map_splits(a) == ["test"]
    assert R.patch_map_splits(R.get_args(["--patch_maps_from", "best.pt", "--patch_maps", "train"])) == ["train"]
    with pytest.raises(SystemExit):
        R.get_args(["--patch_maps", "everything"])


@pytest.mark.parametrize("extra", [["--patch_maps", "test"], ["--patch_maps_from", "best.pt"]])
def test_patch_map_refusals_come_before_the_gpu(monkeypatch, extra):
    import torch
    from moc_amd import run_moc as R

    def no_gpu(*a, **k):
        raise AssertionError("touched the GPU")
    monkeypatch.setattr(torch.cuda, "is_available", no_gpu)
    monkeypatch.setattr(R, "prepare", no_gpu)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one-GPU"):
        R.cli(["--seed", "1"] + extra)
    monkeypatch.setenv("WORLD_SIZE", "1")
    with pytest.raises(SystemExit, match="--folds"):
        R.cli(["--folds", "0,1"] + extra)
    with pytest.raises(SystemExit, match="ablation"):
        R.cli(["--ablation_study", "avg"] + extra)


def test_no_patch_map_flag_changes_nothing(monkeypatch):
    from moc_amd import run_moc as R
    monkeypatch.setenv("WORLD_SIZE", "2")
    R.check_patch_map_args(R.get_args(["--folds", "0,1", "--ablation_study", "avg"]))     # no refusal without the flags


def _hand_made(rng, N=37, C=3, K=5, with_model=True):
    from moc_amd.patch_maps import PatchMap
    coords = rng.integers(0, 100000, size=(N, 2)).astype(np.int64)
    m = PatchMap(path="/data/pt_files/slide_A.pt", label=2, pred=1,
                 pooled=rng.standard_normal(C).astype(np.float32), coords=coords,
                 logits=rng.standard_normal((N, C)).astype(np.float32),
                 selected=rng.random(N) < 0.3,
                 zs_evidence=np.stack([rng.permutation(N)[:K] for _ in range(C)]).astype(np.int64))
    if with_model:
        m.gates = rng.random((N, 4)).astype(np.float32)
        m.mixed = rng.standard_normal((N, C)).astype(np.float32)
        m.evidence = np.stack([rng.permutation(N)[:K] for _ in range(C)]).astype(np.int64)
    return m


@pytest.mark.parametrize("with_model", [True, False])
def test_write_and_load_round_trip(tmp_path, with_model):
    import torch
    from moc_amd import patch_maps as PM
    rng = np.random.default_rng(7)
    maps = [_hand_made(rng, with_model=with_model), _hand_made(rng, N=9, K=9, with_model=with_model)]
    maps[1].path = "/data/npy_files/slide_B.npy"
    index = PM.write_patch_maps(maps, str(tmp_path / "out"))
    assert sorted(os.listdir(tmp_path / "out")) == ["index.json", "slide_A.npz", "slide_B.npz"]
    on_disk = json.load(open(tmp_path / "out" / "index.json"))
    assert on_disk == index and list(on_disk) == ["slide_A", "slide_B"]
    for m, sid in zip(maps, ("slide_A", "slide_B")):
        e = on_disk[sid]
        assert e["file"] == f"{sid}.npz" and e["label"] == m.label and e["pred"] == m.pred
        exp = torch.softmax(torch.from_numpy(m.pooled)[None] * 56.3477, dim=1)[0].numpy()
        np.testing.assert_allclose(e["probabilities"], exp, rtol=0, atol=1e-7)
        got = PM.load_patch_map(str(tmp_path / "out" / e["file"]))
        assert got.path == m.path and got.label == m.label and got.pred == m.pred
        for f in ("pooled", "coords", "logits", "selected", "zs_evidence", "gates", "mixed", "evidence"):
            a, b = getattr(m, f), getattr(got, f)
            if a is None:
                assert b is None, f
            else:
                assert a.dtype == b.dtype and np.array_equal(a, b), f
        z = np.load(str(tmp_path / "out" / e["file"]))
        if with_model:
            assert np.array_equal(z["evidence_coords"], m.coords[m.evidence])
            assert z["evidence_coords"].shape == m.evidence.shape + (2,)
        else:
            assert "evidence_coords" not in z.files
        assert np.array_equal(z["zs_evidence_coords"], m.coords[m.zs_evidence])


def test_explicit_slide_ids(tmp_path):
    from moc_amd import patch_maps as PM
    rng = np.random.default_rng(3)
    maps = [_hand_made(rng), _hand_made(rng)]             # same path twice: ids must be given
    with pytest.raises(AssertionError):
        PM.write_patch_maps(maps, str(tmp_path / "a"))
    PM.write_patch_maps(maps, str(tmp_path / "b"), slide_ids=["s1", "s2"])
    assert set(json.load(open(tmp_path / "b" / "index.json"))) == {"s1", "s2"}

