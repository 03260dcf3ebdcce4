"""Sensitivity sweeps without a GPU: moc_topk_mean_multi is declared, bound, exported and documented with the ABI still
20; its host-side refusals come before any launch; the sweep CLI parses its lists and discard sets; the JSON / CSV writer
is a pure function."""
import ctypes
import json
import os
import re

import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_multi_entry_declared_bound_exported_documented_abi_20():
    from moc_amd import _lib
    src = open(os.path.join(ROOT, "include", "moc_hip.h")).read()
    assert re.search(r"int\s+moc_topk_mean_multi\s*\(", src)
    assert int(re.search(r"#define MOC_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION == 20
    assert "moc_topk_mean_multi" in _lib.SIGNATURES
    assert "moc_topk_mean_multi" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    h = _lib.lib()
    assert hasattr(h, "moc_topk_mean_multi") and h.moc_version() == 20


def _call(h, Ks, n_K=None, pooled=16, keys=16):
    """Fake device pointers: never touched -- a launch would fault on them, a refusal returns first."""
    arr = (ctypes.c_int32 * max(len(Ks), 1))(*Ks)
    return h.moc_topk_mean_multi(keys, 100, 16, 100, 16, None, 1, 2, ctypes.cast(arr, ctypes.c_void_p),
                                 len(Ks) if n_K is None else n_K, 0, pooled, None, None, None)


@pytest.mark.parametrize("Ks, n_K, msg", [
    ([1], 0, b"n_K=0"),
    ([1] * 9, 9, b"n_K=9"),
    ([5, 0], None, b"K=0"),
    ([5, 65, 1], None, b"K=65"),
])
def test_multi_entry_refuses_bad_k_lists_on_the_host(Ks, n_K, msg):
    from moc_amd import _lib
    h = _lib.lib()
    assert _call(h, Ks, n_K) == 1
    assert msg in h.moc_last_error(), h.moc_last_error()
    with pytest.raises(AssertionError):
        _lib.check(1, "moc_topk_mean_multi")


def test_multi_entry_refuses_null_pointers():
    from moc_amd import _lib
    h = _lib.lib()
    assert _call(h, [1, 5], pooled=None) == 1 and b"null pointer" in h.moc_last_error()
    assert _call(h, [1, 5], keys=None) == 1 and b"null pointer" in h.moc_last_error()
    assert h.moc_topk_mean_multi(16, 100, 16, 100, 16, None, 1, 2, None, 1, 0, 16, None, None, None) == 1
    assert b"null pointer" in h.moc_last_error()


def test_cli_parses_lists_and_discard_sets():
    from moc_amd import sweep as S
    a = S.get_args(["--ckpt", "best.pt", "--topjs", "100,200,400,800", "--topks", "1,5,10,20,50", "--discard_sets", "none",
                    "topk", "delta_softmax+delta_diff", "topk+bottomk", "--synthetic", "12", "--shot", "2", "--split", "test",
                    "--out", "o"])
    assert a.topjs == [100, 200, 400, 800] and a.topks == [1, 5, 10, 20, 50]
    assert a.discard_sets == [(), ("topk",), ("delta_softmax", "delta_diff"), ("topk", "bottomk")]
    assert a.ckpt == "best.pt" and not a.zs and a.split == "test" and a.pretrain == "conch"
    a = S.get_args(["--ckpt", "b.pt", "--topjs", "10", "--topks", "3", "--split", "val", "--out", "o"])
    assert a.discard_sets == [()] and a.topjs == [10] and a.topks == [3]
    assert S.parse_discard_set("none") == () and S.discard_name(()) == "none"
    assert S.discard_name(("topk", "bottomk")) == "topk+bottomk"


def test_cli_zs_alone_needs_no_checkpoint():
    from moc_amd import sweep as S
    a = S.get_args(["--zs", "--topks", "1,10,64", "--synthetic", "12", "--split", "test", "--out", "o"])
    assert a.ckpt is None and a.zs and a.topks == [1, 10, 64]
    assert S.check_args(a) is None


@pytest.mark.parametrize("argv", [
    ["--topks", "1,5", "--split", "test", "--out", "o"],                                   # neither --ckpt nor --zs
    ["--ckpt", "b.pt", "--topks", "1,5", "--split", "test", "--out", "o"],                 # --ckpt without --topjs
    ["--ckpt", "b.pt", "--topjs", "10", "--topks", "1,65", "--split", "test", "--out", "o"],   # K above 64
    ["--ckpt", "b.pt", "--topjs", "10", "--topks", "0", "--split", "test", "--out", "o"],
    ["--ckpt", "b.pt", "--topjs", "10,x", "--topks", "1", "--split", "test", "--out", "o"],
    ["--ckpt", "b.pt", "--topjs", "10", "--topks", "1", "--discard_sets", "topk+nonsense", "--split", "test", "--out", "o"],
    ["--ckpt", "b.pt", "--topjs", "10", "--topks", "1", "--discard_sets", "topk+topk", "--split", "test", "--out", "o"],
    ["--ckpt", "b.pt", "--topjs", "10", "--topks", "1", "--split", "holdout", "--out", "o"],
])
def test_cli_refuses(argv):
    from moc_amd import sweep as S
    with pytest.raises(SystemExit):
        S.get_args(argv)


def test_cli_checks_before_gpu_work(tmp_path):
    from moc_amd import sweep as S
    with pytest.raises(SystemExit, match="split"):
        S.check_args(S.get_args(["--zs", "--topks", "1", "--synthetic", "12", "--out", "o"]))
    csv = tmp_path / "s.csv"
    pd.DataFrame({"slide_id": ["a", "b"]}).to_csv(csv, index=False)
    with pytest.raises(SystemExit, match="label"):
        S.check_args(S.get_args(["--zs", "--topks", "1", "--slides", str(csv), "--data_dir", "d", "--out", "o"]))
    with pytest.raises(SystemExit, match="data_dir"):
        S.check_args(S.get_args(["--zs", "--topks", "1", "--slides", str(csv), "--out", "o"]))


def test_writer_on_a_hand_made_table(tmp_path):
    from moc_amd import sweep as S
    ev = {(5, 1, ()): {"loss": 0.1, "acc": 0.75, "auc": 1.0 / 3.0},
          (5, 10, ()): {"loss": 0.2, "acc": 0.5, "auc": 0.9},
          (40, 1, ("topk", "bottomk")): {"loss": 0.30000000000000004, "acc": 1.0, "auc": 0.8},
          (40, 10, ("topk", "bottomk")): {"loss": 0.4, "acc": 0.25, "auc": 0.7}}
    zs = {("topj_pooling", 1): {"loss": 1.5, "acc": 0.5, "auc": 0.6},
          ("bottomk_irrel_classifier_pooling", 10): {"loss": 2.5, "acc": 0.25, "auc": 0.55}}
    doc = S.write_sensitivity(str(tmp_path / "o"), ev, zs, {"topjs": [5, 40], "topks": [1, 10]})
    back = json.load(open(tmp_path / "o" / "sensitivity.json"))
    assert back == doc and back["args"] == {"topjs": [5, 40], "topks": [1, 10]}
    assert back["evaluation"]["topj=5,topk=1,discard=none"] == ev[(5, 1, ())]                 # the same floats
    assert back["evaluation"]["topj=40,topk=1,discard=topk+bottomk"] == ev[(40, 1, ("topk", "bottomk"))]
    assert back["zero_shot"]["topj_pooling,topk=1"] == zs[("topj_pooling", 1)]
    assert len(back["evaluation"]) == 4 and len(back["zero_shot"]) == 2
    df = pd.read_csv(tmp_path / "o" / "sensitivity.csv", float_precision="round_trip")
    assert list(df.columns) == ["kind", "topj", "topk", "discard", "loss", "acc", "auc"] and len(df) == 6
    e = df[df["kind"] == "eval"]
    assert e["topj"].tolist() == [5, 5, 40, 40] and e["topk"].tolist() == [1, 10, 1, 10]
    assert e["discard"].tolist() == ["none", "none", "topk+bottomk", "topk+bottomk"]
    assert e["loss"].tolist() == [0.1, 0.2, 0.30000000000000004, 0.4] and e["auc"].tolist()[0] == 1.0 / 3.0
    z = df[df["kind"] != "eval"]
    assert z["kind"].tolist() == ["zs:topj_pooling", "zs:bottomk_irrel_classifier_pooling"] and z["topj"].isna().all()
    # one table alone
    doc = S.write_sensitivity(str(tmp_path / "z"), None, zs, None)
    assert "evaluation" not in doc and len(pd.read_csv(tmp_path / "z" / "sensitivity.csv")) == 2
