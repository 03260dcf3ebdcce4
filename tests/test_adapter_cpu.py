"""The fused adapter forward without a GPU: the two C entries are exported and bound, every contract violation of
moc_adapter_logits is refused on the host with a message that names the argument, `fused` is off by default, and a
module with `fused = True` on the CPU falls back to the torch path bit for bit."""
import contextlib
import ctypes
import io
import math

import pytest
import torch

import helpers_baselines as HB
from oracle import baselines_oracle as BO


def test_library_exports_the_adapter_entries():
    from moc_amd import _lib
    h = _lib.lib()
    assert hasattr(h, "moc_adapter_workspace") and hasattr(h, "moc_adapter_logits")
    assert "moc_adapter_workspace" in _lib.SIGNATURES and "moc_adapter_logits" in _lib.SIGNATURES
    assert h.moc_version() == _lib.ABI_VERSION
    # 768 KiB of bf16-term images per expert + the transposed classifier
    assert h.moc_adapter_workspace(15000, 512, 128, 1, 2) == 768 * 1024 + 2 * 512 * 4
    assert h.moc_adapter_workspace(1, 512, 128, 8, 64) == 8 * 768 * 1024 + 64 * 512 * 4
    for bad in [(0, 512, 128, 1, 2), (5, 256, 128, 1, 2), (5, 512, 64, 1, 2), (5, 512, 128, 0, 2), (5, 512, 128, 9, 2),
                (5, 512, 128, 1, 0), (5, 512, 128, 1, 65)]:
        assert h.moc_adapter_workspace(*bad) == 0, bad


def _call(lib_, **over):
    """moc_adapter_logits with made-up (never dereferenced) 16-byte aligned addresses; `over` replaces arguments."""
    E = over.get("E", 1)
    a = dict(X=0x1000, N=100, c=512, W1=[0x2000 + 0x100 * e for e in range(max(E, 1))],
             W2=[0x4000 + 0x100 * e for e in range(max(E, 1))], h=128, E=E, G=None if E == 1 else 0x6000, Wc=0x7000, C=2,
             ratio=0.1, logits=0x8000, ws=0x9000, ws_bytes=1 << 30)
    a.update(over)
    arr = lambda v: None if v is None else ctypes.cast((ctypes.c_void_p * len(v))(*v), ctypes.c_void_p)
    rc = lib_.moc_adapter_logits(a["X"], a["N"], a["c"], arr(a["W1"]), arr(a["W2"]), a["h"], a["E"], a["G"], a["Wc"], a["C"],
                              ctypes.c_float(a["ratio"]), a["logits"], a["ws"], a["ws_bytes"], None)
    return rc, lib_.moc_last_error().decode()


@pytest.mark.parametrize("over,word", [
    (dict(X=None), "X"), (dict(W1=None), "W1"), (dict(W2=None), "W2"), (dict(Wc=None), "Wc"), (dict(logits=None), "logits"),
    (dict(ws=None), "workspace"), (dict(W1=[None]), "W1[0]"), (dict(E=3, W2=[0x4000, 0x4100, None]), "W2[2]"),
    (dict(N=0), "N="), (dict(c=256), "c=256"), (dict(h=64), "h=64"), (dict(E=0), "E=0"), (dict(E=9), "E=9"),
    (dict(C=0), "C=0"), (dict(C=65), "C=65"),
    (dict(G=0x6000), "G"), (dict(E=2, G=None), "G"),
    (dict(X=0x1004), "X"), (dict(W1=[0x2008]), "W1[0]"), (dict(E=2, W2=[0x4000, 0x4104]), "W2[1]"), (dict(E=2, G=0x6004), "G"),
    (dict(ws=0x9008), "workspace"),
    (dict(ws_bytes=768 * 1024 + 4096 - 1), "workspace_bytes"),
    (dict(ratio=math.nan), "ratio"), (dict(ratio=math.inf), "ratio"),
])
def test_adapter_logits_refuses_on_the_host(over, word):
    from moc_amd import _lib
    rc, msg = _call(_lib.lib(), **over)
    assert rc != 0 and msg.startswith("moc_adapter_logits") and word in msg, (rc, msg)


def test_engine_entry_refuses_cpu_tensors():
    from moc_amd import engine
    with pytest.raises(AssertionError, match="no CPU fallback"):
        engine.adapter_logits(torch.zeros(4, 512), [torch.zeros(128, 512)], [torch.zeros(512, 128)], None, torch.zeros(512, 2), 0.1)


def test_fused_is_off_by_default():
    import moc_amd.model_adapters as A
    assert A.Conch_CLIP_Ada.fused is False and A.Conch_MOE_CLIP_Ada.fused is False
    assert A.Conch_CLIP_Ada(classifier_tensor=torch.zeros(512, 2)).fused is False
    assert callable(A.Conch_CLIP_Ada.forward_fused) and callable(A.Conch_MOE_CLIP_Ada.forward_fused)


@pytest.mark.parametrize("name", ["clip", "clip_short", "moe", "moe_switch", "moe_router"])
def test_fused_module_on_the_cpu_takes_the_torch_path(name):
    """No GPU tensor in sight: forward_fused must give what forward gives, output and gradients, bit for bit."""
    i = [c[0] for c in HB.BASELINE_CASES].index(name)
    _, kind, kw, N, label = HB.BASELINE_CASES[i]
    seed = 4000 + 17 * i
    runs = []
    for fused in (False, True):
        with BO.patched(), contextlib.redirect_stdout(io.StringIO()):
            import moc_amd.model_adapters as A
            cls, kwargs = HB.build_case(A, kind, kw, seed)
            model = cls(**kwargs)
            model.fused = fused
            runs.append(HB.run_case(model, kind, N, label, seed))
    assert runs[0].keys() == runs[1].keys()
    for k in runs[0]:
        assert (runs[0][k] == runs[1][k]).all(), k
    assert sorted(model.state_dict()) == sorted(cls(**kwargs).state_dict())
