"""The Nystrom backward without a GPU: the four C entries are exported, declared and bound; moc_nystrom_backward_workspace
sizes the built shape below one [8, n_pad, 256] fp32 score matrix and returns 0 for every other shape; each new entry
refuses null pointers and another shape on the host (made-up, never dereferenced device addresses: nothing is launched);
`fused_train` is off by default, reaches both TransMIL layers, and on the CPU changes neither values nor gradients."""
import copy
import ctypes as C
import os
import re

import pytest
import torch

import helpers_baselines as HB

P = C.c_void_p
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "moc_nystrom_backward_workspace": (C.c_size_t, [C.c_int64, C.c_int, C.c_int, C.c_int]),
    "moc_nystrom_landmark_values_lse": (C.c_int, [P, C.c_int64, C.c_int, C.c_int, C.c_int, P, P, P, P, C.c_size_t, P]),
    "moc_nystrom_landmark_backward": (C.c_int, [P, C.c_int64, C.c_int, C.c_int, C.c_int, P, P, P, P, P, P, P, C.c_size_t, P]),
    "moc_nystrom_token_backward": (C.c_int, [P, C.c_int64, C.c_int, C.c_int, C.c_int, P, P, C.c_float, P, P, P, P, P,
                                             C.c_size_t, P]),
}
EINVAL, EUNSUPPORTED = 1, 2


def test_the_four_entries_are_exported_declared_and_bound():
    from moc_amd import _lib
    h = _lib.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "moc_hip.h")).read(), flags=re.S)
    for name, (res, args) in NEW.items():
        assert hasattr(h, name), name
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in moc_hip.h"
        assert _lib.SIGNATURES[name] == (res, args), name
        fn = getattr(h, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert h.moc_version() == 20 and _lib.ABI_VERSION == 20


def test_backward_workspace_is_below_one_score_matrix():
    from moc_amd import _lib
    h = _lib.lib()
    for bad in [(512, 4, 64, 256), (512, 8, 64, 128), (300, 8, 64, 256), (0, 8, 64, 256), (512, 8, 32, 256)]:
        assert h.moc_nystrom_backward_workspace(*bad) == 0, bad
    for n_pad in (256, 512, 768, 2304, 15360):
        nbytes = h.moc_nystrom_backward_workspace(n_pad, 8, 64, 256)
        assert 0 < nbytes < 8 * n_pad * 256 * 4, (n_pad, nbytes)


def _lse(h, **over):
    a = dict(qkv=0x10000, n_pad=512, heads=8, dim_head=64, landmarks=256, q_l=0x20000, W=0x30000, lse=0x40000, ws=0x50000,
             ws_bytes=1 << 30)
    a.update(over)
    rc = h.moc_nystrom_landmark_values_lse(a["qkv"], a["n_pad"], a["heads"], a["dim_head"], a["landmarks"], a["q_l"], a["W"],
                                           a["lse"], a["ws"], a["ws_bytes"], None)
    return rc, h.moc_last_error().decode()


def _lbwd(h, **over):
    a = dict(qkv=0x10000, n_pad=512, heads=8, dim_head=64, landmarks=256, q_l=0x20000, W=0x30000, lse=0x40000, dW=0x50000,
             dqkv=0x60000, dq_l=0x70000, ws=0x80000, ws_bytes=1 << 30)
    a.update(over)
    rc = h.moc_nystrom_landmark_backward(a["qkv"], a["n_pad"], a["heads"], a["dim_head"], a["landmarks"], a["q_l"], a["W"],
                                         a["lse"], a["dW"], a["dqkv"], a["dq_l"], a["ws"], a["ws_bytes"], None)
    return rc, h.moc_last_error().decode()


def _tbwd(h, **over):
    a = dict(qkv=0x10000, n_pad=512, heads=8, dim_head=64, landmarks=256, k_l=0x20000, Y=0x30000, scale=0.125, dout=0x40000,
             dqkv=0x50000, dk_l=0x60000, dY=0x70000, ws=0x80000, ws_bytes=1 << 30)
    a.update(over)
    rc = h.moc_nystrom_token_backward(a["qkv"], a["n_pad"], a["heads"], a["dim_head"], a["landmarks"], a["k_l"], a["Y"],
                                      C.c_float(a["scale"]), a["dout"], a["dqkv"], a["dk_l"], a["dY"], a["ws"], a["ws_bytes"],
                                      None)
    return rc, h.moc_last_error().decode()


ENTRIES = [("moc_nystrom_landmark_values_lse", _lse, ("qkv", "q_l", "W", "lse", "ws")),
           ("moc_nystrom_landmark_backward", _lbwd, ("qkv", "q_l", "W", "lse", "dW", "dqkv", "dq_l", "ws")),
           ("moc_nystrom_token_backward", _tbwd, ("qkv", "k_l", "Y", "dout", "dqkv", "dk_l", "dY", "ws"))]


@pytest.mark.parametrize("name,call,pointers", ENTRIES)
def test_each_entry_refuses_on_the_host(name, call, pointers):
    from moc_amd import _lib
    h = _lib.lib()
    for p in pointers:
        rc, msg = call(h, **{p: None})
        assert rc == EINVAL and msg.startswith(name), (p, rc, msg)
        rc, msg = call(h, **{p: 0x10004})
        assert rc == EINVAL and msg.startswith(name) and "aligned" in msg, (p, rc, msg)
    rc, msg = call(h, **{p: None for p in pointers})
    assert rc == EINVAL and msg.startswith(name), (rc, msg)
    for over in (dict(heads=4), dict(dim_head=32), dict(landmarks=128)):
        rc, msg = call(h, **over)
        assert rc == EUNSUPPORTED and msg.startswith(name), (over, rc, msg)
    for n_pad in (0, 255, 300, -256):
        rc, msg = call(h, n_pad=n_pad)
        assert rc == EINVAL and msg.startswith(name) and "n_pad" in msg, (n_pad, rc, msg)
    rc, msg = call(h, ws_bytes=1024)
    assert rc == EINVAL and msg.startswith(name) and "ws_bytes" in msg, (rc, msg)


def test_backward_entries_want_the_documented_workspace_and_a_finite_scale():
    from moc_amd import _lib
    h = _lib.lib()
    need = h.moc_nystrom_backward_workspace(512, 8, 64, 256)
    for call in (_lbwd, _tbwd):
        rc, msg = call(h, ws_bytes=need - 1)
        assert rc == EINVAL and "ws_bytes" in msg, (rc, msg)
    for bad in (float("nan"), float("inf")):
        rc, msg = _tbwd(h, scale=bad)
        assert rc == EINVAL and msg.startswith("moc_nystrom_token_backward") and "scale" in msg, (rc, msg)


def test_engine_entries_refuse_cpu_tensors():
    from moc_amd import engine
    hmd, qkv = torch.zeros(8, 256, 64), torch.zeros(256, 1536)
    with pytest.raises(AssertionError, match="no CPU fallback"):
        engine.nystrom_landmark_values_lse(qkv, hmd)
    with pytest.raises(AssertionError, match="no CPU fallback"):
        engine.nystrom_landmark_backward(qkv, hmd, hmd, torch.zeros(8, 256), hmd)
    with pytest.raises(AssertionError, match="no CPU fallback"):
        engine.nystrom_token_backward(qkv, hmd, hmd, 0.125, torch.zeros(256, 512))


def test_fused_train_is_off_by_default_and_reaches_both_layers():
    from moc_amd.model_mil import TransMIL
    from moc_amd.nystrom import NystromAttention
    assert NystromAttention.fused_train is False and NystromAttention(dim=512).fused_train is False
    model = TransMIL(n_classes=2, size_arg="conch")
    assert model.fused_train is False
    model.fused_train = True
    assert model.layer1.attn.fused_train is True and model.layer2.attn.fused_train is True and model.fused_train is True
    assert model.fused is False                                               # a switch of its own
    model.layer1.attn.fused_train = False
    assert model.fused_train is False
    model.fused_train = False
    assert model.layer2.attn.fused_train is False
    assert sorted(model.state_dict()) == sorted(TransMIL(n_classes=2, size_arg="conch").state_dict())


def _grads(module, out):
    module.zero_grad()
    out.square().sum().backward()
    return {k: p.grad.clone() for k, p in module.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("n", [1, 257, 700])
def test_fused_train_on_the_cpu_is_the_torch_path(n, monkeypatch):
    from moc_amd import engine
    from moc_amd.nystrom import NystromAttention

    def boom(*a, **k):
        raise AssertionError("a kernel wrapper was called on the CPU")
    for name in ("nystrom_landmark_values", "nystrom_token_values", "nystrom_landmark_values_lse", "nystrom_landmark_backward",
                 "nystrom_token_backward"):
        monkeypatch.setattr(engine, name, boom)
    torch.manual_seed(190 + n)
    attn = NystromAttention(dim=512, dim_head=64, heads=8, num_landmarks=256, pinv_iterations=6, residual=True).eval()
    x = torch.nn.functional.layer_norm(HB.randn(9300 + n, 1, n, 512), (512,))
    x1 = x.clone().requires_grad_(True)
    plain = attn(x1)
    want, want_x = _grads(attn, plain), x1.grad.clone()
    attn.fused = attn.fused_train = True
    x2 = x.clone().requires_grad_(True)
    got = attn(x2)
    assert got.grad_fn is not None and torch.equal(got, plain)
    have = _grads(attn, got)
    assert torch.equal(x2.grad, want_x)
    for k in want:
        assert torch.equal(have[k], want[k]), k
    with torch.no_grad():
        assert torch.equal(attn(x), plain.detach())


def test_fused_train_transmil_on_the_cpu_is_the_torch_path():
    from moc_amd.model_mil import TransMIL
    torch.manual_seed(78)
    model = TransMIL(n_classes=3, size_arg="conch").eval()
    twin = copy.deepcopy(model)
    twin.fused = twin.fused_train = True
    data = HB.randn(9400, 300, 512)
    a, b = model(data)[0], twin(data)[0]
    assert torch.equal(a, b)
    want, have = _grads(model, a), _grads(twin, b)
    assert sorted(want) == sorted(have) and len(want) > 10
    for k in want:
        assert torch.equal(have[k], want[k]), k
