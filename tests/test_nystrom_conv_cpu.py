"""The residual convolution's backward without a GPU: the two C entries are exported, declared and bound;
moc_nystrom_conv_backward_workspace is below one [n_pad, 512] fp32 tensor for the built shape and 0 for every other shape
or tap count; the entry refuses null and misaligned pointers, another shape, bad tap counts and a short workspace on the
host (made-up, never dereferenced device addresses: nothing is launched); `fused_conv` is off by default, reaches both
TransMIL layers, and on the CPU changes neither values nor gradients.  The two gradient formulas of DESIGN.md section 8c,
and the closed form that the GPU file's impulse test expects, are checked here against float64 autograd of F.conv2d."""
import copy
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

import helpers_baselines as HB

P = C.c_void_p
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "moc_nystrom_conv_backward_workspace": (C.c_size_t, [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int]),
    "moc_nystrom_conv_backward": (C.c_int, [P, C.c_int64, C.c_int, C.c_int, C.c_int, P, C.c_int, P, P, P, P, C.c_size_t, P]),
}
EINVAL, EUNSUPPORTED = 1, 2
NAME = "moc_nystrom_conv_backward"
POINTERS = ("qkv", "conv_w", "dout", "dqkv", "dconv_w", "ws")
WRAPPERS = ("nystrom_landmark_values", "nystrom_token_values", "nystrom_landmark_values_lse", "nystrom_landmark_backward",
            "nystrom_token_backward", "nystrom_conv_backward", "nystrom_pinv")


def test_the_two_entries_are_exported_declared_and_bound():
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


def test_workspace_is_below_one_gradient_tensor():
    from moc_amd import _lib
    h = _lib.lib()
    for bad in [(512, 4, 64, 256), (512, 8, 64, 128), (300, 8, 64, 256), (0, 8, 64, 256), (512, 8, 32, 256)]:
        assert h.moc_nystrom_conv_backward_workspace(*bad, 33) == 0, bad
    for taps in (0, 2, 35):
        assert h.moc_nystrom_conv_backward_workspace(512, 8, 64, 256, taps) == 0, taps
    for n_pad in (256, 512, 2304, 15360):
        for taps in (1, 3, 33):
            nbytes = h.moc_nystrom_conv_backward_workspace(n_pad, 8, 64, 256, taps)
            assert 0 < nbytes < n_pad * 512 * 4, (n_pad, taps, nbytes)


def _call(h, **over):
    a = dict(qkv=0x10000, n_pad=512, heads=8, dim_head=64, landmarks=256, conv_w=0x20000, taps=33, dout=0x30000, dqkv=0x40000,
             dconv_w=0x50000, ws=0x60000, ws_bytes=1 << 30)
    a.update(over)
    rc = h.moc_nystrom_conv_backward(a["qkv"], a["n_pad"], a["heads"], a["dim_head"], a["landmarks"], a["conv_w"], a["taps"],
                                     a["dout"], a["dqkv"], a["dconv_w"], a["ws"], a["ws_bytes"], None)
    return rc, h.moc_last_error().decode()


def test_the_entry_refuses_on_the_host():
    from moc_amd import _lib
    h = _lib.lib()
    for p in POINTERS:
        rc, msg = _call(h, **{p: None})
        assert rc == EINVAL and msg.startswith(NAME), (p, rc, msg)
        rc, msg = _call(h, **{p: 0x10004})
        assert rc == EINVAL and msg.startswith(NAME) and "aligned" in msg, (p, rc, msg)
    rc, msg = _call(h, **{p: None for p in POINTERS})
    assert rc == EINVAL and msg.startswith(NAME), (rc, msg)
    for over in (dict(heads=4), dict(dim_head=32), dict(landmarks=128)):
        rc, msg = _call(h, **over)
        assert rc == EUNSUPPORTED and msg.startswith(NAME), (over, rc, msg)
    for n_pad in (0, 255, 300, -256):
        rc, msg = _call(h, n_pad=n_pad)
        assert rc == EINVAL and msg.startswith(NAME) and "n_pad" in msg, (n_pad, rc, msg)
    for taps in (0, 2, -1):
        rc, msg = _call(h, taps=taps)
        assert rc == EINVAL and msg.startswith(NAME) and "taps" in msg, (taps, rc, msg)
    rc, msg = _call(h, taps=35)
    assert rc == EUNSUPPORTED and msg.startswith(NAME) and "taps" in msg, (rc, msg)
    for n_pad in (256, 512, 2304):
        need = h.moc_nystrom_conv_backward_workspace(n_pad, 8, 64, 256, 33)
        rc, msg = _call(h, n_pad=n_pad, ws_bytes=need - 1)
        assert rc == EINVAL and msg.startswith(NAME) and "ws_bytes" in msg, (n_pad, rc, msg)


def test_engine_entry_refuses_cpu_tensors():
    from moc_amd import engine
    with pytest.raises(AssertionError, match="no CPU fallback"):
        engine.nystrom_conv_backward(torch.zeros(256, 1536), torch.zeros(8, 33), torch.zeros(256, 512), torch.zeros(256, 1536))


def test_fused_conv_is_off_by_default_and_reaches_both_layers():
    from moc_amd.model_mil import TransMIL
    from moc_amd.nystrom import NystromAttention
    assert NystromAttention.fused_conv is False and NystromAttention(dim=512).fused_conv is False
    model = TransMIL(n_classes=2, size_arg="conch")
    assert model.fused_conv is False
    model.fused_conv = True
    assert model.layer1.attn.fused_conv is True and model.layer2.attn.fused_conv is True and model.fused_conv is True
    assert model.fused is False and model.fused_train is False                # a switch of its own
    model.layer1.attn.fused_conv = False
    assert model.fused_conv is False
    model.fused_conv = False
    assert model.layer2.attn.fused_conv is False
    assert sorted(model.state_dict()) == sorted(TransMIL(n_classes=2, size_arg="conch").state_dict())


def _grads(module, out):
    module.zero_grad()
    out.square().sum().backward()
    return {k: p.grad.clone() for k, p in module.named_parameters() if p.grad is not None}


def _no_kernels(monkeypatch):
    from moc_amd import engine

    def boom(*a, **k):
        raise AssertionError("a kernel wrapper was called on the CPU")
    for name in WRAPPERS:
        monkeypatch.setattr(engine, name, boom)


@pytest.mark.parametrize("n", [1, 257, 700])
def test_fused_conv_on_the_cpu_is_the_torch_path(n, monkeypatch):
    from moc_amd.nystrom import NystromAttention
    _no_kernels(monkeypatch)
    torch.manual_seed(290 + n)
    attn = NystromAttention(dim=512, dim_head=64, heads=8, num_landmarks=256, pinv_iterations=6, residual=True).eval()
    x = F.layer_norm(HB.randn(9500 + n, 1, n, 512), (512,))
    x1 = x.clone().requires_grad_(True)
    plain = attn(x1)
    want, want_x = _grads(attn, plain), x1.grad.clone()
    attn.fused = attn.fused_train = attn.fused_conv = True
    x2 = x.clone().requires_grad_(True)
    got = attn(x2)
    assert got.grad_fn is not None and torch.equal(got, plain)
    have = _grads(attn, got)
    assert torch.equal(x2.grad, want_x)
    assert sorted(have) == sorted(want) and "res_conv.weight" in have
    for k in want:
        assert torch.equal(have[k], want[k]), k
    with torch.no_grad():
        assert torch.equal(attn(x), plain.detach())


def test_fused_conv_transmil_on_the_cpu_is_the_torch_path(monkeypatch):
    from moc_amd.model_mil import TransMIL
    _no_kernels(monkeypatch)
    torch.manual_seed(79)
    model = TransMIL(n_classes=3, size_arg="conch").eval()
    twin = copy.deepcopy(model)
    twin.fused = twin.fused_train = twin.fused_conv = True
    data = HB.randn(9600, 300, 512)
    a, b = model(data)[0], twin(data)[0]
    assert torch.equal(a, b)
    want, have = _grads(model, a), _grads(twin, b)
    assert sorted(want) == sorted(have) and len(want) > 10
    for k in want:
        assert torch.equal(have[k], want[k]), k


# ---------------------------------------------------------------- the formulas the kernel implements
def _conv_autograd(v, w, dout):
    """float64 autograd of the layer's own convolution: v, dout [n, 8, 64], w [8, taps] -> (dv, dw)."""
    v, w = v.double().clone().requires_grad_(True), w.double().clone().requires_grad_(True)
    taps = w.shape[1]
    out = F.conv2d(v.permute(1, 0, 2).unsqueeze(0), w.reshape(8, 1, taps, 1), padding=(taps // 2, 0), groups=8)
    out.backward(dout.double().permute(1, 0, 2).unsqueeze(0))
    return v.grad, w.grad


@pytest.mark.parametrize("taps", [33, 3, 1])
def test_the_two_formulas_are_the_gradients_of_conv2d(taps):
    n = 80
    v, w, dout = HB.randn(9700 + taps, n, 8, 64), HB.randn(9710 + taps, 8, taps), HB.randn(9720 + taps, n, 8, 64)
    ref_dv, ref_dw = _conv_autograd(v, w, dout)
    half = taps // 2
    pad = lambda t: F.pad(t.double(), (0, 0, 0, 0, half, half))               # noqa: E731  (zero rows outside the sequence)
    vp, dp = pad(v), pad(dout)
    # dv[j] = sum_t w[t] dout[j - t + taps / 2];  dw[t] = sum_i sum_d dout[i] v[i + t - taps / 2]
    dv = sum(w[:, t].double()[None, :, None] * dp[2 * half - t:2 * half - t + n] for t in range(taps))
    dw = torch.stack([(dout.double() * vp[t:t + n]).sum(dim=(0, 2)) for t in range(taps)], dim=1)
    assert torch.allclose(dv, ref_dv, rtol=0, atol=1e-12) and torch.allclose(dw, ref_dw, rtol=0, atol=1e-10)


@pytest.mark.parametrize("r", [0, 15, 16, 40, 79])
def test_an_impulse_reads_the_taps_backwards(r):
    """dout = a at (r, h, d): dv[j, h, d] = a w[h, j - r + 16] for |j - r| <= 16 and dw[h, t] = a v[r + t - 16, h, d] --
    what tests/test_gpu_nystrom_conv.py asks of the kernel with `==`."""
    n, h, d, a = 80, 5, 37, 1.75
    v, w = HB.randn(9800, n, 8, 64), HB.randn(9801, 8, 33)
    dout = torch.zeros(n, 8, 64)
    dout[r, h, d] = a
    ref_dv, ref_dw = _conv_autograd(v, w, dout)
    want_dv, want_dw = torch.zeros(n, 8, 64, dtype=torch.float64), torch.zeros(8, 33, dtype=torch.float64)
    for j in range(max(0, r - 16), min(n, r + 17)):
        want_dv[j, h, d] = a * float(w[h, j - r + 16])
    for t in range(33):
        if 0 <= r + t - 16 < n:
            want_dw[h, t] = a * float(v[r + t - 16, h, d])
    assert torch.equal(want_dv, ref_dv) and torch.equal(want_dw, ref_dw)
