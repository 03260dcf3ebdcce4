"""TransMIL's PPEG on moc_ppeg.hip without a GPU: the three C entries are exported, declared and bound;
moc_ppeg_backward_workspace keeps its bounds (at most 2 MiB while H W < 1,024, below one [H W, 512] fp32 tensor from there
on, 0 for another dim); both entries refuse on the host (made-up, never dereferenced device addresses: nothing is
launched); the engine wrappers refuse CPU tensors; `PPEG.fused` / `TransMIL.fused_ppeg` are off by default, a switch of
their own, and change nothing on the CPU.  The formulas of include/moc_hip.h -- one merged 49-tap table, the same table
read backwards for dx, one table of sums G whose three windows are the weight gradients, one shared bias sum -- and the
closed form that the GPU file's impulse tests expect are checked against float64 autograd of PPEG itself."""
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
    "moc_ppeg_forward": (C.c_int, [P, C.c_int, C.c_int, C.c_int, P, P, P, P, P, P, P, P]),
    "moc_ppeg_backward_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "moc_ppeg_backward": (C.c_int, [P, C.c_int, C.c_int, C.c_int, P, P, P, P, P, P, P, P, P, P, P, P, C.c_size_t, P]),
}
EINVAL, EUNSUPPORTED = 1, 2
FWD_POINTERS = ("x", "w7", "b7", "w5", "b5", "w3", "b3", "out")
BWD_POINTERS = ("x", "w7", "w5", "w3", "dout", "dx", "dw7", "db7", "dw5", "db5", "dw3", "db3", "ws")
WRAPPERS = ("nystrom_landmark_values", "nystrom_token_values", "nystrom_landmark_values_lse", "nystrom_landmark_backward",
            "nystrom_token_backward", "nystrom_conv_backward", "nystrom_pinv", "nystrom_pinv_iterates", "nystrom_pinv_backward",
            "ppeg_forward", "ppeg_backward")
SWITCHES = ("fused", "fused_pinv", "fused_train", "fused_conv", "fused_pinv_train")


def test_the_three_entries_are_exported_declared_and_bound():
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


def test_workspace_bounds():
    from moc_amd import _lib
    h = _lib.lib()
    for H, W in [(1, 1), (7, 7), (31, 31), (32, 32), (123, 123), (5, 40)]:
        nbytes = h.moc_ppeg_backward_workspace(H, W, 512)
        assert nbytes > 0 and nbytes % 8 == 0, (H, W, nbytes)
        if H * W < 1024:
            assert nbytes <= 2 << 20, (H, W, nbytes)
        else:
            assert nbytes < H * W * 512 * 4, (H, W, nbytes)
        assert h.moc_ppeg_backward_workspace(H, W, 256) == 0
    for bad in [(0, 5), (5, 0), (-1, 3), (1 << 12, (1 << 10) + 1)]:
        assert h.moc_ppeg_backward_workspace(*bad, 512) == 0, bad
    assert h.moc_ppeg_backward_workspace(1 << 11, 1 << 11, 512) < (1 << 22) * 512 * 4    # the largest square there is
    assert 0 < h.moc_ppeg_backward_workspace(1, 1 << 22, 512) < (1 << 22) * 512 * 4      # and the thinnest


BIG = 1 << 36                                                                 # bytes between two made-up buffers


def _fwd(h, **over):
    a = dict(H=20, W=20, dim=512)
    a.update({p: (k + 1) * BIG for k, p in enumerate(FWD_POINTERS)})
    a.update(over)
    rc = h.moc_ppeg_forward(a["x"], a["H"], a["W"], a["dim"], a["w7"], a["b7"], a["w5"], a["b5"], a["w3"], a["b3"], a["out"], None)
    return rc, h.moc_last_error().decode()


def _bwd(h, **over):
    a = dict(H=20, W=20, dim=512, ws_bytes=1 << 34)
    a.update({p: (k + 1) * BIG for k, p in enumerate(BWD_POINTERS)})
    a.update(over)
    rc = h.moc_ppeg_backward(a["x"], a["H"], a["W"], a["dim"], a["w7"], a["w5"], a["w3"], a["dout"], a["dx"], a["dw7"], a["db7"],
                             a["dw5"], a["db5"], a["dw3"], a["db3"], a["ws"], a["ws_bytes"], None)
    return rc, h.moc_last_error().decode()


@pytest.mark.parametrize("which", ["forward", "backward"])
def test_the_entries_refuse_on_the_host(which):
    from moc_amd import _lib
    h = _lib.lib()
    call, pointers, name = (_fwd, FWD_POINTERS, "moc_ppeg_forward") if which == "forward" else (_bwd, BWD_POINTERS, "moc_ppeg_backward")
    for p in pointers:
        rc, msg = call(h, **{p: None})
        assert rc == EINVAL and msg.startswith(name), (p, rc, msg)
        rc, msg = call(h, **{p: BIG + 4})
        assert rc == EINVAL and msg.startswith(name) and "aligned" in msg, (p, rc, msg)
    rc, msg = call(h, **{p: None for p in pointers})
    assert rc == EINVAL and msg.startswith(name), (rc, msg)
    for dim in (256, 1024, 0):
        rc, msg = call(h, dim=dim)
        assert rc == EUNSUPPORTED and msg.startswith(name) and "dim" in msg, (dim, rc, msg)
    for over in (dict(H=0), dict(W=0), dict(H=-3), dict(W=-1), dict(H=1 << 12, W=(1 << 10) + 1), dict(H=1 << 16, W=1 << 16)):
        rc, msg = call(h, **over)
        assert rc == EINVAL and msg.startswith(name) and "H=" in msg, (over, rc, msg)
    nbytes = (1 + 20 * 20) * 512 * 4                                          # of x, out, dout, dx at 20 x 20
    if which == "forward":
        for out in (BIG, BIG + 16, BIG + nbytes - 16, BIG - nbytes + 16):
            rc, msg = _fwd(h, x=BIG, out=out)
            assert rc == EINVAL and msg.startswith(name) and "overlaps" in msg, (out, rc, msg)
    else:
        for other in ("dout", "x"):
            for dx in (BIG, BIG + 16, BIG + nbytes - 16, BIG - nbytes + 16):
                rc, msg = _bwd(h, **{other: BIG, "dx": dx})
                assert rc == EINVAL and msg.startswith(name) and "overlaps" in msg, (other, dx, rc, msg)
        for H, W in [(1, 1), (20, 20), (33, 33)]:
            need = h.moc_ppeg_backward_workspace(H, W, 512)
            rc, msg = _bwd(h, H=H, W=W, ws_bytes=need - 1)
            assert rc == EINVAL and msg.startswith(name) and "ws_bytes" in msg, (H, W, rc, msg)


def _module(seed=31, dim=512):
    from moc_amd.model_mil import PPEG
    torch.manual_seed(seed)
    return PPEG(dim).eval()


def _params(m):
    return (m.proj.weight, m.proj.bias, m.proj1.weight, m.proj1.bias, m.proj2.weight, m.proj2.bias)


def test_engine_entries_refuse_cpu_tensors():
    from moc_amd import engine
    m = _module()
    w7, b7, w5, b5, w3, b3 = _params(m)
    x = torch.zeros(1, 10, 512)
    with pytest.raises(AssertionError, match="no CPU fallback"):
        engine.ppeg_forward(x, 3, 3, w7, b7, w5, b5, w3, b3)
    with pytest.raises(AssertionError, match="no CPU fallback"):
        engine.ppeg_backward(x, 3, 3, w7, w5, w3, torch.zeros_like(x))


def test_the_switch_is_off_by_default_and_of_its_own():
    from moc_amd.model_mil import PPEG, TransMIL
    assert PPEG.fused is False and PPEG(512).fused is False
    model = TransMIL(n_classes=2, size_arg="conch")
    assert model.fused_ppeg is False
    model.fused_ppeg = True
    assert model.pos_layer.fused is True and model.fused_ppeg is True
    assert not any(getattr(model, s) for s in SWITCHES)                       # it changes none of the attention switches
    for s in SWITCHES:
        setattr(model, s, True)
    model.fused_ppeg = False
    assert model.pos_layer.fused is False and all(getattr(model, s) for s in SWITCHES)
    for s in SWITCHES:
        setattr(model, s, False)
    assert model.fused_ppeg is False
    model.pos_layer.fused = True
    assert model.fused_ppeg is True
    assert sorted(model.state_dict()) == sorted(TransMIL(n_classes=2, size_arg="conch").state_dict())
    assert PPEG.fused is False                                                # the class attribute is left alone


def _grads(module, out):
    module.zero_grad()
    out.square().sum().backward()
    return {k: p.grad.clone() for k, p in module.named_parameters() if p.grad is not None}


def test_fused_ppeg_transmil_on_the_cpu_is_the_torch_path(monkeypatch):
    from moc_amd import engine
    from moc_amd.model_mil import TransMIL

    def boom(*a, **k):
        raise AssertionError("a kernel wrapper was called on the CPU")
    for name in WRAPPERS:
        monkeypatch.setattr(engine, name, boom)
    torch.manual_seed(83)
    model = TransMIL(n_classes=3, size_arg="conch").eval()
    twin = copy.deepcopy(model)
    twin.fused_ppeg = True
    data = HB.randn(9900, 300, 512)
    a, b = model(data)[0], twin(data)[0]
    assert torch.equal(a, b)
    want, have = _grads(model, a), _grads(twin, b)
    assert sorted(want) == sorted(have) and "pos_layer.proj1.weight" in want
    for k in want:
        assert torch.equal(have[k], want[k]), k
    with torch.no_grad():
        assert torch.equal(twin(data)[0], a.detach())


# ---------------------------------------------------------------- the formulas the kernels implement
def ppeg_autograd(m, x, H, W, dout):
    """(out, dx, {parameter name: gradient}) of PPEG `m` itself, in its parameters' precision."""
    m.zero_grad(set_to_none=True)
    x = x.detach().clone().requires_grad_(True)
    out = m(x, H, W)
    out.backward(dout)
    return out.detach(), x.grad, {k: p.grad.clone() for k, p in m.named_parameters()}


def merged_table(w7, w5, w3):
    """[C, 7, 7]: w7 + pad(w5) + pad(w3)."""
    return w7[:, 0] + F.pad(w5[:, 0], (1, 1, 1, 1)) + F.pad(w3[:, 0], (2, 2, 2, 2))


def ppeg_formulas(x, H, W, w7, b7, w5, b5, w3, b3, dout):
    """The header's formulas, tap by tap: (out, dx, G [C, 7, 7], bias sum [C]) from x, dout [1, 1 + H W, C]."""
    Cn = x.shape[2]
    w = merged_table(w7, w5, w3)
    sq = lambda t: F.pad(t[0, 1:].reshape(H, W, Cn), (0, 0, 3, 3, 3, 3))      # noqa: E731  (zeros outside the square)
    xs, ds = sq(x), sq(dout)
    conv, back, G = torch.zeros(H, W, Cn, dtype=x.dtype), torch.zeros(H, W, Cn, dtype=x.dtype), torch.zeros_like(w)
    for i in range(7):                                                        # (dy, dx) = (i - 3, j - 3)
        for j in range(7):
            conv += w[:, i, j] * xs[i:i + H, j:j + W]                         # x[p + d]
            back += w[:, i, j] * ds[6 - i:6 - i + H, 6 - j:6 - j + W]         # dout[p - d]: the table read backwards
            G[:, i, j] = (ds[3:3 + H, 3:3 + W] * xs[i:i + H, j:j + W]).sum(dim=(0, 1))
    out, dx = x.clone(), dout.clone()
    out[0, 1:] += (b7 + b5 + b3) + conv.reshape(H * W, Cn)
    dx[0, 1:] += back.reshape(H * W, Cn)
    return out, dx, G, dout[0, 1:].sum(dim=0)


@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (3, 3), (7, 7), (17, 17), (5, 9), (9, 5)])
def test_the_formulas_are_ppeg_and_its_gradients(H, W):
    dim = 16
    m = _module(40 + H, dim).double()
    x, dout = HB.randn(9910 + H * W, 1, 1 + H * W, dim).double(), HB.randn(9920 + H * W, 1, 1 + H * W, dim).double()
    ref_out, ref_dx, ref = ppeg_autograd(m, x, H, W, dout)
    out, dx, G, db = ppeg_formulas(x, H, W, *[p.detach() for p in _params(m)], dout)
    assert torch.allclose(out, ref_out, rtol=0, atol=1e-11) and torch.allclose(dx, ref_dx, rtol=0, atol=1e-11)
    assert torch.equal(out[0, 0], x[0, 0]) and torch.equal(dx[0, 0], dout[0, 0])
    assert torch.allclose(G, ref["proj.weight"][:, 0], rtol=0, atol=1e-9)
    assert torch.allclose(G[:, 1:6, 1:6], ref["proj1.weight"][:, 0], rtol=0, atol=1e-9)
    assert torch.allclose(G[:, 2:5, 2:5], ref["proj2.weight"][:, 0], rtol=0, atol=1e-9)
    for k in ("proj.bias", "proj1.bias", "proj2.bias"):
        assert torch.allclose(db, ref[k], rtol=0, atol=1e-9), k


def grid(t, step=2.0 ** -10):
    """t rounded to multiples of `step`: sums of a few products of such numbers are exact in fp32 and in any order."""
    return torch.round(t / step) * step


def impulse_backward(x, H, W, w, py, px, c, a):
    """What dout = a at (position p = (py, px), channel c) gives: dx[q] = a (w[c, q - p] + [q = p]) inside the window (dx[q] =
    sum_d w[d] dout[q - d] with dout nonzero at q - d = p only), G[c, d] = a x[p + d, c], db[c] = a, zeros elsewhere.
    x [1, 1 + H W, C], w the merged table [C, 7, 7]."""
    dx, G, db = torch.zeros_like(x), torch.zeros_like(w), torch.zeros(w.shape[0], dtype=w.dtype)
    for i in range(7):
        for j in range(7):
            qy, qx = py + (i - 3), px + (j - 3)                               # q - p = d = (i - 3, j - 3)
            if 0 <= qy < H and 0 <= qx < W:
                dx[0, 1 + qy * W + qx, c] = a * w[c, i, j]
            sy, sx = py + (i - 3), px + (j - 3)
            if 0 <= sy < H and 0 <= sx < W:
                G[c, i, j] = a * x[0, 1 + sy * W + sx, c]
    dx[0, 1 + py * W + px, c] += a
    db[c] = a
    return dx, G, db


def impulse_forward(H, W, w, bias, py, px, c, a, dtype):
    """What x = a at (position (py, px), channel c) and zero elsewhere gives: out[q] = bias + a (w[c, p - q] + [q = p])."""
    out = torch.zeros(1, 1 + H * W, w.shape[0], dtype=dtype)
    out[0, 1:] = bias
    for i in range(7):
        for j in range(7):
            qy, qx = py - (i - 3), px - (j - 3)                               # out[q] reads x[q + d]: q + d = p
            if 0 <= qy < H and 0 <= qx < W:
                out[0, 1 + qy * W + qx, c] += a * w[c, i, j]
    out[0, 1 + py * W + px, c] += a
    return out


IMPULSES = [(0, 0), (0, 19), (19, 0), (19, 19), (0, 3), (3, 0), (3, 3), (16, 16), (19, 10)]


@pytest.mark.parametrize("py,px", IMPULSES)
def test_the_impulse_closed_forms(py, px):
    H = W = 20
    dim, c, a = 8, (3 * py + px) % 8, -0.5 if (py + px) % 2 else 2.0
    m = _module(77, dim).double()
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(grid(p))
    w7, b7, w5, b5, w3, b3 = [p.detach() for p in _params(m)]
    w = merged_table(w7, w5, w3)
    x = grid(HB.randn(9930, 1, 1 + H * W, dim)).double()
    dout = torch.zeros_like(x)
    dout[0, 1 + py * W + px, c] = a
    _, ref_dx, ref = ppeg_autograd(m, x, H, W, dout)
    dx, G, db = impulse_backward(x, H, W, w, py, px, c, a)
    assert torch.equal(dx, ref_dx) and torch.equal(G, ref["proj.weight"][:, 0]) and torch.equal(db, ref["proj.bias"])
    assert torch.equal(G[:, 1:6, 1:6], ref["proj1.weight"][:, 0]) and torch.equal(G[:, 2:5, 2:5], ref["proj2.weight"][:, 0])
    xi = torch.zeros_like(x)
    xi[0, 1 + py * W + px, c] = a
    ref_out, _, _ = ppeg_autograd(m, xi, H, W, dout)
    assert torch.equal(impulse_forward(H, W, w, b7 + b5 + b3, py, px, c, a, torch.float64), ref_out)
