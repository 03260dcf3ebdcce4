"""The gradient through the landmark pseudo-inverse (moc_nystrom_pinv_iterates, moc_nystrom_pinv_backward;
nystrom.LandmarkPinv; NystromAttention.fused_pinv_train) without a GPU: the formulas the kernels implement, restated in torch
below and checked against float64 autograd of moore_penrose_iter_pinv (even split among tied maxima included); the three C
entries exported and bound with the documented signatures at ABI 20; the workspace; every contract violation refused on the
host (made-up, never dereferenced device addresses: nothing is launched); the engine entries refusing CPU tensors; and the
switch off by default, reaching both layers, and changing nothing on the CPU."""
import ctypes as C

import pytest
import torch

import helpers_baselines as HB

P = C.c_void_p
MAT = 8 * 256 * 256 * 4                                               # bytes of one [8, 256, 256] fp32 matrix
EINVAL, EUNSUPPORTED = 1, 2


# ---------------------------------------------------------------- the formulas
def pinv_iterates(X, iters):
    """[Z_0 .. Z_iters] and den of moore_penrose_iter_pinv for X [h, m, m]."""
    eye = torch.eye(X.shape[-1], dtype=X.dtype)
    col, row = X.abs().sum(dim=-1), X.abs().sum(dim=-2)
    den = col.max() * row.max()
    Zs = [X.transpose(-1, -2) / den]
    for _ in range(iters):
        Z = Zs[-1]
        XZ = X @ Z
        P2 = XZ @ (7 * eye - XZ)
        P3 = XZ @ (15 * eye - P2)
        Zs.append(0.25 * Z @ (13 * eye - P3))
    return Zs


def pinv_backward(X, Zs, dZ):
    """dX from the iterates and dZ = d(Z_iters): the chain of products, then the init with ties sharing evenly."""
    T = lambda a: a.transpose(-1, -2)                                 # noqa: E731
    eye = torch.eye(X.shape[-1], dtype=X.dtype)
    dX = torch.zeros_like(X)
    for t in range(len(Zs) - 2, -1, -1):
        Z = Zs[t]
        XZ = X @ Z
        P2 = XZ @ (7 * eye - XZ)
        P3 = XZ @ (15 * eye - P2)
        dZa = 0.25 * dZ @ T(13 * eye - P3)
        dP3 = -0.25 * T(Z) @ dZ
        dP2 = -(T(XZ) @ dP3)
        dXZ = dP3 @ T(15 * eye - P2) + dP2 @ T(7 * eye - XZ) - T(XZ) @ dP2
        dX = dX + dXZ @ T(Z)
        dZ = dZa + T(X) @ dXZ
    col, row = X.abs().sum(dim=-1), X.abs().sum(dim=-2)               # [h, m] over j, [h, m] over i
    c, r = col.max(), row.max()
    den = c * r
    dX = dX + T(dZ) / den
    dden = -(dZ * Zs[0]).sum() / den
    dc, dr = dden * r, dden * c
    tie_c, tie_r = (col == c), (row == r)
    dX = dX + (dc / tie_c.sum()) * tie_c.to(X.dtype).unsqueeze(-1) * X.sign()
    dX = dX + (dr / tie_r.sum()) * tie_r.to(X.dtype).unsqueeze(-2) * X.sign()
    return dX


def _inputs(kind):
    h, m = 3, 32                                                      # the formulas hold for any shape
    g = torch.Generator().manual_seed({"softmax": 1, "signed": 2, "ties": 3}[kind])
    X = torch.randn(h, m, m, generator=g, dtype=torch.float64)
    if kind == "signed":
        return X / 16 + torch.eye(m, dtype=torch.float64)
    X = X.softmax(dim=-1)
    if kind == "ties":
        i = int(X.abs().sum(dim=-2)[1].argmax())
        j = (i + 7) % m
        X[1, :, j] = X[1, :, i]                                       # the maximal column of head 1, duplicated
        X[1, :, [i, j]] *= 1.5                                        # and made the maximum over all heads
        X[0, 5] *= 2.0                                                # the one maximal row ...
        X[2, 9] = X[0, 5]                                             # ... and its copy in another head
        col, row = X.abs().sum(dim=-1), X.abs().sum(dim=-2)
        assert int((col == col.max()).sum()) == 2 and int((row == row.max()).sum()) == 2
    return X


@pytest.mark.parametrize("kind", ["softmax", "signed", "ties"])
@pytest.mark.parametrize("iters", [0, 1, 2, 6])
def test_the_formulas_are_float64_autograd_of_the_torch_function(kind, iters):
    from moc_amd.nystrom import moore_penrose_iter_pinv
    X = _inputs(kind)
    dZ = torch.randn(X.shape, generator=torch.Generator().manual_seed(10 + iters), dtype=torch.float64)
    leaf = X.clone().requires_grad_(True)
    Z = moore_penrose_iter_pinv(leaf, iters)
    Z.backward(dZ)
    Zs = pinv_iterates(X, iters)
    assert torch.allclose(Zs[-1], Z.detach(), rtol=1e-12, atol=0)
    got, ref = pinv_backward(X, Zs, dZ), leaf.grad
    top = float(ref.abs().max())
    err = float((got - ref).abs().max())
    print(f"pinv backward formulas {kind} iters={iters}: max|ref| {top:.3e}  error {err:.3e}")
    assert err <= 1e-11 * max(1.0, top)                               # float64 against float64: summation order only


# ---------------------------------------------------------------- bindings, workspace, refusals
def test_library_exports_the_entries_with_the_documented_signatures():
    from moc_amd import _lib
    h = _lib.lib()
    assert h.moc_version() == 20 and _lib.ABI_VERSION == 20
    want = {
        "moc_nystrom_pinv_iterates": (C.c_int, [P, C.c_int, C.c_int, C.c_int, P, P, C.c_size_t, P]),
        "moc_nystrom_pinv_backward_workspace": (C.c_size_t, [C.c_int, C.c_int]),
        "moc_nystrom_pinv_backward": (C.c_int, [P, C.c_int, C.c_int, C.c_int, P, P, P, P, C.c_size_t, P]),
    }
    for name, (res, args) in want.items():
        assert hasattr(h, name), name
        assert _lib.SIGNATURES[name] == (res, args), name
        fn = getattr(h, name)
        assert fn.restype is res and list(fn.argtypes) == args
    import os
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "moc_hip.h")).read()
    for name in want:
        assert name + "(" in header, name


def test_workspace_is_sized_for_the_built_shape_and_zero_elsewhere():
    from moc_amd import _lib
    h = _lib.lib()
    n = h.moc_nystrom_pinv_backward_workspace(8, 256)
    assert n >= 8 * MAT and n % 16 == 0                               # XZ, P2, P3, dP3, dP2, dXZ and a ping-pong dZ at the least
    for bad in [(4, 256), (8, 128), (8, 0), (16, 256), (8, 512), (0, 256), (-8, 256), (8, -256)]:
        assert h.moc_nystrom_pinv_backward_workspace(*bad) == 0, bad


def _iterates(lib_, **over):
    a = dict(A=0x1000000, heads=8, landmarks=256, iters=6, Zs=0x10000000, ws=0x40000000, ws_bytes=1 << 30)
    a.update(over)
    rc = lib_.moc_nystrom_pinv_iterates(a["A"], a["heads"], a["landmarks"], a["iters"], a["Zs"], a["ws"], a["ws_bytes"], None)
    return rc, lib_.moc_last_error().decode()


def _backward(lib_, **over):
    a = dict(A=0x1000000, heads=8, landmarks=256, iters=6, Zs=0x10000000, dZ=0x2000000, dA=0x3000000, ws=0x40000000,
             ws_bytes=1 << 30)
    a.update(over)
    rc = lib_.moc_nystrom_pinv_backward(a["A"], a["heads"], a["landmarks"], a["iters"], a["Zs"], a["dZ"], a["dA"], a["ws"],
                                        a["ws_bytes"], None)
    return rc, lib_.moc_last_error().decode()


@pytest.mark.parametrize("over,code,word", [
    (dict(heads=4), EUNSUPPORTED, "heads=4"), (dict(landmarks=128), EUNSUPPORTED, "landmarks=128"),
    (dict(heads=0), EUNSUPPORTED, "heads=0"), (dict(landmarks=512), EUNSUPPORTED, "landmarks=512"),
    (dict(A=None), EINVAL, "A is null"), (dict(Zs=None), EINVAL, "Zs is null"), (dict(ws=None), EINVAL, "ws is null"),
    (dict(A=0x1000004), EINVAL, "aligned"), (dict(Zs=0x10000008), EINVAL, "aligned"), (dict(ws=0x40000001), EINVAL, "aligned"),
    (dict(Zs=0x1000000), EINVAL, "overlap"), (dict(A=0x10000000 + 7 * MAT - 16), EINVAL, "overlap"),
    (dict(ws=0x10000000 + 6 * MAT), EINVAL, "overlap"), (dict(ws=0x1000000 + MAT - 16), EINVAL, "overlap"),
    (dict(ws_bytes=0), EINVAL, "ws_bytes=0"), (dict(ws_bytes=5 * MAT), EINVAL, "ws_bytes"),
    (dict(iters=-1), EINVAL, "iters=-1"), (dict(iters=65), EINVAL, "iters=65"),
])
def test_iterates_refuses_on_the_host(over, code, word):
    from moc_amd import _lib
    rc, msg = _iterates(_lib.lib(), **over)
    assert rc == code and msg.startswith("moc_nystrom_pinv_iterates") and word in msg, (rc, msg)


def test_iterates_sizes_zs_by_the_iteration_count():
    """A buffer right behind Zs is clear of it at 2 iterations (three matrices) and inside it at 6."""
    from moc_amd import _lib
    rc, msg = _iterates(_lib.lib(), A=0x10000000 + 3 * MAT, iters=6)
    assert rc == EINVAL and "overlap" in msg
    rc, msg = _iterates(_lib.lib(), A=0x10000000 + 3 * MAT, iters=2, ws_bytes=0)       # past the overlap check's place
    assert rc == EINVAL and "ws_bytes=0" in msg


@pytest.mark.parametrize("over,code,word", [
    (dict(heads=4), EUNSUPPORTED, "heads=4"), (dict(heads=16), EUNSUPPORTED, "heads=16"),
    (dict(landmarks=128), EUNSUPPORTED, "landmarks=128"), (dict(landmarks=0), EUNSUPPORTED, "landmarks=0"),
    (dict(A=None), EINVAL, "A is null"), (dict(Zs=None), EINVAL, "Zs is null"), (dict(dZ=None), EINVAL, "dZ is null"),
    (dict(dA=None), EINVAL, "dA is null"), (dict(ws=None), EINVAL, "ws is null"),
    (dict(A=0x1000004), EINVAL, "aligned"), (dict(Zs=0x10000008), EINVAL, "aligned"), (dict(dZ=0x2000002), EINVAL, "aligned"),
    (dict(dA=0x3000004), EINVAL, "aligned"), (dict(ws=0x40000001), EINVAL, "aligned"),
    (dict(dA=0x1000000), EINVAL, "A and dA overlap"), (dict(dA=0x2000000 + MAT - 16), EINVAL, "dZ and dA overlap"),
    (dict(dA=0x10000000 + 6 * MAT), EINVAL, "Zs and dA overlap"), (dict(dZ=0x1000000 + 16), EINVAL, "A and dZ overlap"),
    (dict(A=0x10000000 + 16), EINVAL, "A and Zs overlap"), (dict(dZ=0x10000000 + 7 * MAT - 16), EINVAL, "Zs and dZ overlap"),
    (dict(ws=0x3000000 + MAT - 16), EINVAL, "dA and ws overlap"), (dict(ws=0x1000000), EINVAL, "A and ws overlap"),
    (dict(ws=0x10000000 + MAT), EINVAL, "Zs and ws overlap"), (dict(ws=0x2000000), EINVAL, "dZ and ws overlap"),
    (dict(ws_bytes=0), EINVAL, "ws_bytes=0"), (dict(ws_bytes=8 * MAT), EINVAL, "ws_bytes"),
    (dict(iters=-1), EINVAL, "iters=-1"), (dict(iters=65), EINVAL, "iters=65"),
])
def test_backward_refuses_on_the_host(over, code, word):
    from moc_amd import _lib
    rc, msg = _backward(_lib.lib(), **over)
    assert rc == code and msg.startswith("moc_nystrom_pinv_backward") and word in msg, (rc, msg)


def test_a_workspace_one_byte_short_is_refused_with_both_sizes_named():
    from moc_amd import _lib
    h = _lib.lib()
    need = h.moc_nystrom_pinv_backward_workspace(8, 256)
    rc, msg = _backward(h, ws_bytes=need - 1)
    assert rc == EINVAL and msg.startswith("moc_nystrom_pinv_backward") and f"ws_bytes={need - 1}" in msg and str(need) in msg
    need = h.moc_nystrom_pinv_workspace(8, 256)
    rc, msg = _iterates(h, ws_bytes=need - 1)
    assert rc == EINVAL and msg.startswith("moc_nystrom_pinv_iterates") and f"ws_bytes={need - 1}" in msg and str(need) in msg


def test_engine_entries_refuse_cpu_tensors():
    from moc_amd import engine
    a = torch.zeros(8, 256, 256)
    with pytest.raises(AssertionError, match="no CPU fallback"):
        engine.nystrom_pinv_iterates(a, 6)
    with pytest.raises(AssertionError, match="no CPU fallback"):
        engine.nystrom_pinv_iterates(torch.zeros(8, 128, 128), 6)
    with pytest.raises(AssertionError, match="no CPU fallback"):
        engine.nystrom_pinv_backward(a, torch.zeros(7, 8, 256, 256), a, 6)


# ---------------------------------------------------------------- the switch
def test_fused_pinv_train_is_off_by_default_and_reaches_both_layers():
    from moc_amd.model_mil import TransMIL
    from moc_amd.nystrom import LandmarkPinv, NystromAttention
    assert issubclass(LandmarkPinv, torch.autograd.Function)
    assert NystromAttention.fused_pinv_train is False
    assert NystromAttention(dim=512).fused_pinv_train is False
    model = TransMIL(n_classes=2, size_arg="conch")
    assert model.fused_pinv_train is False
    model.fused_pinv_train = True
    assert model.layer1.attn.fused_pinv_train is True and model.layer2.attn.fused_pinv_train is True
    assert model.fused_pinv_train is True
    assert not (model.fused or model.fused_pinv or model.fused_train or model.fused_conv)     # separate switches
    assert model.layer1.attn.fused_pinv is False
    model.layer2.attn.fused_pinv_train = False
    assert model.fused_pinv_train is False
    model.fused_pinv_train = False
    assert model.layer1.attn.fused_pinv_train is False
    assert sorted(model.state_dict()) == sorted(TransMIL(n_classes=2, size_arg="conch").state_dict())


ENTRIES = ("nystrom_pinv", "nystrom_pinv_iterates", "nystrom_pinv_backward", "nystrom_landmark_values", "nystrom_token_values",
           "nystrom_landmark_values_lse", "nystrom_landmark_backward", "nystrom_token_backward", "nystrom_conv_backward")


def _boom(monkeypatch):
    from moc_amd import engine

    def boom(*a, **k):
        raise AssertionError("a kernel wrapper was called on the CPU")
    for name in ENTRIES:
        monkeypatch.setattr(engine, name, boom)


def _all_on(m):
    m.fused = m.fused_pinv = m.fused_train = m.fused_conv = m.fused_pinv_train = True


@pytest.mark.parametrize("n", [257, 300])
def test_the_layer_on_the_cpu_is_the_torch_path_bit_for_bit(n, monkeypatch):
    from moc_amd.nystrom import NystromAttention
    _boom(monkeypatch)
    torch.manual_seed(290 + n)
    attn = NystromAttention(dim=512, dim_head=64, heads=8, num_landmarks=256, pinv_iterations=6, residual=True).eval()
    x = torch.nn.functional.layer_norm(HB.randn(9500 + n, 1, n, 512), (512,))
    G = HB.randn(9600 + n, 1, n, 512)

    def step():
        attn.zero_grad(set_to_none=True)
        leaf = x.clone().requires_grad_(True)
        out = attn(leaf)
        (out * G).sum().backward()
        return [out.detach(), leaf.grad] + [p.grad.clone() for p in attn.parameters()]

    plain = step()
    with torch.no_grad():
        plain_ng = attn(x)
    attn.fused_pinv_train = True                                              # alone: nothing
    assert all(torch.equal(a, b) for a, b in zip(step(), plain))
    _all_on(attn)
    assert all(torch.equal(a, b) for a, b in zip(step(), plain))
    with torch.no_grad():
        assert torch.equal(attn(x), plain_ng)


def test_transmil_on_the_cpu_is_the_torch_path_bit_for_bit(monkeypatch):
    from moc_amd.model_mil import TransMIL
    _boom(monkeypatch)
    torch.manual_seed(79)
    model = TransMIL(n_classes=3, size_arg="conch").eval()
    data = HB.randn(9700, 300, 512)

    def step():
        model.zero_grad(set_to_none=True)
        logits = model(data)[0]
        torch.nn.functional.cross_entropy(logits, torch.tensor([1])).backward()
        return [logits.detach()] + [p.grad.clone() for p in model.parameters() if p.grad is not None]

    plain = step()
    _all_on(model)
    got = step()
    assert len(got) == len(plain) > 10 and all(torch.equal(a, b) for a, b in zip(got, plain))
