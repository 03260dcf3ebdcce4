"""The landmark pseudo-inverse on HIP (moc_nystrom_pinv) without a GPU: the two C entries are exported and bound with the
documented signatures, the workspace is sized for the one built shape and 0 elsewhere, every contract violation is
refused on the host with a message that names it (made-up, never dereferenced device addresses: nothing is launched),
`fused_pinv` is off by default everywhere, and on the CPU it changes nothing."""
import ctypes as C

import pytest
import torch

import helpers_baselines as HB

P = C.c_void_p
MAT = 8 * 256 * 256 * 4                                               # bytes of one [8, 256, 256] fp32 matrix


def test_library_exports_the_pinv_entries_with_the_documented_signatures():
    from moc_amd import _lib
    h = _lib.lib()
    assert h.moc_version() == 20 and _lib.ABI_VERSION == 20
    want = {
        "moc_nystrom_pinv_workspace": (C.c_size_t, [C.c_int, C.c_int]),
        "moc_nystrom_pinv": (C.c_int, [P, C.c_int, C.c_int, C.c_int, P, P, C.c_size_t, P]),
    }
    for name, (res, args) in want.items():
        assert hasattr(h, name), name
        assert _lib.SIGNATURES[name] == (res, args), name
        fn = getattr(h, name)
        assert fn.restype is res and list(fn.argtypes) == args


def test_workspace_is_sized_for_the_built_shape_and_zero_elsewhere():
    from moc_amd import _lib
    h = _lib.lib()
    n = h.moc_nystrom_pinv_workspace(8, 256)
    assert n >= 5 * MAT and n % 16 == 0                               # XZ, P2, P3, a ping-pong Z, and the partial maxima
    for bad in [(4, 256), (8, 128), (8, 0), (16, 256), (8, 512), (0, 256), (-8, 256), (8, -256)]:
        assert h.moc_nystrom_pinv_workspace(*bad) == 0, bad


def _pinv(lib_, **over):
    a = dict(A=0x1000000, heads=8, landmarks=256, iters=6, Z=0x2000000, ws=0x4000000, ws_bytes=1 << 30)
    a.update(over)
    rc = lib_.moc_nystrom_pinv(a["A"], a["heads"], a["landmarks"], a["iters"], a["Z"], a["ws"], a["ws_bytes"], None)
    return rc, lib_.moc_last_error().decode()


EINVAL, EUNSUPPORTED = 1, 2


def _need():
    from moc_amd import _lib
    return _lib.lib().moc_nystrom_pinv_workspace(8, 256)


@pytest.mark.parametrize("over,code,word", [
    (dict(heads=4), EUNSUPPORTED, "heads=4"), (dict(heads=16), EUNSUPPORTED, "heads=16"), (dict(heads=0), EUNSUPPORTED, "heads=0"),
    (dict(landmarks=128), EUNSUPPORTED, "landmarks=128"), (dict(landmarks=512), EUNSUPPORTED, "landmarks=512"),
    (dict(landmarks=0), EUNSUPPORTED, "landmarks=0"),
    (dict(A=None), EINVAL, "A is null"), (dict(Z=None), EINVAL, "Z is null"), (dict(ws=None), EINVAL, "ws is null"),
    (dict(A=0x1000004), EINVAL, "aligned"), (dict(Z=0x2000008), EINVAL, "aligned"), (dict(ws=0x4000001), EINVAL, "aligned"),
    (dict(Z=0x1000000), EINVAL, "overlap"), (dict(Z=0x1000000 + MAT - 16), EINVAL, "overlap"),
    (dict(A=0x2000000 + MAT - 16), EINVAL, "overlap"),
    (dict(ws_bytes=0), EINVAL, "ws_bytes=0"), (dict(ws_bytes=5 * MAT), EINVAL, "ws_bytes"),
    (dict(iters=-1), EINVAL, "iters=-1"), (dict(iters=65), EINVAL, "iters=65"),
])
def test_pinv_refuses_on_the_host(over, code, word):
    from moc_amd import _lib
    rc, msg = _pinv(_lib.lib(), **over)
    assert rc == code and msg.startswith("moc_nystrom_pinv") and word in msg, (rc, msg)


def test_a_workspace_one_byte_short_is_refused_with_both_sizes_named():
    from moc_amd import _lib
    rc, msg = _pinv(_lib.lib(), ws_bytes=_need() - 1)
    assert rc == EINVAL and msg.startswith("moc_nystrom_pinv") and f"ws_bytes={_need() - 1}" in msg and str(_need()) in msg


def test_engine_entry_refuses_cpu_tensors_and_other_shapes():
    from moc_amd import engine
    with pytest.raises(AssertionError, match="no CPU fallback"):
        engine.nystrom_pinv(torch.zeros(8, 256, 256), 6)
    with pytest.raises(AssertionError, match="no CPU fallback"):
        engine.nystrom_pinv(torch.zeros(8, 128, 128), 6)


def test_fused_pinv_is_off_by_default():
    from moc_amd.model_mil import TransMIL
    from moc_amd.nystrom import NystromAttention
    assert NystromAttention.fused_pinv is False
    assert NystromAttention(dim=512).fused_pinv is False
    model = TransMIL(n_classes=2, size_arg="conch")
    assert model.fused_pinv is False and model.fused is False
    model.fused_pinv = True
    assert model.layer1.attn.fused_pinv is True and model.layer2.attn.fused_pinv is True and model.fused_pinv is True
    assert model.fused is False and model.layer1.attn.fused is False          # the two switches are separate
    model.layer2.attn.fused_pinv = False
    assert model.fused_pinv is False
    model.fused_pinv = False
    assert model.layer1.attn.fused_pinv is False
    assert sorted(model.state_dict()) == sorted(TransMIL(n_classes=2, size_arg="conch").state_dict())


@pytest.mark.parametrize("n", [1, 257, 700])
def test_fused_pinv_on_the_cpu_takes_the_torch_path(n, monkeypatch):
    from moc_amd import engine
    from moc_amd.nystrom import NystromAttention

    def boom(*a, **k):
        raise AssertionError("a kernel wrapper was called on the CPU")
    for name in ("nystrom_pinv", "nystrom_landmark_values", "nystrom_token_values"):
        monkeypatch.setattr(engine, name, boom)
    torch.manual_seed(190 + n)
    attn = NystromAttention(dim=512, dim_head=64, heads=8, num_landmarks=256, pinv_iterations=6, residual=True).eval()
    x = torch.nn.functional.layer_norm(HB.randn(9300 + n, 1, n, 512), (512,))
    with torch.no_grad():
        plain = attn(x)
        attn.fused_pinv = True                                                # alone: nothing
        assert torch.equal(attn(x), plain)
        attn.fused = True
        assert torch.equal(attn(x), plain) and torch.equal(attn.forward_fused(x), plain)
    y = attn(x)                                                               # gradient mode: still the torch path
    assert y.grad_fn is not None and torch.equal(y.detach(), plain)


def test_fused_pinv_transmil_on_the_cpu_takes_the_torch_path(monkeypatch):
    from moc_amd import engine
    from moc_amd.model_mil import TransMIL

    def boom(*a, **k):
        raise AssertionError("a kernel wrapper was called on the CPU")
    monkeypatch.setattr(engine, "nystrom_pinv", boom)
    torch.manual_seed(78)
    model = TransMIL(n_classes=3, size_arg="conch").eval()
    data = HB.randn(9400, 300, 512)
    with torch.no_grad():
        plain = model(data)
        model.fused = model.fused_pinv = True
        got = model(data)
    for a, b in zip(plain[:3], got[:3]):
        assert torch.equal(a, b)
