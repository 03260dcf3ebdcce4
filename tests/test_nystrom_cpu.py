"""The fused Nystrom forward without a GPU: the three C entries are exported and bound with the documented signatures,
moc_nystrom_workspace sizes the supported shape and returns 0 for every other, each contract violation is refused on the
host with a message (made-up, never dereferenced device addresses: nothing is launched), `fused` is off by default, and
with `fused = True` on the CPU NystromAttention and TransMIL give the torch path's result bit for bit."""
import ctypes as C

import pytest
import torch

import helpers_baselines as HB

P = C.c_void_p


def test_abi_version_is_still_20():
    from moc_amd import _lib
    assert _lib.lib().moc_version() == 20 and _lib.ABI_VERSION == 20


def test_library_exports_the_nystrom_entries_with_the_documented_signatures():
    from moc_amd import _lib
    h = _lib.lib()
    want = {
        "moc_nystrom_workspace": (C.c_size_t, [C.c_int64, C.c_int, C.c_int, C.c_int]),
        "moc_nystrom_landmark_values": (C.c_int, [P, C.c_int64, C.c_int, C.c_int, C.c_int, P, P, P, C.c_size_t, P]),
        "moc_nystrom_token_values": (C.c_int, [P, C.c_int64, C.c_int, C.c_int, C.c_int, P, P, P, C.c_int, C.c_float, P, P]),
    }
    for name, (res, args) in want.items():
        assert hasattr(h, name), name
        assert _lib.SIGNATURES[name] == (res, args), name
        fn = getattr(h, name)
        assert fn.restype is res and list(fn.argtypes) == args


def test_workspace_is_positive_for_the_built_shape_and_zero_elsewhere():
    from moc_amd import _lib
    h = _lib.lib()
    for j in (1, 2, 3, 9, 17, 60):
        n_pad = 256 * j
        chunks = (n_pad + 511) // 512                                 # one (max, sum, accumulator) triple per 512 tokens
        assert h.moc_nystrom_workspace(n_pad, 8, 64, 256) == chunks * 8 * 256 * 66 * 4
    for bad in [(0, 8, 64, 256), (-256, 8, 64, 256), (255, 8, 64, 256), (257, 8, 64, 256), (128, 8, 64, 256), (600, 8, 64, 256),
                (512, 4, 64, 256), (512, 16, 64, 256), (512, 8, 32, 256), (512, 8, 128, 256), (512, 8, 64, 128),
                (512, 8, 64, 512), (512, 8, 64, 0), (512, 0, 64, 256), (512, 8, 0, 256)]:
        assert h.moc_nystrom_workspace(*bad) == 0, bad


def _landmark(lib_, **over):
    a = dict(qkv=0x10000, n_pad=512, heads=8, dim_head=64, landmarks=256, q_l=0x20000, W=0x30000, ws=0x40000, ws_bytes=1 << 30)
    a.update(over)
    rc = lib_.moc_nystrom_landmark_values(a["qkv"], a["n_pad"], a["heads"], a["dim_head"], a["landmarks"], a["q_l"], a["W"],
                                          a["ws"], a["ws_bytes"], None)
    return rc, lib_.moc_last_error().decode()


def _token(lib_, **over):
    a = dict(qkv=0x10000, n_pad=512, heads=8, dim_head=64, landmarks=256, k_l=0x20000, Y=0x30000, conv_w=0x40000, taps=33,
             scale=0.125, out=0x50000)
    a.update(over)
    rc = lib_.moc_nystrom_token_values(a["qkv"], a["n_pad"], a["heads"], a["dim_head"], a["landmarks"], a["k_l"], a["Y"],
                                       a["conv_w"], a["taps"], C.c_float(a["scale"]), a["out"], None)
    return rc, lib_.moc_last_error().decode()


SHAPE_REFUSALS = [
    (dict(n_pad=0), "n_pad"), (dict(n_pad=255), "n_pad"), (dict(n_pad=128), "n_pad"), (dict(n_pad=257), "n_pad"),
    (dict(n_pad=700), "n_pad"), (dict(n_pad=-256), "n_pad"),
    (dict(heads=4), "heads=4"), (dict(heads=16), "heads=16"), (dict(dim_head=32), "dim_head=32"), (dict(dim_head=128), "dim_head=128"),
    (dict(landmarks=128), "landmarks=128"), (dict(landmarks=512), "landmarks=512"), (dict(landmarks=0), "landmarks=0"),
]


@pytest.mark.parametrize("over,word", SHAPE_REFUSALS + [
    (dict(qkv=None), "qkv"), (dict(q_l=None), "q_l"), (dict(W=None), "W"), (dict(ws=None), "ws"),
    (dict(ws_bytes=8 * 256 * 66 * 4 - 1), "ws_bytes"), (dict(n_pad=1024, ws_bytes=8 * 256 * 66 * 4), "ws_bytes"),
    (dict(qkv=0x10004), "aligned"), (dict(W=0x30008), "aligned"),
])
def test_landmark_values_refuses_on_the_host(over, word):
    from moc_amd import _lib
    rc, msg = _landmark(_lib.lib(), **over)
    assert rc != 0 and msg.startswith("moc_nystrom_landmark_values") and word in msg, (rc, msg)


@pytest.mark.parametrize("over,word", SHAPE_REFUSALS + [
    (dict(qkv=None), "qkv"), (dict(k_l=None), "k_l"), (dict(Y=None), "Y"), (dict(out=None), "out"),
    (dict(taps=32), "taps=32"), (dict(taps=0), "taps=0"), (dict(taps=2), "taps=2"), (dict(taps=35), "taps=35"),
    (dict(taps=34), "taps=34"), (dict(taps=-1), "taps=-1"),
    (dict(scale=float("nan")), "scale"), (dict(out=0x50004), "aligned"),
])
def test_token_values_refuses_on_the_host(over, word):
    from moc_amd import _lib
    rc, msg = _token(_lib.lib(), **over)
    assert rc != 0 and msg.startswith("moc_nystrom_token_values") and word in msg, (rc, msg)


def test_unsupported_shapes_are_reported_as_unsupported():
    from moc_amd import _lib
    h = _lib.lib()
    assert _landmark(h, heads=4)[0] == 2 and _token(h, landmarks=128)[0] == 2 and _token(h, taps=35)[0] == 2      # MOC_EUNSUPPORTED
    assert _landmark(h, n_pad=700)[0] == 1 and _token(h, taps=32)[0] == 1 and _token(h, qkv=None)[0] == 1         # MOC_EINVAL


def test_engine_entries_refuse_cpu_tensors_and_bad_shapes():
    from moc_amd import engine
    hmd = torch.zeros(8, 256, 64)
    with pytest.raises(AssertionError, match="no CPU fallback"):
        engine.nystrom_landmark_values(torch.zeros(256, 1536), hmd)
    with pytest.raises(AssertionError, match="no CPU fallback"):
        engine.nystrom_token_values(torch.zeros(256, 1536), hmd, hmd, None, 0.125)


def test_fused_is_off_by_default():
    from moc_amd.model_mil import TransMIL
    from moc_amd.nystrom import NystromAttention
    assert NystromAttention.fused is False and callable(NystromAttention.forward_fused)
    assert NystromAttention(dim=512).fused is False
    model = TransMIL(n_classes=2, size_arg="conch")
    assert model.fused is False
    model.fused = True
    assert model.layer1.attn.fused is True and model.layer2.attn.fused is True and model.fused is True
    model.layer2.attn.fused = False
    assert model.fused is False
    model.fused = False
    assert model.layer1.attn.fused is False
    assert sorted(model.state_dict()) == sorted(TransMIL(n_classes=2, size_arg="conch").state_dict())


@pytest.mark.parametrize("n", [1, 255, 257, 700])
def test_fused_attention_on_the_cpu_takes_the_torch_path(n, monkeypatch):
    from moc_amd import engine
    from moc_amd.nystrom import NystromAttention

    def boom(*a, **k):
        raise AssertionError("a kernel wrapper was called on the CPU")
    monkeypatch.setattr(engine, "nystrom_landmark_values", boom)
    monkeypatch.setattr(engine, "nystrom_token_values", boom)
    torch.manual_seed(90 + n)
    attn = NystromAttention(dim=512, dim_head=64, heads=8, num_landmarks=256, pinv_iterations=6, residual=True).eval()
    x = torch.nn.functional.layer_norm(HB.randn(9100 + n, 1, n, 512), (512,))
    with torch.no_grad():
        plain = attn(x)
        attn.fused = True
        assert torch.equal(attn(x), plain) and torch.equal(attn.forward_fused(x), plain)
    y = attn(x)                                                               # gradient mode: still the torch path
    assert y.grad_fn is not None and torch.equal(y.detach(), plain)
    with pytest.raises(AssertionError):                                       # the torch code's own refusal
        attn(x, return_attn=True)


def test_fused_transmil_on_the_cpu_takes_the_torch_path():
    from moc_amd.model_mil import TransMIL
    torch.manual_seed(77)
    model = TransMIL(n_classes=3, size_arg="conch").eval()
    data = HB.randn(9200, 300, 512)
    with torch.no_grad():
        plain, plain_rows = model(data), model.forward_patch_level(data)
        model.fused = True
        got, got_rows = model(data), model.forward_patch_level(data)
    for a, b in zip(plain[:3], got[:3]):
        assert torch.equal(a, b)
    assert torch.equal(plain_rows, got_rows)
