"""Attention rows without a GPU (moc_nystrom_attention_rows; engine.nystrom_attention_rows; NystromAttention.forward_rows;
TransMIL.attention_maps): the C entry is exported, declared and bound and refuses on the host (made-up, never dereferenced
device addresses: nothing is launched); the engine wrapper refuses CPU tensors; on the CPU forward_rows and attention_maps
run the torch code -- every engine.nystrom_* wrapper is made to raise -- and give forward's own bits beside rows that are
checked against a float64 evaluation of the WHOLE matrix attn1 @ pinv @ attn3 (`full_attention`, rows picked afterwards),
against exact softmax attention in the limit where every token is its own landmark, and against the identity that a full
row sums to coef.sum()."""
import copy
import ctypes as C
import os
import re
from math import ceil

import pytest
import torch
import torch.nn.functional as F

import helpers_baselines as HB

P = C.c_void_p
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "moc_nystrom_attention_rows"
SIGNATURE = (C.c_int, [P, C.c_int64, C.c_int, C.c_int, C.c_int, P, P, P, C.c_int, P, P])
EINVAL, EUNSUPPORTED = 1, 2
POINTERS = ("qkv", "q_l", "lse", "coef", "out")
WRAPPERS = ("nystrom_landmark_values", "nystrom_token_values", "nystrom_landmark_values_lse", "nystrom_landmark_backward",
            "nystrom_token_backward", "nystrom_conv_backward", "nystrom_pinv", "nystrom_pinv_iterates", "nystrom_pinv_backward",
            "nystrom_attention_rows", "ppeg_forward", "ppeg_backward")


def full_attention(att, x):
    """(attn1 @ pinv @ attn3 [b, h, n_pad, n_pad], coef = attn1 @ pinv [b, h, n_pad, m]) of layer `att` for x [b, n, dim], in
    their precision: moc_amd/nystrom.py's _forward_torch restated up to the three softmax kernels."""
    from moc_amd.nystrom import moore_penrose_iter_pinv
    b, n, _ = x.shape
    h, m = att.heads, att.num_landmarks
    if n % m > 0:
        x = F.pad(x, (0, 0, m - (n % m), 0), value=0)
    q, k, _ = (t.reshape(b, t.shape[1], h, -1).transpose(1, 2) for t in att.to_qkv(x).chunk(3, dim=-1))
    q = q * att.scale
    l = ceil(n / m)
    q_l = q.reshape(b, h, -1, l, q.shape[-1]).sum(dim=3) / l
    k_l = k.reshape(b, h, -1, l, k.shape[-1]).sum(dim=3) / l
    attn1 = (q @ k_l.transpose(-1, -2)).softmax(dim=-1)
    attn2 = (q_l @ k_l.transpose(-1, -2)).softmax(dim=-1)
    attn3 = (q_l @ k.transpose(-1, -2)).softmax(dim=-1)
    coef = attn1 @ moore_penrose_iter_pinv(attn2, att.pinv_iterations)
    return coef @ attn3, coef


def reference_rows(att, x, rows):
    """[h, R, n] in float64: the rows of the full matrix of a double copy of `att`, the last n columns (batch 1)."""
    n = x.shape[1]
    with torch.no_grad():
        full, _ = full_attention(copy.deepcopy(att).double(), x.double())
    pad = full.shape[-1] - n
    return full[0][:, [pad + r for r in rows], pad:]


@pytest.fixture
def no_kernels(monkeypatch):
    from moc_amd import engine

    def boom(*a, **k):
        raise AssertionError("a kernel wrapper was called on the CPU")
    for name in WRAPPERS:
        monkeypatch.setattr(engine, name, boom)


def test_the_entry_is_exported_declared_and_bound():
    from moc_amd import _lib, engine
    h = _lib.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "moc_hip.h")).read(), flags=re.S)
    assert hasattr(h, NAME)
    decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, header)
    assert decl, f"{NAME} is not declared in moc_hip.h"
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["const float* qkv", "int64_t n_pad", "int heads", "int dim_head", "int landmarks", "const float* q_l",
                    "const float* lse", "const float* coef", "int R", "float* out", "moc_stream_t stream"], args
    assert _lib.SIGNATURES[NAME] == SIGNATURE
    fn = getattr(h, NAME)
    assert fn.restype is SIGNATURE[0] and list(fn.argtypes) == SIGNATURE[1]
    assert h.moc_version() == 20 and _lib.ABI_VERSION == 20
    assert engine.NYSTROM_MAX_ROWS == 16


BIG = 1 << 36                                                                 # bytes between two made-up buffers


def _call(h, **over):
    a = dict(n_pad=512, heads=8, dim_head=64, landmarks=256, R=3)
    a.update({p: (k + 1) * BIG for k, p in enumerate(POINTERS)})
    a.update(over)
    rc = getattr(h, NAME)(a["qkv"], a["n_pad"], a["heads"], a["dim_head"], a["landmarks"], a["q_l"], a["lse"], a["coef"], a["R"],
                          a["out"], None)
    return rc, h.moc_last_error().decode()


def test_the_entry_refuses_on_the_host():
    from moc_amd import _lib
    h = _lib.lib()
    for over in (dict(heads=4), dict(heads=16), dict(dim_head=32), dict(dim_head=128), dict(landmarks=128), dict(landmarks=512),
                 dict(n_pad=(1 << 22) + 256), dict(n_pad=1 << 23)):
        rc, msg = _call(h, **over)
        assert rc == EUNSUPPORTED and msg.startswith(NAME), (over, rc, msg)
    for n_pad in (0, -256, 255, 257, 300, 128):
        rc, msg = _call(h, n_pad=n_pad)
        assert rc == EINVAL and msg.startswith(NAME) and "n_pad" in msg, (n_pad, rc, msg)
    for R in (0, 17, -1, 256):
        rc, msg = _call(h, R=R)
        assert rc == EINVAL and msg.startswith(NAME) and "R=" in msg, (R, rc, msg)
    for p in POINTERS:
        rc, msg = _call(h, **{p: None})
        assert rc == EINVAL and msg.startswith(NAME) and "null" in msg, (p, rc, msg)
        rc, msg = _call(h, **{p: BIG + 4})
        assert rc == EINVAL and msg.startswith(NAME) and "aligned" in msg, (p, rc, msg)
    rc, msg = _call(h, **{p: None for p in POINTERS})
    assert rc == EINVAL and msg.startswith(NAME), (rc, msg)
    sizes = dict(qkv=512 * 1536 * 4, q_l=8 * 256 * 64 * 4, lse=8 * 256 * 4, coef=8 * 3 * 256 * 4)
    out_bytes = 8 * 3 * 512 * 4
    for other, nbytes in sizes.items():                                       # `out` inside, at either end of and around each input
        for out in (BIG, BIG + 16, BIG + nbytes - 16, BIG - out_bytes + 16):
            rc, msg = _call(h, **{other: BIG, "out": out})
            assert rc == EINVAL and msg.startswith(NAME) and "overlaps" in msg, (other, out, rc, msg)
    # (a valid call is not made here: it would launch)


def test_the_engine_wrapper_refuses_cpu_tensors():
    from moc_amd import engine
    with pytest.raises(AssertionError, match="no CPU fallback"):
        engine.nystrom_attention_rows(torch.zeros(256, 1536), torch.zeros(8, 256, 64), torch.zeros(8, 256), torch.zeros(8, 1, 256))


def _small(seed=0, **kw):
    from moc_amd.nystrom import NystromAttention
    torch.manual_seed(seed)
    kw = dict(dict(dim=64, dim_head=8, heads=8, num_landmarks=16), **kw)
    return NystromAttention(**kw).eval()


@pytest.mark.parametrize("fused", [False, True])
def test_forward_rows_on_the_cpu(no_kernels, fused):
    att = _small(11)
    att.fused = att.fused_pinv = fused                                        # on the CPU the switches change nothing
    x, rows = HB.randn(9700, 1, 37, 64), [0, 36]                              # 37 -> padded to 48 at the front
    with torch.no_grad():
        want = att(x)
    x.requires_grad_(True)                                                    # a wanted gradient changes nothing either
    out, attn = att.forward_rows(x, rows)
    assert torch.equal(out, want) and not out.requires_grad and not attn.requires_grad
    assert attn.shape == (8, 2, 37) and attn.dtype == torch.float32
    ref = reference_rows(att, x.detach(), rows)
    err = float((attn.double() - ref).abs().max())
    print(f"forward_rows cpu fused={fused}: max|ref| {float(ref.abs().max()):.3e}  error {err:.3e}")
    assert torch.allclose(attn.double(), ref, rtol=0, atol=1e-5)
    _, again = att.forward_rows(x, torch.tensor(rows))                         # a tensor of indices is as good as a list
    assert torch.equal(again, attn)
    _, one = att.forward_rows(x, [36])
    # (a product of one row may add its 16 + 16 terms, each at most 1, in another order than a product of two: 32 x 2^-24)
    assert one.shape == (8, 1, 37) and torch.allclose(one[:, 0], attn[:, 1], rtol=0, atol=2e-6)


def test_rows_are_exact_attention_where_every_token_is_a_landmark():
    """tests/test_baselines_cpu.py test_nystrom_attention_restatement_limits' configuration and tolerance."""
    att = _small(0, num_landmarks=32, pinv_iterations=30, residual=False)
    x, rows = HB.randn(9701, 2, 32, 64), [0, 5, 31]
    out, attn = att.forward_rows(x, rows)
    with torch.no_grad():
        assert torch.equal(out, att(x))
        q, k, _ = (t.reshape(2, 32, 8, 8).transpose(1, 2) for t in att.to_qkv(x).chunk(3, -1))
        exact = torch.softmax(q * att.scale @ k.transpose(-1, -2), -1)[:, :, rows]
    assert attn.shape == (2, 8, 3, 32)                                        # a batch keeps its dimension
    print(f"exact-attention limit: error {float((attn - exact).abs().max()):.3e}")
    assert torch.allclose(attn, exact, rtol=0, atol=2e-4)


@pytest.mark.parametrize("n", [48, 37])
def test_a_full_row_sums_to_its_coefficients(n):
    """The rows of attn3 sum to one, so a row of attn1 @ pinv @ attn3 over all n_pad columns sums to coef.sum(); without
    padding forward_rows returns all of them.  With padding the real tokens hold only a part: no constant is asserted."""
    att = _small(12).double()
    x, rows = HB.randn(9702 + n, 1, n, 64).double(), [0, 7, n - 1]
    with torch.no_grad():
        full, coef = full_attention(att, x)
    pad = full.shape[-1] - n
    pick = [pad + r for r in rows]
    assert torch.allclose(full[0][:, pick].sum(-1), coef[0][:, pick].sum(-1), rtol=0, atol=1e-12)
    _, attn = att.forward_rows(x, rows)
    assert attn.dtype == torch.float64 and torch.allclose(attn, full[0][:, pick, pad:], rtol=0, atol=1e-12)
    if pad == 0:
        assert torch.allclose(attn.sum(-1), coef[0][:, pick].sum(-1), rtol=0, atol=1e-12)
    else:
        share = attn.sum(-1) / coef[0][:, pick].sum(-1)
        print(f"n={n}: the real tokens hold {float(share.mean()):.3f} of a row (the padding's zero keys the rest)")
        assert not torch.allclose(attn.sum(-1), coef[0][:, pick].sum(-1), rtol=0, atol=1e-3)


@pytest.mark.parametrize("rows", [[], [-1], [37], [0, 37], [3, -2]])
def test_bad_rows_raise(rows):
    att = _small(13)
    with pytest.raises(ValueError, match="rows"):
        att.forward_rows(torch.zeros(1, 37, 64), rows)


def test_attention_maps_on_the_cpu(no_kernels):
    from moc_amd.model_mil import TransMIL
    torch.manual_seed(21)
    model = TransMIL(n_classes=2, size_arg="conch").eval()
    data = torch.randn(50, 512)
    with torch.no_grad():
        want = model(data)[0]
    for switches in ((), ("fused", "fused_pinv", "fused_train", "fused_conv", "fused_pinv_train", "fused_ppeg")):
        twin = copy.deepcopy(model)
        for s in switches:
            setattr(twin, s, True)
        logits, maps = twin.attention_maps(data)
        assert torch.equal(logits, want) and not logits.requires_grad
        assert sorted(maps) == ["layer1", "layer2"]
        for k, a in maps.items():
            assert a.shape == (8, 50) and torch.isfinite(a).all() and not a.requires_grad, k
    assert sorted(model.state_dict()) == sorted(TransMIL(n_classes=2, size_arg="conch").state_dict())


def test_a_map_is_the_class_tokens_row_of_the_layer():
    """attention_maps' layer-1 map against the layer asked directly: row 0, columns 1..n of the 1 + side^2 tokens."""
    from moc_amd.model_mil import TransMIL
    torch.manual_seed(22)
    model = TransMIL(n_classes=2, size_arg="conch").eval()
    data = torch.randn(50, 512)                                               # side 8: 64 patch tokens, 14 of them wrap-around
    _, maps = model.attention_maps(data)
    with torch.no_grad():
        h, side, n = model._embed(data)
        assert (tuple(h.shape), side, n) == ((1, 65, 512), 8, 50)
        x = model.layer1.norm(h)
    ref = reference_rows(model.layer1.attn, x, [0])
    assert torch.allclose(maps["layer1"].double(), ref[:, 0, 1:51], rtol=0, atol=1e-5)
