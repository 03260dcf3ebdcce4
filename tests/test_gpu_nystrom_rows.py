"""Attention rows on the GPU (moc_nystrom_attention_rows; engine.nystrom_attention_rows; NystromAttention.forward_rows;
TransMIL.attention_maps): the entry alone against a float64 evaluation on the CPU, value range, exact checks, what it
writes, row sums, the layer, the model, and which path a call takes.

The judging rule is that of tests/test_gpu_nystrom_conv.py (its `_judge`): in the same test torch's fp32 evaluation on the
GPU and the fused path are each compared with the float64 evaluation; the fused error may be at most max(f x torch's error,
2^-20 x max|reference|) and never more than 1e-4 x max(1, max|reference|).  f = 2 for the entry alone, f = 4 for the layer and
the model.  Both errors are printed.

Inputs come from a seeded layer: qkv from to_qkv, q_l and k_l from the landmark means, lse from
engine.nystrom_landmark_values_lse, coef = softmax_256(scale q[rows] k_l^T) pinv.  Shapes: a workgroup is one head x 256
tokens, so n_pad = 256 is one workgroup a head (and one token per landmark), 512 and 768 two and three, 2,304 nine; a wave
takes two 16-token tiles; R = 1, 3 and 16 are one row, a part of one group of four rows, and the whole MFMA tile.  The layer
runs on 600 and 2,100 tokens (front padding 168 and 204), the model on a 600-patch bag (626 tokens, padded to 768)."""
import copy
import functools
import math

import pytest
import torch

import helpers_baselines as HB
from test_gpu_nystrom_conv import _judge
from test_gpu_nystrom_train import _layer, _model, _tokens
from test_nystrom_rows_cpu import reference_rows

pytestmark = pytest.mark.gpu

H, D, M = 8, 64, 256
SCALE = D ** -0.5
ENTRIES = ("nystrom_landmark_values", "nystrom_landmark_values_lse", "nystrom_token_values", "nystrom_pinv", "nystrom_attention_rows")


def _heads(qkv, part):
    return qkv[:, 512 * part:512 * (part + 1)].reshape(qkv.shape[0], H, D).transpose(0, 1)       # [8, n, 64]


@functools.lru_cache(maxsize=None)
def _inputs(n_pad, gain=1):
    """(qkv [n_pad, 1536], q_l, k_l [8, 256, 64], pinv [8, 256, 256]) in fp32 on the CPU, from a seeded layer whose input is
    scaled by `gain`."""
    from moc_amd.nystrom import moore_penrose_iter_pinv
    with torch.no_grad():
        qkv = _layer(9101).to_qkv(_tokens(9100 + n_pad, n_pad) * gain)[0].contiguous()
        q_l = (_heads(qkv, 0) * SCALE).reshape(H, M, -1, D).sum(dim=2) / (n_pad // M)
        k_l = _heads(qkv, 1).reshape(H, M, -1, D).sum(dim=2) / (n_pad // M)
        pinv = moore_penrose_iter_pinv((q_l @ k_l.transpose(1, 2)).softmax(dim=-1), 6)
    return qkv, q_l.contiguous(), k_l.contiguous(), pinv


def _rows(n_pad, R):
    return [(i * (n_pad - 1)) // max(R - 1, 1) for i in range(R)]              # 0 .. n_pad - 1, both ends included


@functools.lru_cache(maxsize=None)
def _case(n_pad, R, gain=1):
    """(qkv, q_l, coef [8, R, 256]) in fp32 and the float64 out [8, R, n_pad] = coef softmax(q_l k^T, -1), all on the CPU."""
    qkv, q_l, k_l, pinv = _inputs(n_pad, gain)
    with torch.no_grad():
        q_r = _heads(qkv, 0)[:, _rows(n_pad, R)] * SCALE
        coef = ((q_r @ k_l.transpose(1, 2)).softmax(dim=-1) @ pinv).contiguous()
        ref = coef.double() @ (q_l.double() @ _heads(qkv.double(), 1).transpose(1, 2)).softmax(dim=-1)
    return (qkv, q_l, coef), ref


def _run(qkv, q_l, coef):
    from moc_amd import engine
    _, lse = engine.nystrom_landmark_values_lse(qkv, q_l)
    return engine.nystrom_attention_rows(qkv, q_l, lse, coef), lse


def _torch32(qkv, q_l, coef):
    return coef @ (q_l @ _heads(qkv, 1).transpose(1, 2)).softmax(dim=-1)


@pytest.mark.parametrize("R", [1, 3, 16])
@pytest.mark.parametrize("n_pad", [256, 512, 768, 2304])
def test_entry_matches_float64(gpu_device, n_pad, R):
    cpu, ref = _case(n_pad, R)
    qkv, q_l, coef = (t.to(gpu_device) for t in cpu)
    keep = [t.clone() for t in (qkv, q_l, coef)]
    out, lse = _run(qkv, q_l, coef)
    assert out.shape == (H, R, n_pad) and out.dtype == torch.float32
    assert all(torch.equal(a, b) for a, b in zip((qkv, q_l, coef), keep)), "an input was written"
    _judge(f"rows entry n_pad={n_pad} R={R}", out, _torch32(qkv, q_l, coef), ref, 2)


@pytest.mark.parametrize("n_pad,R", [(512, 3), (2304, 16)])
def test_entry_keeps_its_range(gpu_device, n_pad, R):
    """The layer input scaled by 8: scores 64 times as large, most weights underflow; exp(s - lse) must stay finite."""
    cpu, ref = _case(n_pad, R, 8)
    qkv, q_l, coef = (t.to(gpu_device) for t in cpu)
    top = float((q_l.double() @ _heads(qkv.double(), 1).transpose(1, 2)).abs().max())
    assert top > 10.0, top                                                    # "into the tens"
    out, lse = _run(qkv, q_l, coef)
    print(f"rows range n_pad={n_pad}: largest |score| {top:.1f}, lse up to {float(lse.max()):.1f}, "
          f"{float((ref == 0).double().mean()):.3f} of the float64 outputs are exact zeros")
    _judge(f"rows range n_pad={n_pad} R={R}", out, _torch32(qkv, q_l, coef), ref, 2)


def test_zero_coefficients_give_exact_zeros(gpu_device):
    qkv, q_l, coef = (t.to(gpu_device) for t in _case(768, 3)[0])
    out, _ = _run(qkv, q_l, torch.zeros_like(coef))
    assert out.shape == (H, 3, 768) and not out.any()


@pytest.mark.parametrize("m", [0, 15, 16, 255])
def test_a_one_hot_row_is_a_row_of_attn3_and_scales_exactly(gpu_device, m):
    n_pad = 512
    (qkv, q_l, _), _ = _case(n_pad, 3)
    coef = torch.zeros(H, 2, M)
    coef[:, 0, m], coef[:, 1, m] = 1.0, 2.0
    ref = (q_l.double() @ _heads(qkv.double(), 1).transpose(1, 2)).softmax(dim=-1)[:, m]
    g = [t.to(gpu_device) for t in (qkv, q_l, coef)]
    out, _ = _run(*g)
    assert bool((out[:, 1] == 2 * out[:, 0]).all()), "doubling a coefficient must double the row exactly"
    assert bool((out[:, 0] > 0).all())
    _judge(f"rows one-hot m={m}", out[:, 0], _torch32(*g)[:, 0], ref, 2)


def test_entry_is_deterministic_and_stream_independent(gpu_device):
    from moc_amd import engine
    qkv, q_l, coef = (t.to(gpu_device) for t in _case(2304, 16)[0])
    _, lse = engine.nystrom_landmark_values_lse(qkv, q_l)
    a, b = engine.nystrom_attention_rows(qkv, q_l, lse, coef), engine.nystrom_attention_rows(qkv, q_l, lse, coef)
    assert torch.equal(a, b)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = engine.nystrom_attention_rows(qkv, q_l, lse, coef)
    side.synchronize()
    assert torch.equal(a, c)


@pytest.mark.parametrize("n_pad", [256, 2304])
def test_entry_stays_inside_its_buffer(gpu_device, n_pad):
    """0xA5 bands before and after `out`; with R = 3 and room for 16 rows a head, everything past the [8, 3, n_pad] block
    keeps the sentinel."""
    from moc_amd import _lib, engine
    dev, h, pad, R = gpu_device, _lib.lib(), 4096, 3
    qkv, q_l, coef = (t.to(dev) for t in _case(n_pad, R)[0])
    keep = [t.clone() for t in (qkv, q_l, coef)]
    _, lse = engine.nystrom_landmark_values_lse(qkv, q_l)
    want = engine.nystrom_attention_rows(qkv, q_l, lse, coef)
    room, used = H * 16 * n_pad, H * R * n_pad
    buf = torch.full(((room + 2 * pad) * 4,), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    rc = h.moc_nystrom_attention_rows(qkv.data_ptr(), n_pad, H, D, M, q_l.data_ptr(), lse.data_ptr(), coef.data_ptr(), R,
                                      buf.data_ptr() + 4 * pad, None)
    assert rc == 0, h.moc_last_error()
    torch.cuda.synchronize()
    assert bool((buf[:4 * pad] == 0xA5).all()), "written before out"
    assert bool((buf[4 * (pad + used):] == 0xA5).all()), "written past the R rows"
    assert torch.equal(buf[4 * pad:4 * (pad + used)].view(torch.float32).view(H, R, n_pad), want)
    assert all(torch.equal(a, b) for a, b in zip((qkv, q_l, coef), keep)), "an input was written"


@pytest.mark.parametrize("n_pad,R", [(256, 16), (2304, 3)])
def test_row_sums_are_the_coefficient_sums(gpu_device, n_pad, R):
    """The rows of attn3 sum to one: each output may be off by the rule's floor, a sum over n_pad of them by n_pad floors."""
    cpu, ref = _case(n_pad, R)
    qkv, q_l, coef = (t.to(gpu_device) for t in cpu)
    out, _ = _run(qkv, q_l, coef)
    got, want = out.double().sum(-1).cpu(), cpu[2].double().sum(-1)
    bound = n_pad * 2.0 ** -20 * float(ref.abs().max())
    err = float((got - want).abs().max())
    print(f"rows sums n_pad={n_pad} R={R}: coef sums {float(want.min()):.4f} .. {float(want.max()):.4f}  error {err:.3e}  (bound {bound:.3e})")
    assert err <= bound


# ---------------------------------------------------------------- the layer
@pytest.fixture
def calls(monkeypatch):
    from moc_amd import engine
    seen = {}
    for name in ENTRIES:
        real = getattr(engine, name)
        seen[name] = 0

        def counted(*a, _real=real, _name=name, **k):
            seen[_name] += 1
            return _real(*a, **k)
        monkeypatch.setattr(engine, name, counted)
    return seen


def _reset(calls):
    for k in calls:
        calls[k] = 0


@functools.lru_cache(maxsize=None)
def _layer_case(n):
    """(layer, x [1, n, 512], rows) on the CPU and the float64 rows [8, R, n]."""
    layer, x, rows = _layer(9200), _tokens(9300 + n, n), [0, 1, n // 2, n - 1]
    return (layer, x, rows), reference_rows(layer, x, rows)


@pytest.mark.parametrize("n", [600, 2100])
def test_layer_rows(gpu_device, calls, n):
    (layer, x, rows), ref = _layer_case(n)
    attn, gx = copy.deepcopy(layer).to(gpu_device), x.to(gpu_device)
    with torch.no_grad():
        plain_out = attn(gx)
    out32, rows32 = attn.forward_rows(gx, rows)                               # `fused` off: the torch code
    assert torch.equal(out32, plain_out) and not any(calls.values())
    assert rows32.shape == (H, len(rows), n)

    attn.fused = True
    with torch.no_grad():
        fused_out = attn(gx)
    _reset(calls)
    out, got = attn.forward_rows(gx, rows)
    assert calls == {"nystrom_landmark_values": 0, "nystrom_landmark_values_lse": 1, "nystrom_token_values": 1, "nystrom_pinv": 0,
                     "nystrom_attention_rows": 1}, calls
    assert torch.equal(out, fused_out), "out differs from the fused forward"
    assert got.shape == (H, len(rows), n) and not out.requires_grad and not got.requires_grad
    _judge(f"layer rows n={n}", got, rows32, ref, 4)

    attn.fused_pinv = True
    with torch.no_grad():
        fused_out = attn(gx)
    _reset(calls)
    out, got = attn.forward_rows(gx, rows)
    assert calls["nystrom_pinv"] == 1 and calls["nystrom_attention_rows"] == 1 and calls["nystrom_landmark_values_lse"] == 1
    assert torch.equal(out, fused_out), "out differs from the fused forward with fused_pinv"
    _judge(f"layer rows n={n} fused_pinv", got, rows32, ref, 4)


def test_which_path_a_call_takes(gpu_device, calls):
    (layer, x, _), _ = _layer_case(600)
    attn, gx = copy.deepcopy(layer).to(gpu_device), x.to(gpu_device)
    attn.fused = True
    with torch.no_grad():
        fused_out = attn(gx)
    _reset(calls)
    many = list(range(0, 17 * 35, 35))                                        # 17 rows: one more than a call takes
    out, got = attn.forward_rows(gx, many)
    assert calls["nystrom_attention_rows"] == 0 and calls["nystrom_landmark_values_lse"] == 0, calls
    assert torch.equal(out, fused_out) and got.shape == (H, 17, 600)          # `out` keeps forward's bits
    _, sixteen = attn.forward_rows(gx, many[:16])
    assert calls["nystrom_attention_rows"] == 1
    assert torch.allclose(sixteen, got[:, :16], rtol=0, atol=1e-5)
    _reset(calls)
    plain = copy.deepcopy(attn)
    plain.fused = False
    for a_x in (torch.cat([gx, gx.flip(1)]), gx.double()):                    # a batch, another dtype: the torch code
        a = copy.deepcopy(attn).to(a_x.dtype)
        b = copy.deepcopy(plain).to(a_x.dtype)
        (o1, r1), (o2, r2) = a.forward_rows(a_x, [0, 5]), b.forward_rows(a_x, [0, 5])
        assert torch.equal(o1, o2) and torch.equal(r1, r2)
    assert not any(calls.values()), calls
    gx.requires_grad_(True)                                                   # a wanted gradient changes nothing: no_grad inside
    out, got = attn.forward_rows(gx, [0])
    assert calls["nystrom_attention_rows"] == 1 and torch.equal(out, fused_out) and not out.requires_grad
    with pytest.raises(ValueError, match="rows"):
        attn.forward_rows(gx, [600])


# ---------------------------------------------------------------- the model
def _maps64(m, data):
    """The two maps of a float64 TransMIL: tests/test_gpu_nystrom_train.py's `_logits64` walk, each layer's class-token row
    taken from the whole matrix (test_nystrom_rows_cpu.reference_rows)."""
    h = m._fc1(data.unsqueeze(0))
    n = h.shape[1]
    side = int(math.ceil(math.sqrt(n)))
    h = torch.cat([h, h[:, :side * side - n]], dim=1)
    h = torch.cat((m.cls_token.expand(1, -1, -1), h), dim=1)
    a1 = reference_rows(m.layer1.attn, m.layer1.norm(h), [0])
    h = m.pos_layer(m.layer1(h), side, side)
    a2 = reference_rows(m.layer2.attn, m.layer2.norm(h), [0])
    return {"layer1": a1[:, 0, 1:n + 1], "layer2": a2[:, 0, 1:n + 1]}


@functools.lru_cache(maxsize=None)
def _model_case():
    data = HB.randn(9400, 600, 512)
    m64 = copy.deepcopy(_model()).double()
    with torch.no_grad():
        return data, _maps64(m64, data.double())


@pytest.mark.parametrize("switches", [("fused",), ("fused", "fused_pinv", "fused_ppeg")])
def test_attention_maps(gpu_device, calls, switches):
    data, ref = _model_case()
    model, g = copy.deepcopy(_model()).to(gpu_device), data.to(gpu_device)
    plain_logits, plain = model.attention_maps(g)                             # every switch off: the torch code
    assert not any(calls.values())
    with torch.no_grad():
        assert torch.equal(plain_logits, model(g)[0])
    for k in ("layer1", "layer2"):
        err = float((plain[k].double().cpu() - ref[k]).abs().max())
        print(f"TransMIL maps torch {k}: max|ref| {float(ref[k].abs().max()):.3e}  error {err:.3e}")
        assert plain[k].shape == (H, 600) and err <= 1e-5                     # the bound tests/test_nystrom_rows_cpu.py holds fp32 torch to
    for s in switches:
        setattr(model, s, True)
    with torch.no_grad():
        want = model(g)[0]
    _reset(calls)
    logits, maps = model.attention_maps(g)
    assert calls["nystrom_attention_rows"] == 2 and calls["nystrom_landmark_values_lse"] == 2, calls   # two layers
    assert calls["nystrom_pinv"] == (2 if "fused_pinv" in switches else 0)
    assert torch.equal(logits, want), "the logits differ from forward's"
    assert sorted(maps) == ["layer1", "layer2"]
    for k in ("layer1", "layer2"):
        assert maps[k].shape == (H, 600)
        _judge(f"TransMIL maps {'+'.join(switches)} {k}", maps[k], plain[k], ref[k], 4)
