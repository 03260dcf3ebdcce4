"""The gradient through the landmark pseudo-inverse on the GPU (moc_nystrom_pinv_iterates, moc_nystrom_pinv_backward;
engine.nystrom_pinv_iterates / nystrom_pinv_backward; nystrom.LandmarkPinv; NystromAttention.fused_pinv_train,
TransMIL.fused_pinv_train): the entry alone against float64 autograd of moore_penrose_iter_pinv on the CPU, tied maxima,
exactness and hygiene, the layer and the model, and which path a call takes.  One shape: 8 heads x 256 landmarks.

The judging rule is that of tests/test_gpu_nystrom_train.py: in the same test torch's fp32 autograd on the GPU and the
fused path are each compared with the float64 evaluation; the fused error may be at most max(f x torch's error, 2^-20 x
max|reference|) and never more than 1e-4 x max(1, max|reference|).  f = 2 for the entry, f = 4 for the layer and the model.
Both errors are printed.

Why the inputs need care: the rows of a softmax matrix all sum to 1 within an ulp, so WHICH rows tie at the maximal sum c
differs with the precision and the summation order (on the layer's attn2 at n = 257: 5 rows for torch's fp32 sum on the
CPU, 7 in the kernel's order, 1 in float64), and the share of dden r that a row receives with it.  That difference is
constant along a row, and the softmax backward that follows in the layer removes it.  So two kinds of input:
  * gapped -- one row scaled by 1.25 and the maximal column of another head scaled by 1.25, so that both maxima lead by
    1e-3 (relative) or more in fp32 and in float64 (asserted) -- with the whole dA compared;
  * softmax matrices as the layer makes them, with each path's dA turned (on the CPU, in float64, with the same X) into
    dS = X o (dA - sum_j dA o X) first; the column maximum must lead by 1e-5 at the same place in both precisions (asserted).
The tie test copies the gapped input's maximal row into another head and its maximal column beside it: two rows and two
columns tie exactly in every precision, each gets half; bound max(4 R max|ref|, 2^-20 max|ref|) with R torch's relative
error on the untied twin at the same iteration count."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

import helpers_baselines as HB
from test_gpu_nystrom_train import _layer, _layer_ref, _logits64, _model, _model_grads, _step, _tokens

pytestmark = pytest.mark.gpu

H, M = 8, 256
NEW_ENTRIES = ("nystrom_pinv_iterates", "nystrom_pinv_backward")
ENTRIES = NEW_ENTRIES + ("nystrom_landmark_values", "nystrom_token_values", "nystrom_pinv", "nystrom_landmark_values_lse",
                         "nystrom_landmark_backward", "nystrom_token_backward", "nystrom_conv_backward")


def _errors(what, fused, torch32, ref):
    ref = ref.double().cpu()
    top = float(ref.abs().max())
    e_torch = float((torch32.double().cpu() - ref).abs().max())
    e_fused = float((fused.double().cpu() - ref).abs().max())
    floor = 2.0 ** -20 * top
    print(f"nystrom pinv bwd {what}: max|ref| {top:.3e}  torch fp32 {e_torch:.3e}  fused {e_fused:.3e}  (floor {floor:.3e})")
    assert fused.shape == ref.shape and torch.isfinite(fused).all(), what
    return top, e_torch, e_fused, floor


def _judge(what, fused, torch32, ref, f):
    """The rule of the module docstring; prints both errors."""
    top, e_torch, e_fused, floor = _errors(what, fused, torch32, ref)
    assert e_fused <= max(f * e_torch, floor) and e_fused <= 1e-4 * max(1.0, top), (what, e_fused, e_torch, floor)


def _autograd(X, dZ, iters):
    """d X of moore_penrose_iter_pinv by torch autograd, in X's precision and on its device."""
    from moc_amd.nystrom import moore_penrose_iter_pinv
    leaf = X.clone().requires_grad_(True)
    moore_penrose_iter_pinv(leaf, iters).backward(dZ)
    return leaf.grad


def _sums(X):
    return X.abs().sum(dim=-1).reshape(-1), X.abs().sum(dim=-2).reshape(-1)   # "col" (over j), "row" (over i), all heads


def _lead(s):
    """(argmax, relative lead of the maximum over the runner-up)."""
    top2 = torch.topk(s.double(), 2)
    return int(top2.indices[0]), float((top2.values[0] - top2.values[1]) / top2.values[0])


# ---------------------------------------------------------------- inputs, once per case
@functools.lru_cache(maxsize=None)
def _gapped(kind):
    """[8, 256, 256] fp32 on the CPU with both maxima leading: row 5 of one head x 1.25, the maximal column (of another
    head) x 1.25."""
    X = HB.randn(9800, H, M, M)
    X = X.softmax(dim=-1) if kind == "softmax" else X / 16 + torch.eye(M)
    at = int(_sums(X)[1].argmax())
    hc, jc = at // M, at % M
    hr = (hc + 1) % H
    X[hc, :, jc] *= 1.25
    X[hr, 5] *= 1.25
    for Y in (X, X.double()):
        col, row = _sums(Y)
        assert _lead(col)[0] == hr * M + 5 and _lead(col)[1] >= 1e-3
        assert _lead(row)[0] == hc * M + jc and _lead(row)[1] >= 1e-3
    return X.contiguous(), (hr, 5), (hc, jc)


@functools.lru_cache(maxsize=None)
def _tied():
    """_gapped("softmax") with its maximal row copied into another head and its maximal column copied beside it."""
    X, (hr, i), (hc, j) = _gapped("softmax")
    X = X.clone()
    X[hc, :, (j + 7) % M] = X[hc, :, j]
    X[(hr + 2) % H, 9] = X[hr, i]
    for Y in (X, X.double()):
        col, row = _sums(Y)
        assert int((col == col.max()).sum()) == 2 and int((row == row.max()).sum()) == 2
        assert sorted(torch.nonzero(col == col.max()).flatten().tolist()) == sorted([hr * M + i, ((hr + 2) % H) * M + 9])
        assert sorted(torch.nonzero(row == row.max()).flatten().tolist()) == sorted([hc * M + j, hc * M + (j + 7) % M])
    return X.contiguous()


def _dz(iters):
    return HB.randn(9900 + iters, H, M, M)


@functools.lru_cache(maxsize=None)
def _ref(kind, iters):
    """float64 autograd on the CPU."""
    X = _tied() if kind == "tied" else _soft(kind) if kind.startswith("layer") or kind == "sharp" else _gapped(kind)[0]
    return _autograd(X.double(), _dz(iters).double(), iters)


@functools.lru_cache(maxsize=None)
def _soft(kind):
    """Softmax matrices as the layer makes them: softmax(3 randn), or the layer's own attn2 at n = 257 / 1,025."""
    if kind == "sharp":
        return (3 * HB.randn(9810, H, M, M)).softmax(dim=-1).contiguous()
    n = int(kind[len("layer"):])
    attn = _layer(8000)
    x = _tokens(8100 + n, n)
    with torch.no_grad():
        x = F.pad(x, (0, 0, M - (n % M), 0), value=0)
        qkv = attn.to_qkv(x)[0]
        n_pad, inner = qkv.shape[0], qkv.shape[1] // 3
        means = qkv[:, :2 * inner].reshape(M, n_pad // M, 2 * inner).sum(dim=1) / (n_pad // M)
        q_l = (means[:, :inner] * attn.scale).reshape(M, H, -1).transpose(0, 1)
        k_l = means[:, inner:].reshape(M, H, -1).transpose(0, 1)
        return (q_l @ k_l.transpose(-1, -2)).softmax(dim=-1).contiguous()


def _run(X, dZ, iters, dev):
    from moc_amd import engine
    gX, gdZ = X.to(dev), dZ.to(dev)
    Zs = engine.nystrom_pinv_iterates(gX, iters)
    return gX, gdZ, Zs, engine.nystrom_pinv_backward(gX, Zs, gdZ, iters)


# ---------------------------------------------------------------- the entry
@pytest.mark.parametrize("kind", ["softmax", "signed"])
@pytest.mark.parametrize("iters", [0, 1, 2, 6])
def test_backward_matches_float64_autograd_on_gapped_inputs(gpu_device, kind, iters):
    X, dZ = _gapped(kind)[0], _dz(iters)
    gX, gdZ, Zs, dA = _run(X, dZ, iters, gpu_device)
    assert Zs.shape == (iters + 1, H, M, M) and dA.shape == (H, M, M) and dA.dtype == torch.float32
    _judge(f"{kind} iters={iters} dA", dA, _autograd(gX, gdZ, iters), _ref(kind, iters), 2)


@pytest.mark.parametrize("kind", ["sharp", "layer257", "layer1025"])
def test_backward_matches_float64_autograd_through_the_softmax(gpu_device, kind):
    iters = 6
    X, dZ = _soft(kind), _dz(iters)
    (a32, lead32), (a64, lead64) = _lead(_sums(X)[1]), _lead(_sums(X.double())[1])
    print(f"nystrom pinv bwd {kind}: column maximum leads by {lead32:.2e} (fp32) {lead64:.2e} (float64)")
    assert a32 == a64 and lead32 >= 1e-5 and lead64 >= 1e-5
    gX, gdZ, _, dA = _run(X, dZ, iters, gpu_device)
    X64 = X.double()

    def through(d):
        d = d.double().cpu()
        return X64 * (d - (d * X64).sum(dim=-1, keepdim=True))
    _judge(f"{kind} iters={iters} dS", through(dA), through(_autograd(gX, gdZ, iters)), through(_ref(kind, iters)), 2)


@pytest.mark.parametrize("iters", [0, 1])
def test_tied_maxima_share_evenly(gpu_device, iters):
    dZ = _dz(iters)
    gX, gdZ, _, dA = _run(_gapped("softmax")[0], dZ, iters, gpu_device)
    top, e_torch, _, _ = _errors(f"untied twin iters={iters}", dA, _autograd(gX, gdZ, iters), _ref("softmax", iters))
    R = e_torch / top
    ref = _ref("tied", iters)
    gX, gdZ, _, dA = _run(_tied(), dZ, iters, gpu_device)
    top, _, e_fused, floor = _errors(f"tied iters={iters}", dA, _autograd(gX, gdZ, iters), ref)
    assert e_fused <= max(4 * R * top, floor), (e_fused, R, top)


# ---------------------------------------------------------------- exactness and hygiene
@pytest.mark.parametrize("iters", [0, 1, 6, 9])
def test_the_last_iterate_is_the_forward_entrys_result(gpu_device, iters):
    from moc_amd import engine
    X = _soft("layer257").to(gpu_device)
    Zs = engine.nystrom_pinv_iterates(X, iters)
    assert Zs.shape == (iters + 1, H, M, M) and torch.equal(Zs[iters], engine.nystrom_pinv(X, iters))
    for t in range(iters):                                                    # and every earlier one is the forward stopped there
        assert torch.equal(Zs[t], engine.nystrom_pinv(X, t)), t


def test_zero_gradient_determinism_and_what_is_written(gpu_device):
    from moc_amd import _lib, engine
    iters = 2
    gX, gdZ, Zs, dA = _run(_gapped("signed")[0], _dz(iters), iters, gpu_device)
    keep = [t.clone() for t in (gX, gdZ, Zs)]
    assert not engine.nystrom_pinv_backward(gX, Zs, torch.zeros_like(gdZ), iters).any(), "a zero dZ must give exact zeros"
    assert not engine.nystrom_pinv_backward(gX, Zs[:1].clone(), torch.zeros_like(gdZ), 0).any()
    assert torch.equal(engine.nystrom_pinv_backward(gX, Zs, gdZ, iters), dA), "two calls differ"
    assert torch.equal(engine.nystrom_pinv_iterates(gX, iters), Zs)
    # the C entry on a pre-filled dA inside a guard band, a workspace inside one too
    h, pad = _lib.lib(), 4096
    need = h.moc_nystrom_pinv_backward_workspace(H, M)
    out = torch.full((H * M * M + 2 * pad,), 7.25, dtype=torch.float32, device=gpu_device)
    ws = torch.full((need + 2 * pad,), 0xA5, dtype=torch.uint8, device=gpu_device)
    torch.cuda.synchronize()
    rc = h.moc_nystrom_pinv_backward(gX.data_ptr(), H, M, iters, Zs.data_ptr(), gdZ.data_ptr(), out.data_ptr() + 4 * pad,
                                     ws.data_ptr() + pad, need, None)
    assert rc == 0, h.moc_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out[pad:pad + H * M * M].view(H, M, M), dA), "a pre-filled dA is not fully overwritten"
    assert bool((out[:pad] == 7.25).all()) and bool((out[pad + H * M * M:] == 7.25).all()), "dA written out of bounds"
    assert bool((ws[:pad] == 0xA5).all()) and bool((ws[pad + need:] == 0xA5).all()), "workspace written out of bounds"
    assert all(torch.equal(a, b) for a, b in zip((gX, gdZ, Zs), keep)), "an input was written"


def test_the_entries_work_on_another_stream(gpu_device):
    from moc_amd import engine
    iters = 2
    gX, gdZ, Zs, dA = _run(_gapped("signed")[0], _dz(iters), iters, gpu_device)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=gpu_device)
    with torch.cuda.stream(side):
        Zs2 = engine.nystrom_pinv_iterates(gX, iters)
        dA2 = engine.nystrom_pinv_backward(gX, Zs2, gdZ, iters)
    side.synchronize()
    assert torch.equal(Zs2, Zs) and torch.equal(dA2, dA)


# ---------------------------------------------------------------- the layer, the model
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


def _all_on(m):
    m.fused = m.fused_train = m.fused_conv = m.fused_pinv_train = True


@pytest.mark.parametrize("n", [257, 1025])
def test_layer_trains_with_the_fused_pinv_and_matches_float64(gpu_device, calls, n):
    dev = gpu_device
    attn, x, G = _layer(8000).to(dev), _tokens(8100 + n, n).to(dev), HB.randn(8200 + n, 1, n, 512).to(dev)
    ref_out, ref = _layer_ref(n, True)
    plain_out, plain = _step(attn, x, G)
    assert not any(calls.values())
    _all_on(attn)
    got_out, got = _step(attn, x, G)
    assert calls["nystrom_pinv_iterates"] == 1 and calls["nystrom_pinv_backward"] == 1 and calls["nystrom_pinv"] == 0, calls
    assert calls["nystrom_conv_backward"] == calls["nystrom_token_backward"] == calls["nystrom_landmark_backward"] == 1
    assert got_out.shape == (1, n, 512) and sorted(got) == sorted(ref)
    _judge(f"layer n={n} forward", got_out, plain_out, ref_out, 4)
    for k in ("x", "to_qkv.weight", "res_conv.weight"):
        _judge(f"layer n={n} d{k}", got[k], plain[k], ref[k], 4)


def test_transmil_trains_with_the_fused_pinv_and_matches_float64(gpu_device, calls):
    data = HB.randn(8600, 600, 512)
    m64 = copy.deepcopy(_model()).double()
    ref_logits = _logits64(m64, data.double())
    ref = _model_grads(m64, ref_logits)
    model, g = copy.deepcopy(_model()).to(gpu_device), data.to(gpu_device)
    plain_logits = model(g)[0]
    plain = _model_grads(model, plain_logits)
    assert not any(calls.values())
    _all_on(model)
    logits = model(g)[0]
    got = _model_grads(model, logits)
    assert calls["nystrom_pinv_iterates"] == 2 and calls["nystrom_pinv_backward"] == 2 and calls["nystrom_pinv"] == 0, calls
    _judge("TransMIL logits", logits.detach(), plain_logits.detach(), ref_logits.detach(), 4)
    for k in ("layer1.attn.res_conv.weight", "layer2.attn.res_conv.weight", "layer1.attn.to_qkv.weight", "_fc1.0.weight"):
        _judge(f"TransMIL d{k}", got[k], plain[k], ref[k], 4)


def test_which_path_a_call_takes(gpu_device, calls):
    from moc_amd.nystrom import NystromAttention
    dev, n = gpu_device, 300
    attn, x, G = _layer(8000).to(dev), _tokens(8100 + n, n).to(dev), HB.randn(8200 + n, 1, n, 512).to(dev)

    def unchanged(a, xx, gg, **flags):
        """The same call with fused_pinv_train off and on: equal bits, and no call of the new entries."""
        for k, on in flags.items():
            setattr(a, k, on)
        a.fused_pinv_train = False
        want_out, want = _step(a, xx, gg)
        a.fused_pinv_train = True
        got_out, got = _step(a, xx, gg)
        return (not any(calls[k] for k in NEW_ENTRIES) and torch.equal(got_out, want_out)
                and all(torch.equal(got[k], want[k]) for k in want))

    assert unchanged(attn, x, G, fused=False, fused_train=False, fused_conv=False) and not any(calls.values())   # alone
    assert unchanged(attn, x, G, fused=True, fused_train=False, fused_conv=True) and not any(calls.values())     # no fused_train
    assert unchanged(attn, x, G, fused=False, fused_train=True, fused_conv=True) and not any(calls.values())     # no fused
    _all_on(attn)
    _step(attn, x, G)                                                         # all on, gradient mode
    assert calls["nystrom_pinv_iterates"] == 1 and calls["nystrom_pinv_backward"] == 1 and calls["nystrom_pinv"] == 0
    assert calls["nystrom_landmark_values_lse"] == 1 and calls["nystrom_landmark_values"] == 0
    _reset(calls)
    attn.fused_pinv = True
    with torch.no_grad():                                                     # no_grad: the forward's entries only
        attn.fused_pinv_train = False
        want = attn(x)
        attn.fused_pinv_train = True
        assert torch.equal(attn(x), want)
    assert not any(calls[k] for k in NEW_ENTRIES) and calls["nystrom_pinv"] == 2
    assert calls["nystrom_landmark_values"] == 2 and calls["nystrom_token_values"] == 2
    assert not any(calls[k] for k in ("nystrom_landmark_values_lse", "nystrom_landmark_backward", "nystrom_token_backward",
                                      "nystrom_conv_backward"))
    attn.fused_pinv = False
    _reset(calls)

    # shapes the kernels are not built for: the torch path, bit for bit
    plain_attn = copy.deepcopy(attn)
    plain_attn.fused = plain_attn.fused_train = plain_attn.fused_conv = plain_attn.fused_pinv_train = False
    two, G2 = torch.cat([x, x.flip(1)]), torch.cat([G, G])
    torch.manual_seed(1)
    other = NystromAttention(dim=512, dim_head=64, heads=8, num_landmarks=128).to(dev).eval()
    plain_other = copy.deepcopy(other)
    _all_on(other)
    for a, b, xx, gg in ((attn, plain_attn, two, G2),
                         (copy.deepcopy(attn).double(), copy.deepcopy(plain_attn).double(), x.double(), G.double()),
                         (other, plain_other, x, G)):
        (out_a, grads_a), (out_b, grads_b) = _step(a, xx, gg), _step(b, xx, gg)
        assert torch.equal(out_a, out_b) and all(torch.equal(grads_a[k], grads_b[k]) for k in grads_b)
    assert not any(calls.values())
