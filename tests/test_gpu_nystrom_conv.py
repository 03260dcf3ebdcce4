"""The residual convolution's two gradients on the GPU (moc_nystrom_conv_backward; engine.nystrom_conv_backward;
nystrom.TokenValuesResidual; NystromAttention.fused_conv, TransMIL.fused_conv): the entry alone against float64 autograd of
F.conv2d on the CPU, exact impulses, what it writes, determinism, its composition with moc_nystrom_token_backward, the
layer and the model, and which path a call takes.

The judging rule is that of tests/test_gpu_nystrom_train.py: in the same test torch's fp32 autograd on the GPU and the
fused path are each compared with the float64 evaluation; the fused error may be at most max(f x torch's error, 2^-20 x
max|reference|) and never more than 1e-4 x max(1, max|reference|).  f = 2 for the entry alone, f = 4 for the layer and the
model.  Both errors are printed.

Shapes: a workgroup is one head x 128 tokens and leaves one partial tap sum, so n_pad = 256 (the smallest there is) is two
workgroups a head, 512 four, 2,304 eighteen -- five 512-token ranges of that file's kernels, the last one ragged; tiles are
16 tokens with a 16-row halo on either side, zero outside the sequence, so the impulse rows 0, 15, 16, 255, 256 and 511 sit
at the sequence's ends, either side of a tile's edge and either side of a workgroup's.  The layer and model references are
that file's, computed once for both.

The impulse test expects dv[j] = a w[h, j - r + 16]: dv[j] = sum_t w[t] dout[j - t + 16] with dout nonzero at j - t + 16 = r
only, which tests/test_nystrom_conv_cpu.py checks against float64 autograd of F.conv2d."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

import helpers_baselines as HB
from test_gpu_nystrom_train import _layer, _layer_ref, _logits64, _model, _model_grads, _step, _tokens

pytestmark = pytest.mark.gpu

H, D, M = 8, 64, 256
SCALE = D ** -0.5
ENTRIES = ("nystrom_landmark_values", "nystrom_token_values", "nystrom_pinv", "nystrom_landmark_values_lse",
           "nystrom_landmark_backward", "nystrom_token_backward", "nystrom_conv_backward")


def _judge(what, fused, torch32, ref, f):
    """The rule of the module docstring; prints both errors."""
    ref = ref.double().cpu()
    top = float(ref.abs().max())
    e_torch = float((torch32.double().cpu() - ref).abs().max())
    e_fused = float((fused.double().cpu() - ref).abs().max())
    floor = 2.0 ** -20 * top
    print(f"nystrom conv {what}: max|ref| {top:.3e}  torch fp32 {e_torch:.3e}  fused {e_fused:.3e}  (floor {floor:.3e})")
    assert fused.shape == ref.shape and torch.isfinite(fused).all(), what
    assert e_fused <= max(f * e_torch, floor) and e_fused <= 1e-4 * max(1.0, top), (what, e_fused, e_torch, floor)


@functools.lru_cache(maxsize=None)
def _conv_w(taps):
    """[8, taps] from a seeded layer's res_conv."""
    from moc_amd.nystrom import NystromAttention
    torch.manual_seed(7400 + taps)
    attn = NystromAttention(dim=512, dim_head=D, heads=H, num_landmarks=M, residual_conv_kernel=taps)
    return attn.res_conv.weight.detach().reshape(H, taps).contiguous()


def _conv_autograd(qkv, w, dout):
    """(dv [n_pad, 512], dw [8, taps]) by autograd of the layer's own F.conv2d on qkv's v columns, in the tensors' precision."""
    n_pad, taps = qkv.shape[0], w.shape[1]
    qkv, w = qkv.clone().requires_grad_(True), w.clone().requires_grad_(True)
    v = qkv[:, 1024:].reshape(1, n_pad, H, D).transpose(1, 2)
    out = F.conv2d(v, w.reshape(H, 1, taps, 1), padding=(taps // 2, 0), groups=H)
    out.transpose(1, 2).reshape(n_pad, H * D).backward(dout)
    return qkv.grad[:, 1024:], w.grad


@functools.lru_cache(maxsize=None)
def _case(n_pad, taps, lead_zero=0):
    """(qkv, conv_w, dout) in fp32 and the float64 (dv, dw), all on the CPU."""
    x = _tokens(7000 + n_pad, n_pad)
    x[:, :lead_zero] = 0
    with torch.no_grad():
        qkv = _layer(7001).to_qkv(x)[0].contiguous()
    w, dout = _conv_w(taps), HB.randn(7300 + n_pad, n_pad, H * D)
    return (qkv, w, dout), _conv_autograd(qkv.double(), w.double(), dout.double())


def _run(qkv, w, dout, fill=0.0):
    from moc_amd import engine
    dqkv = torch.full_like(qkv, fill)
    return dqkv, engine.nystrom_conv_backward(qkv, w, dout, dqkv)


CASES = [(256, 33, 0), (512, 33, 0), (2304, 33, 0), (512, 3, 0), (512, 1, 0), (512, 33, 255)]


@pytest.mark.parametrize("n_pad,taps,lead_zero", CASES)
def test_entry_matches_float64_autograd(gpu_device, n_pad, taps, lead_zero):
    cpu, (ref_dv, ref_dw) = _case(n_pad, taps, lead_zero)
    qkv, w, dout = (t.to(gpu_device) for t in cpu)
    keep = [t.clone() for t in (qkv, w, dout)]
    dqkv, dw = _run(qkv, w, dout, fill=7.25)
    assert dw.shape == (H, taps) and dw.dtype == torch.float32
    assert all(torch.equal(a, b) for a, b in zip((qkv, w, dout), keep)), "an input was written"
    assert bool((dqkv[:, :1024] == 7.25).all()), "the q and k columns were written"
    t_dv, t_dw = _conv_autograd(qkv, w, dout)
    what = f"entry n_pad={n_pad} taps={taps} lead_zero={lead_zero}"
    _judge(what + " dv", dqkv[:, 1024:], t_dv, ref_dv, 2)
    _judge(what + " dw", dw, t_dw, ref_dw, 2)


@pytest.mark.parametrize("r", [0, 15, 16, 255, 256, 511])
def test_an_impulse_gives_the_taps_exactly(gpu_device, r):
    n_pad = 512
    (qkv, w, _), _ = _case(n_pad, 33)
    h, d, a = (3 * r + 1) % H, (7 * r + 5) % D, torch.tensor(1.75 if r % 2 else -0.3, dtype=torch.float32)
    dout = torch.zeros(n_pad, H * D)
    dout[r, 64 * h + d] = a
    want_dv, want_dw = torch.zeros(n_pad, H * D), torch.zeros(H, 33)
    for j in range(max(0, r - 16), min(n_pad, r + 17)):
        want_dv[j, 64 * h + d] = a * w[h, j - r + 16]
    for t in range(33):
        if 0 <= r + t - 16 < n_pad:
            want_dw[h, t] = a * qkv[r + t - 16, 1024 + 64 * h + d]
    assert int((want_dv != 0).sum()) == min(n_pad, r + 17) - max(0, r - 16) and int((want_dw != 0).sum()) >= 17
    dqkv, dw = _run(qkv.to(gpu_device), w.to(gpu_device), dout.to(gpu_device))
    assert bool((dqkv[:, 1024:].cpu() == want_dv).all()), "dv is not the reversed tap table at the impulse"
    assert bool((dw.cpu() == want_dw).all()), "dw is not the row of v values around the impulse"
    assert not dqkv[:, :1024].any()


def test_a_zero_gradient_gives_exact_zeros(gpu_device):
    qkv, w, dout = (t.to(gpu_device) for t in _case(512, 33)[0])
    dqkv, dw = _run(qkv, w, torch.zeros_like(dout))
    assert not dqkv.any() and not dw.any()


def test_entry_is_deterministic(gpu_device):
    qkv, w, dout = (t.to(gpu_device) for t in _case(2304, 33)[0])
    (a_dqkv, a_dw), (b_dqkv, b_dw) = _run(qkv, w, dout), _run(qkv, w, dout)
    assert torch.equal(a_dqkv, b_dqkv) and torch.equal(a_dw, b_dw)


@pytest.mark.parametrize("n_pad", [256, 2304])
def test_entry_stays_inside_its_buffers(gpu_device, n_pad):
    from moc_amd import _lib
    dev, h, pad, taps = gpu_device, _lib.lib(), 4096, 33                      # pad: floats (or bytes of the workspace)
    inputs = tuple(t.to(dev) for t in _case(n_pad, taps)[0])
    qkv, w, dout = inputs
    keep = [t.clone() for t in inputs]
    nbytes = h.moc_nystrom_conv_backward_workspace(n_pad, H, D, M, taps)
    assert 0 < nbytes < n_pad * H * D * 4

    def band(numel):
        return torch.full((numel + 2 * pad,), 7.25, dtype=torch.float32, device=dev)

    def inside(t, numel):
        return t[pad:pad + numel]

    def untouched(t, numel):
        return bool((t[:pad] == 7.25).all()) and bool((t[pad + numel:] == 7.25).all())

    ws = torch.full((nbytes + 2 * pad,), 0xA5, dtype=torch.uint8, device=dev)
    dqkv, dw = band(n_pad * 3 * H * D), band(H * taps)
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr() + 4 * pad                                      # noqa: E731
    rc = h.moc_nystrom_conv_backward(qkv.data_ptr(), n_pad, H, D, M, w.data_ptr(), taps, dout.data_ptr(), p(dqkv), p(dw),
                                     ws.data_ptr() + pad, nbytes, None)
    assert rc == 0, h.moc_last_error()
    torch.cuda.synchronize()
    assert bool((ws[:pad] == 0xA5).all()) and bool((ws[pad + nbytes:] == 0xA5).all()), "workspace written out of bounds"
    assert untouched(dqkv, n_pad * 3 * H * D), "dqkv written out of bounds"
    assert untouched(dw, H * taps), "dconv_w written out of bounds"
    assert all(torch.equal(a, b) for a, b in zip(inputs, keep)), "an input was written"
    got = inside(dqkv, n_pad * 3 * H * D).view(n_pad, -1)
    assert bool((got[:, :1024] == 7.25).all()), "the q and k columns were written"
    want_dqkv, want_dw = _run(qkv, w, dout)
    assert torch.equal(got[:, 1024:], want_dqkv[:, 1024:]) and torch.equal(inside(dw, H * taps).view(H, taps), want_dw)


def test_token_values_residual_composes_the_two_backward_entries(gpu_device):
    from moc_amd import engine
    from moc_amd.nystrom import TokenValuesResidual
    n_pad = 512
    qkv, w, dout = (t.to(gpu_device) for t in _case(n_pad, 33)[0])
    k_l = (qkv[:, 512:1024].reshape(M, n_pad // M, H, D).sum(1) / (n_pad // M)).transpose(0, 1).contiguous()
    Y = (HB.randn(7500, H, M, D) * 0.1).to(gpu_device)
    leaves = [t.clone().requires_grad_(True) for t in (qkv, k_l, Y, w)]
    out = TokenValuesResidual.apply(*leaves, SCALE)
    assert torch.equal(out, engine.nystrom_token_values(qkv, k_l, Y, w, SCALE))
    out.backward(dout)
    dqkv_t, dk_l, dY = engine.nystrom_token_backward(qkv, k_l, Y, SCALE, dout)
    dqkv_c, dw = _run(qkv, w, dout)
    got = leaves[0].grad
    assert torch.equal(got[:, :512], dqkv_t[:, :512]) and not got[:, 512:1024].any()
    assert torch.equal(got[:, 1024:], dqkv_c[:, 1024:]) and got[:, 1024:].any()
    assert torch.equal(leaves[1].grad, dk_l) and torch.equal(leaves[2].grad, dY) and torch.equal(leaves[3].grad, dw)


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


@pytest.mark.parametrize("n", [1, 257, 1025])
def test_layer_trains_with_the_fused_residual_and_matches_float64(gpu_device, calls, n):
    dev = gpu_device
    attn, x, G = _layer(8000).to(dev), _tokens(8100 + n, n).to(dev), HB.randn(8200 + n, 1, n, 512).to(dev)
    ref_out, ref = _layer_ref(n, True)
    plain_out, plain = _step(attn, x, G)
    assert not any(calls.values())
    attn.fused = attn.fused_train = attn.fused_conv = True
    got_out, got = _step(attn, x, G)
    assert calls["nystrom_conv_backward"] == 1 and calls["nystrom_token_values"] == 1, calls
    assert calls["nystrom_landmark_values_lse"] == calls["nystrom_landmark_backward"] == calls["nystrom_token_backward"] == 1
    with torch.no_grad():
        assert torch.equal(got_out, attn(x)), "the training forward differs from the no-grad fused forward"
    assert got_out.shape == (1, n, 512) and sorted(got) == sorted(ref) and "res_conv.weight" in got
    assert got["res_conv.weight"].shape == attn.res_conv.weight.shape
    _judge(f"layer n={n} forward", got_out, plain_out, ref_out, 2)
    for k in sorted(ref):
        _judge(f"layer n={n} d{k}", got[k], plain[k], ref[k], 4)


def test_layer_without_a_residual_is_untouched(gpu_device, calls):
    n = 700
    dev = gpu_device
    attn, x, G = _layer(8000, False).to(dev), _tokens(8100 + n, n).to(dev), HB.randn(8200 + n, 1, n, 512).to(dev)
    attn.fused = attn.fused_train = True
    want_out, want = _step(attn, x, G)
    attn.fused_conv = True
    got_out, got = _step(attn, x, G)
    assert calls["nystrom_conv_backward"] == 0 and calls["nystrom_token_backward"] == 2
    assert torch.equal(got_out, want_out) and sorted(got) == sorted(want)
    assert all(torch.equal(got[k], want[k]) for k in want)


def test_which_path_a_call_takes(gpu_device, calls, monkeypatch):
    dev, n = gpu_device, 300
    attn, x, G = _layer(8000).to(dev), _tokens(8100 + n, n).to(dev), HB.randn(8200 + n, 1, n, 512).to(dev)

    def unchanged(xx, gg, **flags):
        """The same call with fused_conv off and on: equal bits, and no call of the new entry."""
        for k, on in flags.items():
            setattr(attn, k, on)
        attn.fused_conv = False
        want_out, want = _step(attn, xx, gg)
        attn.fused_conv = True
        got_out, got = _step(attn, xx, gg)
        return (calls["nystrom_conv_backward"] == 0 and torch.equal(got_out, want_out)
                and all(torch.equal(got[k], want[k]) for k in want))

    assert unchanged(x, G, fused=False, fused_train=False) and not any(calls.values())          # alone: the torch code
    assert unchanged(x, G, fused=True, fused_train=False) and not any(calls.values())           # without fused_train
    assert unchanged(x, G, fused=False, fused_train=True) and not any(calls.values())           # without fused
    wide = torch.zeros(1, n, 520, device=dev)
    wide[:, :, :512] = x
    assert unchanged(wide[:, :, :512], G, fused=True, fused_train=True) and not any(calls.values())   # a non-contiguous x
    with torch.no_grad():                                                                       # no_grad: the fused forward
        attn.fused_conv = False
        want = attn(x)
        attn.fused_conv = True
        assert torch.equal(attn(x), want)
    assert calls["nystrom_conv_backward"] == 0 and calls["nystrom_landmark_values"] == 2 and calls["nystrom_token_values"] == 2
    _reset(calls)

    def boom(*a, **k):
        raise AssertionError("res_conv's own forward was called")
    monkeypatch.setattr(attn.res_conv, "forward", boom)
    _, grads = _step(attn, x, G)                                                                # all three on
    assert calls["nystrom_conv_backward"] == 1 and calls["nystrom_token_values"] == 1 and calls["nystrom_token_backward"] == 1
    assert calls["nystrom_landmark_values"] == 0 and calls["nystrom_pinv"] == 0
    assert all(torch.isfinite(g).all() for g in grads.values()) and grads["res_conv.weight"].any()


# ---------------------------------------------------------------- the model
def test_transmil_trains_with_the_fused_residual_and_matches_float64(gpu_device, calls):
    data = HB.randn(8600, 600, 512)
    m64 = copy.deepcopy(_model()).double()
    ref_logits = _logits64(m64, data.double())
    ref = _model_grads(m64, ref_logits)
    model, g = copy.deepcopy(_model()).to(gpu_device), data.to(gpu_device)
    plain_logits = model(g)[0]
    plain = _model_grads(model, plain_logits)
    assert not any(calls.values())
    model.fused = model.fused_train = model.fused_conv = True
    logits = model(g)[0]
    got = _model_grads(model, logits)
    assert calls["nystrom_conv_backward"] == 2 and calls["nystrom_token_values"] == 2, calls     # once per layer
    assert calls["nystrom_token_backward"] == 2 and calls["nystrom_landmark_backward"] == 2
    _judge("TransMIL logits", logits.detach(), plain_logits.detach(), ref_logits.detach(), 4)
    for k in ("layer1.attn.res_conv.weight", "layer2.attn.res_conv.weight", "layer1.attn.to_qkv.weight", "_fc1.0.weight"):
        _judge(f"TransMIL d{k}", got[k], plain[k], ref[k], 4)
