"""Training on the fused Nystrom products (moc_nystrom_landmark_values_lse, moc_nystrom_landmark_backward,
moc_nystrom_token_backward; engine.nystrom_*; nystrom.LandmarkValues / TokenValues; NystromAttention.fused_train,
TransMIL.fused_train): each entry alone, the layer and the model against float64 autograd of the restatement
(moc_amd/nystrom.py) on the CPU, determinism, isolation, which path a call takes, and the peak memory of a step.

Tolerances are measured, not chosen -- the rule of tests/test_gpu_nystrom.py, made relative because gradient magnitudes
vary: in the same test torch's fp32 autograd on the GPU and the fused path are each compared with the float64 evaluation;
the fused error may be at most max(f x torch's error, 2^-20 x max|reference|) and never more than 1e-4 x max(1,
max|reference|).  f = 2 for a kernel alone (one reordered summation chain), f = 4 for the layer and the model (two
reordered chains that feed the shared pseudo-inverse backward).  Both errors are printed.

Shapes as in tests/test_gpu_nystrom.py: the landmark-parallel kernels split the tokens in ranges of 512, so n_pad = 256
is one ragged range, 512 one full range, 2,304 = 4 x 512 + 256 several ranges and a ragged last one; the token-parallel
kernels work in 16-token tiles, sixteen to a 256-token workgroup."""
import copy
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import helpers_baselines as HB

pytestmark = pytest.mark.gpu

H, D, M = 8, 64, 256
SCALE = D ** -0.5


def _judge(what, fused, torch32, ref, f):
    """The rule of the module docstring; prints both errors."""
    ref = ref.double().cpu()
    top = float(ref.abs().max())
    e_torch = float((torch32.double().cpu() - ref).abs().max())
    e_fused = float((fused.double().cpu() - ref).abs().max())
    floor = 2.0 ** -20 * top
    print(f"nystrom train {what}: max|ref| {top:.3e}  torch fp32 {e_torch:.3e}  fused {e_fused:.3e}  (floor {floor:.3e})")
    assert fused.shape == ref.shape and torch.isfinite(fused).all(), what
    assert e_fused <= max(f * e_torch, floor) and e_fused <= 1e-4 * max(1.0, top), (what, e_fused, e_torch, floor)


def _layer(seed, residual=True):
    from moc_amd.nystrom import NystromAttention
    torch.manual_seed(seed)
    return NystromAttention(dim=512, dim_head=D, heads=H, num_landmarks=M, pinv_iterations=6, residual=residual,
                            dropout=0.1).eval()


def _tokens(seed, n):
    return F.layer_norm(HB.randn(seed, 1, n, 512), (512,))


def _heads(qkv, part):
    """q (0), k (1) or v (2) as [8, n, 64]."""
    return qkv[:, 512 * part:512 * (part + 1)].reshape(qkv.shape[0], H, D).transpose(0, 1)


def _means(t):
    return t.reshape(H, M, -1, D).sum(dim=2) / (t.shape[1] // M)


def _top_score(qkv, side):
    q, k = _heads(qkv, 0).double() * SCALE, _heads(qkv, 1).double()
    q, k = (_means(q), k) if side == "A" else (q, _means(k))
    return float((q @ k.transpose(1, 2)).abs().max())


@functools.lru_cache(maxsize=None)
def _qkv(n_pad, lead_zero=0, sharp=None):
    """[n_pad, 1536] fp32 on the CPU as to_qkv leaves it; `lead_zero` front-padding (zero) rows; `sharp` = "A" / "B": q and k
    scaled so that that side's scores reach +-100 (without a subtracted maximum, exp overflows)."""
    x = _tokens(7000 + n_pad, n_pad)
    x[:, :lead_zero] = 0
    with torch.no_grad():
        qkv = _layer(7001).to_qkv(x)[0].contiguous()
    if sharp:
        qkv[:, :1024] *= (100.0 / _top_score(qkv, sharp)) ** 0.5
        assert 99.0 <= _top_score(qkv, sharp) <= 101.0
    return qkv


# ---------------------------------------------------------------- the landmark side: references, once per case
def _landmark_fwd(qkv, q_l):
    return (q_l @ _heads(qkv, 1).transpose(1, 2)).softmax(dim=-1) @ _heads(qkv, 2)


def _landmark_autograd(qkv, q_l, dW):
    qkv, q_l = qkv.clone().requires_grad_(True), q_l.clone().requires_grad_(True)
    _landmark_fwd(qkv, q_l).backward(dW)
    return qkv.grad, q_l.grad


@functools.lru_cache(maxsize=None)
def _landmark_case(n_pad, lead_zero, sharp):
    """(qkv, q_l, dW) in fp32 and the float64 (lse, dqkv, dq_l), all on the CPU."""
    qkv = _qkv(n_pad, lead_zero, "A" if sharp else None)
    q_l = _means(_heads(qkv, 0) * SCALE).contiguous()
    dW = HB.randn(7100 + n_pad, H, M, D)
    lse = torch.logsumexp(q_l.double() @ _heads(qkv.double(), 1).transpose(1, 2), dim=-1)
    return (qkv, q_l, dW), (lse,) + _landmark_autograd(qkv.double(), q_l.double(), dW.double())


L_CASES = [(256, 0, False), (512, 0, False), (2304, 0, False), (512, 255, False), (512, 0, True)]


@pytest.mark.parametrize("n_pad,sharp", [(256, False), (512, False), (2304, False), (512, True)])
def test_lse_entry_keeps_the_forward_bits_and_matches_float64(gpu_device, n_pad, sharp):
    from moc_amd import engine
    (qkv, q_l, _), (ref_lse, _, _) = _landmark_case(n_pad, 0, sharp)
    g_qkv, g_ql = qkv.to(gpu_device), q_l.to(gpu_device)
    keep = g_qkv.clone()
    W, lse = engine.nystrom_landmark_values_lse(g_qkv, g_ql)
    assert torch.equal(W, engine.nystrom_landmark_values(g_qkv, g_ql)), "W differs from the entry without lse"
    assert lse.shape == (H, M) and lse.dtype == torch.float32 and torch.equal(g_qkv, keep)
    torch32 = torch.logsumexp(g_ql @ _heads(g_qkv, 1).transpose(1, 2), dim=-1)
    _judge(f"lse n_pad={n_pad} sharp={sharp}", lse, torch32, ref_lse, 2)


@pytest.mark.parametrize("n_pad,lead_zero,sharp", L_CASES)
def test_landmark_backward_matches_float64_autograd(gpu_device, n_pad, lead_zero, sharp):
    from moc_amd import engine
    (qkv, q_l, dW), (_, ref_dqkv, ref_dql) = _landmark_case(n_pad, lead_zero, sharp)
    g_qkv, g_ql, g_dW = qkv.to(gpu_device), q_l.to(gpu_device), dW.to(gpu_device)
    keep = [t.clone() for t in (g_qkv, g_ql, g_dW)]
    W, lse = engine.nystrom_landmark_values_lse(g_qkv, g_ql)
    dqkv, dq_l = engine.nystrom_landmark_backward(g_qkv, g_ql, W, lse, g_dW)
    assert dqkv.shape == (n_pad, 3 * H * D) and dq_l.shape == (H, M, D)
    assert all(torch.equal(a, b) for a, b in zip((g_qkv, g_ql, g_dW), keep)), "an input was written"
    assert not dqkv[:, :512].any(), "the q columns must be exact zeros"
    t_dqkv, t_dql = _landmark_autograd(g_qkv, g_ql, g_dW)
    what = f"landmark backward n_pad={n_pad} lead_zero={lead_zero} sharp={sharp}"
    _judge(what + " dk", dqkv[:, 512:1024], t_dqkv[:, 512:1024], ref_dqkv[:, 512:1024], 2)
    _judge(what + " dv", dqkv[:, 1024:], t_dqkv[:, 1024:], ref_dqkv[:, 1024:], 2)
    _judge(what + " dq_l", dq_l, t_dql, ref_dql, 2)


# ---------------------------------------------------------------- the token side
def _token_fwd(qkv, k_l, Y):
    out = ((_heads(qkv, 0) * SCALE) @ k_l.transpose(1, 2)).softmax(dim=-1) @ Y
    return out.transpose(0, 1).reshape(qkv.shape[0], H * D)


def _token_autograd(qkv, k_l, Y, dout):
    qkv, k_l, Y = (t.clone().requires_grad_(True) for t in (qkv, k_l, Y))
    _token_fwd(qkv, k_l, Y).backward(dout)
    return qkv.grad, k_l.grad, Y.grad


@functools.lru_cache(maxsize=None)
def _token_case(n_pad, sharp):
    qkv = _qkv(n_pad, 0, "B" if sharp else None)
    k_l = _means(_heads(qkv, 1)).contiguous()
    Y, dout = HB.randn(7200 + n_pad, H, M, D) * 0.1, HB.randn(7300 + n_pad, n_pad, H * D)
    return (qkv, k_l, Y, dout), _token_autograd(qkv.double(), k_l.double(), Y.double(), dout.double())


@pytest.mark.parametrize("n_pad,sharp", [(256, False), (512, False), (2304, False), (512, True)])
def test_token_backward_matches_float64_autograd(gpu_device, n_pad, sharp):
    from moc_amd import engine
    cpu, (ref_dqkv, ref_dkl, ref_dY) = _token_case(n_pad, sharp)
    g_qkv, g_kl, g_Y, g_dout = (t.to(gpu_device) for t in cpu)
    keep = [t.clone() for t in (g_qkv, g_kl, g_Y, g_dout)]
    dqkv, dk_l, dY = engine.nystrom_token_backward(g_qkv, g_kl, g_Y, SCALE, g_dout)
    assert dqkv.shape == (n_pad, 3 * H * D) and dk_l.shape == dY.shape == (H, M, D)
    assert all(torch.equal(a, b) for a, b in zip((g_qkv, g_kl, g_Y, g_dout), keep)), "an input was written"
    assert not dqkv[:, 512:].any(), "the k and v columns must be exact zeros"
    t_dqkv, t_dkl, t_dY = _token_autograd(g_qkv, g_kl, g_Y, g_dout)
    what = f"token backward n_pad={n_pad} sharp={sharp}"
    _judge(what + " dq", dqkv[:, :512], t_dqkv[:, :512], ref_dqkv[:, :512], 2)
    _judge(what + " dk_l", dk_l, t_dkl, ref_dkl, 2)
    _judge(what + " dY", dY, t_dY, ref_dY, 2)


def test_token_backward_of_a_zero_gradient_is_exactly_zero(gpu_device):
    from moc_amd import engine
    qkv, k_l, Y, dout = (t.to(gpu_device) for t in _token_case(512, False)[0])
    for t in engine.nystrom_token_backward(qkv, k_l, Y, SCALE, torch.zeros_like(dout)):
        assert not t.any()


# ---------------------------------------------------------------- determinism and isolation
def test_backward_entries_are_deterministic(gpu_device):
    from moc_amd import engine
    qkv, q_l, dW = (t.to(gpu_device) for t in _landmark_case(2304, 0, False)[0])
    W, lse = engine.nystrom_landmark_values_lse(qkv, q_l)
    a, b = engine.nystrom_landmark_backward(qkv, q_l, W, lse, dW), engine.nystrom_landmark_backward(qkv, q_l, W, lse, dW)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    qkv, k_l, Y, dout = (t.to(gpu_device) for t in _token_case(2304, False)[0])
    a, b = engine.nystrom_token_backward(qkv, k_l, Y, SCALE, dout), engine.nystrom_token_backward(qkv, k_l, Y, SCALE, dout)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("n_pad", [256, 2304])
def test_backward_kernels_stay_inside_their_buffers(gpu_device, n_pad):
    from moc_amd import _lib, engine
    dev, h, pad = gpu_device, _lib.lib(), 4096                                # pad: floats (or bytes of the workspaces)
    qkv, q_l, dW = (t.to(dev) for t in _landmark_case(n_pad, 0, False)[0])
    _, k_l, Y, dout = (t.to(dev) for t in _token_case(n_pad, False)[0])
    tq = _token_case(n_pad, False)[0][0].to(dev)
    inputs = (qkv, q_l, dW, tq, k_l, Y, dout)
    keep = [t.clone() for t in inputs]
    fwd_bytes, bwd_bytes = h.moc_nystrom_workspace(n_pad, H, D, M), h.moc_nystrom_backward_workspace(n_pad, H, D, M)
    assert 0 < bwd_bytes < H * n_pad * M * 4

    def band(numel):
        return torch.full((numel + 2 * pad,), 7.25, dtype=torch.float32, device=dev)

    def inside(t, numel):
        return t[pad:pad + numel]

    def untouched(t, numel):
        return bool((t[:pad] == 7.25).all()) and bool((t[pad + numel:] == 7.25).all())

    ws_f = torch.full((fwd_bytes + 2 * pad,), 0xA5, dtype=torch.uint8, device=dev)
    ws_b = torch.full((bwd_bytes + 2 * pad,), 0xA5, dtype=torch.uint8, device=dev)
    W, lse = band(H * M * D), band(H * M)
    dqkv_l, dqkv_t, dq_l, dk_l, dY = band(n_pad * 3 * H * D), band(n_pad * 3 * H * D), band(H * M * D), band(H * M * D), band(H * M * D)
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr() + 4 * pad                                      # noqa: E731
    rc = h.moc_nystrom_landmark_values_lse(qkv.data_ptr(), n_pad, H, D, M, q_l.data_ptr(), p(W), p(lse), ws_f.data_ptr() + pad,
                                           fwd_bytes, None)
    assert rc == 0, h.moc_last_error()
    rc = h.moc_nystrom_landmark_backward(qkv.data_ptr(), n_pad, H, D, M, q_l.data_ptr(), p(W), p(lse), dW.data_ptr(), p(dqkv_l),
                                         p(dq_l), ws_b.data_ptr() + pad, bwd_bytes, None)
    assert rc == 0, h.moc_last_error()
    torch.cuda.synchronize()
    assert bool((ws_b[:pad] == 0xA5).all()) and bool((ws_b[pad + bwd_bytes:] == 0xA5).all()), "workspace written out of bounds"
    rc = h.moc_nystrom_token_backward(tq.data_ptr(), n_pad, H, D, M, k_l.data_ptr(), Y.data_ptr(), ctypes.c_float(SCALE),
                                      dout.data_ptr(), p(dqkv_t), p(dk_l), p(dY), ws_b.data_ptr() + pad, bwd_bytes, None)
    assert rc == 0, h.moc_last_error()
    torch.cuda.synchronize()
    assert bool((ws_f[:pad] == 0xA5).all()) and bool((ws_f[pad + fwd_bytes:] == 0xA5).all()), "forward workspace out of bounds"
    assert bool((ws_b[:pad] == 0xA5).all()) and bool((ws_b[pad + bwd_bytes:] == 0xA5).all()), "workspace written out of bounds"
    for name, t, numel in (("W", W, H * M * D), ("lse", lse, H * M), ("dqkv (landmark)", dqkv_l, n_pad * 3 * H * D),
                           ("dqkv (token)", dqkv_t, n_pad * 3 * H * D), ("dq_l", dq_l, H * M * D), ("dk_l", dk_l, H * M * D),
                           ("dY", dY, H * M * D)):
        assert untouched(t, numel), f"{name} written out of bounds"
    assert all(torch.equal(a, b) for a, b in zip(inputs, keep)), "an input was written"
    Wv, lv = inside(W, H * M * D).view(H, M, D), inside(lse, H * M).view(H, M)
    want = engine.nystrom_landmark_backward(qkv, q_l, Wv, lv, dW)
    assert torch.equal(inside(dqkv_l, n_pad * 3 * H * D).view(n_pad, -1), want[0])
    assert torch.equal(inside(dq_l, H * M * D).view(H, M, D), want[1])
    want = engine.nystrom_token_backward(tq, k_l, Y, SCALE, dout)
    assert torch.equal(inside(dqkv_t, n_pad * 3 * H * D).view(n_pad, -1), want[0])
    assert torch.equal(inside(dk_l, H * M * D).view(H, M, D), want[1]) and torch.equal(inside(dY, H * M * D).view(H, M, D), want[2])


# ---------------------------------------------------------------- the layer
TRAIN_ENTRIES = ("nystrom_landmark_values_lse", "nystrom_landmark_backward", "nystrom_token_backward")
OTHER_ENTRIES = ("nystrom_landmark_values", "nystrom_token_values", "nystrom_pinv")


@pytest.fixture
def calls(monkeypatch):
    from moc_amd import engine
    seen = {}
    for name in TRAIN_ENTRIES + OTHER_ENTRIES:
        real = getattr(engine, name)
        seen[name] = 0

        def counted(*a, _real=real, _name=name, **k):
            seen[_name] += 1
            return _real(*a, **k)
        monkeypatch.setattr(engine, name, counted)
    return seen


def _step(attn, x, G):
    """(output, {name: gradient}) of sum(attn(x) * G) with respect to x and every parameter."""
    attn.zero_grad(set_to_none=True)
    x = x.detach().requires_grad_(True)                                       # (keeps the strides of a non-contiguous x)
    out = attn(x)
    (out * G).sum().backward()
    grads = {"x": x.grad}
    grads.update({k: p.grad.clone() for k, p in attn.named_parameters()})
    return out.detach(), grads


@functools.lru_cache(maxsize=None)
def _layer_ref(n, residual):
    return _step(copy.deepcopy(_layer(8000, residual)).double(), _tokens(8100 + n, n).double(), HB.randn(8200 + n, 1, n, 512).double())


@pytest.mark.parametrize("n,residual", [(1, True), (257, True), (1025, True), (700, False)])
def test_layer_trains_on_the_kernels_and_matches_float64(gpu_device, calls, n, residual):
    dev = gpu_device
    attn, x, G = _layer(8000, residual).to(dev), _tokens(8100 + n, n).to(dev), HB.randn(8200 + n, 1, n, 512).to(dev)
    ref_out, ref = _layer_ref(n, residual)
    plain_out, plain = _step(attn, x, G)
    assert not any(calls.values())
    attn.fused = attn.fused_train = True
    got_out, got = _step(attn, x, G)
    assert [calls[k] for k in TRAIN_ENTRIES] == [1, 1, 1] and calls["nystrom_token_values"] == 1, calls
    assert calls["nystrom_landmark_values"] == 0 and calls["nystrom_pinv"] == 0
    assert got_out.shape == (1, n, 512) and sorted(got) == sorted(ref)
    _judge(f"layer n={n} residual={residual} forward", got_out, plain_out, ref_out, 2)
    for k in sorted(ref):
        _judge(f"layer n={n} residual={residual} d{k}", got[k], plain[k], ref[k], 4)


def test_which_path_a_call_takes(gpu_device, calls):
    from moc_amd.nystrom import NystromAttention
    dev = gpu_device
    attn, x, G = _layer(8000).to(dev), _tokens(8100 + 300, 300).to(dev), HB.randn(8200 + 300, 1, 300, 512).to(dev)
    plain_out, plain = _step(attn, x, G)

    def same(a):
        out, grads = _step(a, x, G)
        return torch.equal(out, plain_out) and all(torch.equal(grads[k], plain[k]) for k in plain)

    attn.fused_train = True                                                   # without `fused`: the torch code
    assert same(attn) and not any(calls.values())
    attn.fused_train, attn.fused = False, True                                # `fused` alone in grad mode: the torch code
    assert same(attn) and not any(calls.values())
    with torch.no_grad():                                                     # no_grad: fused_train changes nothing
        fused_only = attn(x)
        attn.fused_train = True
        assert torch.equal(attn(x), fused_only)
    assert calls["nystrom_landmark_values"] == 2 and calls["nystrom_token_values"] == 2
    assert not any(calls[k] for k in TRAIN_ENTRIES)
    for k in calls:
        calls[k] = 0

    # shapes the kernels are not built for take the torch code in grad mode too, bit for bit
    plain_attn = copy.deepcopy(attn)
    plain_attn.fused = plain_attn.fused_train = False
    two, G2 = torch.cat([x, x.flip(1)]), torch.cat([G, G])
    wide = torch.zeros(1, 300, 520, device=dev)
    wide[:, :, :512] = x
    torch.manual_seed(1)
    other = NystromAttention(dim=512, dim_head=64, heads=8, num_landmarks=128).to(dev).eval()
    plain_other = copy.deepcopy(other)
    other.fused = other.fused_train = True
    for a, b, xx, gg in ((attn, plain_attn, two, G2), (attn, plain_attn, wide[:, :, :512], G),
                         (copy.deepcopy(attn).double(), copy.deepcopy(plain_attn).double(), x.double(), G.double()),
                         (other, plain_other, x, G)):
        (out_a, grads_a), (out_b, grads_b) = _step(a, xx, gg), _step(b, xx, gg)
        assert torch.equal(out_a, out_b) and all(torch.equal(grads_a[k], grads_b[k]) for k in grads_b)
    assert not any(calls.values())

    attn.fused_pinv = True                                                    # its kernel forms no gradient: ignored here
    _, grads = _step(attn, x, G)
    assert calls["nystrom_pinv"] == 0 and [calls[k] for k in TRAIN_ENTRIES] == [1, 1, 1]
    assert all(torch.isfinite(g).all() for g in grads.values())


# ---------------------------------------------------------------- the model
@functools.lru_cache(maxsize=None)
def _model():
    from moc_amd.model_mil import TransMIL
    torch.manual_seed(8500)
    return TransMIL(n_classes=3, size_arg="conch").eval()


def _logits64(m, data):
    """TransMIL.forward's logits restated without its `data.float()` (models/model_mil.py:236-253), for a float64 copy."""
    h = m._fc1(data.unsqueeze(0))
    n = h.shape[1]
    side = int(math.ceil(math.sqrt(n)))
    h = torch.cat([h, h[:, :side * side - n]], dim=1)
    h = torch.cat((m.cls_token.expand(1, -1, -1), h), dim=1)
    h = m.layer2(m.pos_layer(m.layer1(h), side, side))
    return m._fc2(m.norm(h)[:, 0])


def _model_grads(model, logits):
    model.zero_grad(set_to_none=True)
    F.cross_entropy(logits, torch.tensor([1], device=logits.device)).backward()
    return {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


def test_transmil_trains_on_the_kernels_and_matches_float64(gpu_device, calls):
    data = HB.randn(8600, 600, 512)
    m64 = copy.deepcopy(_model()).double()
    ref = _model_grads(m64, _logits64(m64, data.double()))
    model, g = copy.deepcopy(_model()).to(gpu_device), data.to(gpu_device)
    plain = _model_grads(model, model(g)[0])
    assert not any(calls.values())
    model.fused = model.fused_train = True
    got = _model_grads(model, model(g)[0])
    assert [calls[k] for k in TRAIN_ENTRIES] == [2, 2, 2], calls                 # two layers
    assert sorted(got) == sorted(ref) == sorted(plain) and len(ref) > 10
    for k in sorted(ref):
        _judge(f"TransMIL d{k}", got[k], plain[k], ref[k], 4)

    model.train()                                                             # dropout draws: no comparison
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    opt.zero_grad(set_to_none=True)
    loss = F.cross_entropy(model(g)[0], torch.tensor([1], device=gpu_device))
    loss.backward()
    assert math.isfinite(float(loss)) and [calls[k] for k in TRAIN_ENTRIES] == [4, 4, 4]
    for k, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    opt.step()
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert any(not torch.equal(p.detach(), before[k]) for k, p in model.named_parameters())


# ---------------------------------------------------------------- memory
def test_a_fused_training_step_peaks_below_the_torch_path(gpu_device, calls):
    """Torch keeps at least three tensors of a score matrix's size per layer (6,144 floats per token); the fused path's
    extras are two qkv gradients and the workspace (under 4,400)."""
    n = 4352
    attn, x, G = _layer(8000).to(gpu_device), _tokens(8100 + n, n).to(gpu_device), HB.randn(8200 + n, 1, n, 512).to(gpu_device)

    def peak():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        _step(attn, x, G)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    torch_peak = peak()
    attn.fused = attn.fused_train = True
    fused_peak = peak()
    print(f"nystrom train peak memory n={n}: torch {torch_peak / 2**20:.1f} MiB  fused {fused_peak / 2**20:.1f} MiB")
    assert [calls[k] for k in TRAIN_ENTRIES] == [1, 1, 1]
    assert fused_peak < torch_peak
