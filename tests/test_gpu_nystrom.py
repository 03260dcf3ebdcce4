"""The fused Nystrom forward on the GPU (moc_nystrom_landmark_values / moc_nystrom_token_values, engine.nystrom_*,
NystromAttention.forward_fused, TransMIL.fused): each kernel alone, the layer and the model against a float64 evaluation
of the restatement (moc_amd/nystrom.py) on the CPU, determinism, isolation, and which path a call takes.

Tolerances are measured, not chosen (tests/test_gpu_adapter.py): in the same test the torch fp32 path on the GPU and the
fused path are each compared with the float64 evaluation; the fused error may be at most
max(2 x torch's error, 2^-20 x max|reference|) -- twice, for another summation order; the 16-ulp floor for cases where
torch's own error happens to be near zero -- and never more than 1e-4 absolute.  Inputs are LayerNorm'd standard-normal
tokens through a freshly initialised layer, which leave that cap room (torch fp32 against float64: about 5e-7 at the layer
output, 1e-7 at the two products).

Kernel A splits the tokens in ranges of 512 (one workgroup per head and range, merged in index order): n_pad = 256 is one
ragged range, 512 one full range, 2,304 = 4 x 512 + 256 and 4,352 = 8 x 512 + 256 several ranges with a ragged last one.
Kernel B works in tiles of 16 tokens, sixteen tiles to a 256-token workgroup: every n_pad >= 512 crosses both boundaries."""
import copy
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import helpers_baselines as HB

pytestmark = pytest.mark.gpu

CAP = 1e-4
H, D, M, TAPS = 8, 64, 256, 33
SCALE = D ** -0.5
N_PADS = [256, 512, 2304, 4352]


def _judge(what, fused, torch32, ref):
    """The rule of the module docstring; prints both errors."""
    ref = ref.double().cpu()
    e_torch = float((torch32.double().cpu() - ref).abs().max())
    e_fused = float((fused.double().cpu() - ref).abs().max())
    floor = 2.0 ** -20 * float(ref.abs().max())
    print(f"nystrom {what}: torch fp32 {e_torch:.3e}  fused {e_fused:.3e}  (floor {floor:.3e})")
    assert torch.isfinite(fused).all(), what
    assert e_fused <= max(2 * e_torch, floor) and e_fused <= CAP, (what, e_fused, e_torch, floor)


def _layer(seed, residual=True):
    from moc_amd.nystrom import NystromAttention
    torch.manual_seed(seed)
    return NystromAttention(dim=512, dim_head=D, heads=H, num_landmarks=M, pinv_iterations=6, residual=residual,
                            dropout=0.1).eval()


def _tokens(seed, n):
    return F.layer_norm(HB.randn(seed, 1, n, 512), (512,))


@functools.lru_cache(maxsize=None)
def _qkv(n_pad, lead_zero=0):
    """[n_pad, 1536] fp32 on the CPU as to_qkv leaves it; `lead_zero` front-padding (zero) rows."""
    x = _tokens(5000 + n_pad, n_pad)
    x[:, :lead_zero] = 0
    with torch.no_grad():
        return _layer(5001).to_qkv(x)[0].contiguous()


def _heads(qkv, part):
    """q (0), k (1) or v (2) as [8, n, 64]."""
    return qkv[:, 512 * part:512 * (part + 1)].reshape(qkv.shape[0], H, D).transpose(0, 1)


def _means(t):
    """segment means [8, 256, 64] of a [8, n, 64] tensor."""
    return t.reshape(H, M, -1, D).sum(dim=2) / (t.shape[1] // M)


def _top_score(qkv, side):
    """largest |score| of kernel A (landmark queries x keys) or of kernel B (queries x landmark keys), in float64"""
    q, k = _heads(qkv, 0).double() * SCALE, _heads(qkv, 1).double()
    q, k = (_means(q), k) if side == "A" else (q, _means(k))
    return float((q @ k.transpose(1, 2)).abs().max())


def _sharpen(qkv, side, target=100.0):
    """q and k scaled so that the kernel's scores reach +-target (without a maximum subtracted, exp overflows)."""
    top = _top_score(qkv, side)
    out = qkv.clone()
    out[:, :1024] *= (target / top) ** 0.5
    return out


# ---------------------------------------------------------------- kernel A alone
def _landmark_ref(qkv, q_l):
    return (q_l @ _heads(qkv, 1).transpose(1, 2)).softmax(dim=-1) @ _heads(qkv, 2)


A_CASES = [(n, 0, False) for n in N_PADS] + [(512, 255, False), (2304, 255, False), (512, 0, True), (4352, 0, True)]


@pytest.mark.parametrize("n_pad,lead_zero,sharp", A_CASES)
def test_landmark_values_match_float64(gpu_device, n_pad, lead_zero, sharp):
    from moc_amd import engine
    qkv = _qkv(n_pad, lead_zero)
    if sharp:
        qkv = _sharpen(qkv, "A")
        assert 99.0 <= _top_score(qkv, "A") <= 101.0
    q_l = _means(_heads(qkv, 0) * SCALE).contiguous()
    ref = _landmark_ref(qkv.double(), q_l.double())
    g_qkv, g_ql = qkv.to(gpu_device), q_l.to(gpu_device)
    keep = g_qkv.clone()
    got = engine.nystrom_landmark_values(g_qkv, g_ql)
    assert got.shape == (H, M, D) and got.dtype == torch.float32
    assert torch.equal(g_qkv, keep), "qkv was written"
    _judge(f"A n_pad={n_pad} lead_zero={lead_zero} sharp={sharp}", got, _landmark_ref(g_qkv, g_ql), ref)


# ---------------------------------------------------------------- kernel B alone
def _conv_w(kind):
    if kind == "none":
        return None
    if kind == "random":
        return HB.randn(5100, H, TAPS) * TAPS ** -0.5
    w = torch.zeros(H, TAPS)
    w[:, int(kind)] = 1.0                                                     # one-hot: out picks v[i + tap - 16]
    return w


def _token_ref(qkv, k_l, Y, w):
    q, v = _heads(qkv, 0) * SCALE, _heads(qkv, 2)
    out = (q @ k_l.transpose(1, 2)).softmax(dim=-1) @ Y
    if w is not None:
        out = out + F.conv2d(v.unsqueeze(0), w.reshape(H, 1, TAPS, 1), padding=(TAPS // 2, 0), groups=H)[0]
    return out.transpose(0, 1).reshape(qkv.shape[0], H * D)


B_CASES = ([(n, kind, False) for n in N_PADS for kind in ("none", "random")]
           + [(n, tap, False) for n in (256, 512) for tap in ("0", "16", "32")] + [(512, "random", True), (4352, "none", True)])


@pytest.mark.parametrize("n_pad,conv,sharp", B_CASES)
def test_token_values_match_float64(gpu_device, n_pad, conv, sharp):
    from moc_amd import engine
    qkv = _qkv(n_pad)
    if sharp:
        qkv = _sharpen(qkv, "B")
        assert 99.0 <= _top_score(qkv, "B") <= 101.0
    k_l = _means(_heads(qkv, 1)).contiguous()
    Y, w = HB.randn(5200 + n_pad, H, M, D) * 0.1, _conv_w(conv)
    ref = _token_ref(qkv.double(), k_l.double(), Y.double(), None if w is None else w.double())
    dev = gpu_device
    g_qkv, g_kl, g_Y, g_w = qkv.to(dev), k_l.to(dev), Y.to(dev), None if w is None else w.to(dev)
    keep = g_qkv.clone()
    got = engine.nystrom_token_values(g_qkv, g_kl, g_Y, g_w, SCALE)
    assert got.shape == (n_pad, H * D) and got.dtype == torch.float32
    assert torch.equal(g_qkv, keep), "qkv was written"
    _judge(f"B n_pad={n_pad} conv={conv} sharp={sharp}", got, _token_ref(g_qkv, g_kl, g_Y, g_w), ref)


@pytest.mark.parametrize("tap", [0, 16, 32])
def test_one_hot_taps_pick_the_shifted_rows_exactly(gpu_device, tap):
    """With Y = 0 the output IS the convolution: a one-hot tap must return v shifted by tap - 16, zero past either end --
    bit for bit, at the sequence's ends and across the 16-token tiles and 256-token workgroups."""
    from moc_amd import engine
    n_pad = 768
    qkv = _qkv(n_pad).to(gpu_device)
    k_l = _means(_heads(qkv, 1)).contiguous()
    out = engine.nystrom_token_values(qkv, k_l, torch.zeros(H, M, D, device=gpu_device), _conv_w(str(tap)).to(gpu_device), SCALE)
    v, shift = qkv[:, 1024:], tap - TAPS // 2
    want = torch.zeros_like(v)
    lo, hi = max(0, -shift), min(n_pad, n_pad - shift)
    want[lo:hi] = v[lo + shift:hi + shift]
    assert torch.equal(out, want)


# ---------------------------------------------------------------- determinism and isolation
def test_kernels_are_deterministic(gpu_device):
    from moc_amd import engine
    qkv = _qkv(2304).to(gpu_device)
    q_l, k_l = _means(_heads(qkv, 0) * SCALE).contiguous(), _means(_heads(qkv, 1)).contiguous()
    w = _conv_w("random").to(gpu_device)
    a1, a2 = engine.nystrom_landmark_values(qkv, q_l), engine.nystrom_landmark_values(qkv, q_l)
    assert torch.equal(a1, a2)
    b1, b2 = engine.nystrom_token_values(qkv, k_l, a1, w, SCALE), engine.nystrom_token_values(qkv, k_l, a1, w, SCALE)
    assert torch.equal(b1, b2)


@pytest.mark.parametrize("n_pad", [256, 2304])
def test_kernels_stay_inside_their_buffers(gpu_device, n_pad):
    import ctypes
    from moc_amd import _lib, engine
    dev, h, pad = gpu_device, _lib.lib(), 4096
    qkv = _qkv(n_pad).to(dev)
    q_l, k_l = _means(_heads(qkv, 0) * SCALE).contiguous(), _means(_heads(qkv, 1)).contiguous()
    w = _conv_w("random").to(dev)
    keep = qkv.clone()
    nbytes = h.moc_nystrom_workspace(n_pad, H, D, M)
    assert nbytes == ((n_pad + 511) // 512) * H * M * (D + 2) * 4
    ws = torch.full((nbytes + 2 * pad,), 0xA5, dtype=torch.uint8, device=dev)
    W = torch.full((H * M * D + 2 * pad,), 7.25, dtype=torch.float32, device=dev)
    out = torch.full((n_pad * H * D + 2 * pad,), 7.25, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    rc = h.moc_nystrom_landmark_values(qkv.data_ptr(), n_pad, H, D, M, q_l.data_ptr(), W.data_ptr() + 4 * pad,
                                       ws.data_ptr() + pad, nbytes, None)
    assert rc == 0, h.moc_last_error()
    Wv = W[pad:pad + H * M * D].view(H, M, D)
    rc = h.moc_nystrom_token_values(qkv.data_ptr(), n_pad, H, D, M, k_l.data_ptr(), Wv.data_ptr(), w.data_ptr(), TAPS,
                                    ctypes.c_float(SCALE), out.data_ptr() + 4 * pad, None)
    torch.cuda.synchronize()
    assert rc == 0, h.moc_last_error()
    assert bool((ws[:pad] == 0xA5).all()) and bool((ws[pad + nbytes:] == 0xA5).all()), "workspace written out of bounds"
    assert bool((W[:pad] == 7.25).all()) and bool((W[pad + H * M * D:] == 7.25).all()), "W written out of bounds"
    assert bool((out[:pad] == 7.25).all()) and bool((out[pad + n_pad * H * D:] == 7.25).all()), "out written out of bounds"
    assert torch.equal(qkv, keep), "qkv was written"
    assert torch.equal(Wv, engine.nystrom_landmark_values(qkv, q_l))
    assert torch.equal(out[pad:pad + n_pad * H * D].view(n_pad, H * D), engine.nystrom_token_values(qkv, k_l, Wv, w, SCALE))


# ---------------------------------------------------------------- the layer
@pytest.fixture
def kernel_calls(monkeypatch):
    from moc_amd import engine
    calls = []
    for name in ("nystrom_landmark_values", "nystrom_token_values"):
        real = getattr(engine, name)
        monkeypatch.setattr(engine, name, lambda *a, _real=real, **k: (calls.append(1), _real(*a, **k))[1])
    return calls


@functools.lru_cache(maxsize=None)
def _layer_ref(n, residual):
    with torch.no_grad():
        return copy.deepcopy(_layer(6000, residual)).double()(_tokens(6100 + n, n).double())


@pytest.mark.parametrize("n,residual", [(n, True) for n in (1, 255, 256, 257, 513, 1025, 4100)] + [(700, False)])
def test_layer_fused_matches_float64(gpu_device, kernel_calls, n, residual):
    attn, x = _layer(6000, residual).to(gpu_device), _tokens(6100 + n, n).to(gpu_device)
    with torch.no_grad():
        plain = attn(x)
        assert not kernel_calls
        attn.fused = True
        got = attn(x)
    assert len(kernel_calls) == 2, "forward_fused did not reach both kernels"
    assert got.shape == plain.shape == (1, n, 512)
    _judge(f"layer n={n} residual={residual}", got, plain, _layer_ref(n, residual))


def test_layer_takes_the_torch_path_where_a_gradient_is_wanted(gpu_device, kernel_calls):
    attn, x = _layer(6000).to(gpu_device), _tokens(6100 + 257, 257).to(gpu_device)
    plain = attn(x)
    attn.fused = True
    got = attn(x)                                                             # gradient mode, parameters require grad
    assert not kernel_calls and got.grad_fn is not None and torch.equal(got, plain)
    for p in attn.parameters():
        p.requires_grad_(False)
    got = attn(x.clone().requires_grad_(True))                                # only the input wants one
    assert not kernel_calls and got.grad_fn is not None and torch.equal(got, plain)
    with torch.no_grad():
        for p in attn.parameters():
            p.requires_grad_(True)
        fused = attn(x)
    assert len(kernel_calls) >= 1 and fused.grad_fn is None
    assert float((fused - plain.detach()).abs().max()) < CAP


def test_layer_falls_back_where_the_kernels_do_not_apply(gpu_device, kernel_calls):
    from moc_amd.nystrom import NystromAttention
    dev = gpu_device
    attn, x = _layer(6000).to(dev), _tokens(6100 + 300, 300).to(dev)
    plain_attn = copy.deepcopy(attn)
    attn.fused = True
    wide = torch.zeros(1, 300, 520, device=dev)
    wide[:, :, :512] = x
    with torch.no_grad():
        two = torch.cat([x, x.flip(1)])
        assert torch.equal(attn(two), plain_attn(two))                        # batch 2
        assert torch.equal(attn(wide[:, :, :512]), plain_attn(wide[:, :, :512]))          # not contiguous
        assert torch.equal(attn.double()(x.double()), plain_attn.double()(x.double()))    # float64
        torch.manual_seed(1)
        other = NystromAttention(dim=512, dim_head=64, heads=8, num_landmarks=128).to(dev).eval()      # 128 landmarks
        want = other(x)
        other.fused = True
        assert torch.equal(other(x), want)
    assert not kernel_calls


# ---------------------------------------------------------------- the model
@functools.lru_cache(maxsize=None)
def _model():
    from moc_amd.model_mil import TransMIL
    torch.manual_seed(6500)
    return TransMIL(n_classes=3, size_arg="conch").eval()


def _model64(model, data):
    """(logits, Y_prob, patch-level logits) of a float64 copy: TransMIL.forward / forward_patch_level restated without
    their `data.float()` (models/model_mil.py:236-266)."""
    m = copy.deepcopy(model).double()
    h = m._fc1(data.double().unsqueeze(0))
    n = h.shape[1]
    side = int(math.ceil(math.sqrt(n)))
    h = torch.cat([h, h[:, :side * side - n]], dim=1)
    h = torch.cat((m.cls_token.expand(1, -1, -1), h), dim=1)
    h = m.layer2(m.pos_layer(m.layer1(h), side, side))
    logits = m._fc2(m.norm(h)[:, 0])
    return logits, F.softmax(logits, dim=1), m._fc2(h).squeeze(0)[1:n + 1]


@pytest.mark.parametrize("rows", [600, 3000])
def test_transmil_fused_matches_float64(gpu_device, kernel_calls, rows):
    data = HB.randn(6600 + rows, rows, 512)
    with torch.no_grad():
        ref_logits, ref_prob, ref_rows = _model64(_model(), data)
        model, g = copy.deepcopy(_model()).to(gpu_device), data.to(gpu_device)
        plain, plain_rows = model(g), model.forward_patch_level(g)
        assert not kernel_calls
        model.fused = True
        got, got_rows = model(g), model.forward_patch_level(g)
    assert len(kernel_calls) == 8                                             # two layers x two kernels x two passes
    _judge(f"TransMIL rows={rows} logits", got[0], plain[0], ref_logits)
    _judge(f"TransMIL rows={rows} Y_prob", got[1], plain[1], ref_prob)
    _judge(f"TransMIL rows={rows} patch level", got_rows, plain_rows, ref_rows)
    assert got_rows.shape == (rows, 3)
    assert torch.equal(got[2], plain[2]) and got[3] is None and got[4] is None
