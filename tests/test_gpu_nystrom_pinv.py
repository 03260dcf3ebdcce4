"""The landmark pseudo-inverse on the GPU (moc_nystrom_pinv, engine.nystrom_pinv, NystromAttention.fused_pinv,
TransMIL.fused_pinv).  One shape, [8, 256, 256] fp32 (2 MiB a matrix).

1. Exact, without a tolerance.  A[h] = s_h P_h with a different permutation matrix per head: every product then has ONE
   non-zero term per output, both maxima of the absolute sums are exactly 1 (s_0 = 1), and Z[h] = a_h P_h^T where a_h
   follows the scalar recurrence in numpy float32, op by op.  The kernels and torch's function must both return exactly
   that matrix -- which catches a transposition, tile or head indexing, the three diagonal constants, the buffer
   ping-pong, and a reciprocal multiply where the init divides.
2. Against the float64 iteration on the CPU, with torch's own fp32 function on the same GPU as the yardstick:
   e_kernel <= max(4 e_torch, 4 R max|ref|, 2^-20 max|ref|), R the largest e_torch / max|ref| over the cases of the same
   iteration count, and e_kernel <= 1e-4 max|ref| in any case.  The kernels differ from torch only in summation order;
   two fp32 evaluations that differ only in that (a library GEMM against k in steps of four, on the CPU, these inputs) had
   errors up to 6x apart within one case and 2.03x apart pooled, at relative errors of 1e-7 to 1.2e-5: the factor 4 is
   twice the pooled spread.  An indexing error gives O(1) relative error, four orders of magnitude above the cap.
3. Isolation and determinism: canaries around Z and the workspace, A unchanged, two calls the same bits, the raw entry
   equal to the wrapper.
4. The layer and the model with `fused = fused_pinv = True` against their float64 copies (the plain torch path as the
   yardstick, the same factor, floor and cap), and which calls reach the wrapper at all."""
import copy
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers_baselines as HB

pytestmark = pytest.mark.gpu

H, D, M = 8, 64, 256
S = np.array([1, 0.5, 0.8125, 0.3, 0.9999, 0.062, 0.7, 0.45], dtype=np.float32)


def _torch_pinv(x, iters):
    from moc_amd.nystrom import moore_penrose_iter_pinv
    return moore_penrose_iter_pinv(x.unsqueeze(0), iters)[0]


# ---------------------------------------------------------------- 1. exact
def _recurrence(s, iters):
    """a_h after `iters` iterations, numpy float32, one rounding per operation."""
    f = np.float32
    a = s / (f(1) * f(1))
    for _ in range(iters):
        xz = s * a
        t = f(7) - xz
        t = xz * t
        t = f(15) - t
        t = xz * t
        t = f(13) - t
        a = (f(0.25) * a) * t
    assert a.dtype == np.float32
    return a


@functools.lru_cache(maxsize=None)
def _perms():
    g = torch.Generator().manual_seed(7100)
    return torch.stack([torch.randperm(M, generator=g) for _ in range(H)])


def _scaled_perms(order):
    """(A [8, 256, 256] with A[k] = s_h P_h for h = order[k], the per-head scale and permutation in that order)"""
    perm, s = _perms()[order], torch.from_numpy(S)[order]
    A = torch.zeros(H, M, M)
    A[torch.arange(H)[:, None], torch.arange(M)[None, :], perm] = s[:, None].expand(H, M)
    return A, s.numpy(), perm


def _expected(s, perm, iters):
    a = torch.from_numpy(_recurrence(s, iters))
    Z = torch.zeros(H, M, M)
    Z[torch.arange(H)[:, None], perm, torch.arange(M)[None, :]] = a[:, None].expand(H, M)       # a_h P_h^T
    return Z


@pytest.mark.parametrize("iters", [0, 1, 2, 6, 9])
def test_scaled_permutations_give_the_scalar_recurrence_exactly(gpu_device, iters):
    from moc_amd import engine
    fwd, rev = list(range(H)), list(range(H))[::-1]
    A, s, perm = _scaled_perms(fwd)
    assert len({tuple(p.tolist()) for p in perm}) == H and not torch.equal(perm[0], torch.arange(M))
    want = _expected(s, perm, iters)
    g = A.to(gpu_device)
    got = engine.nystrom_pinv(g, iters)
    assert got.shape == (H, M, M) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), want), f"kernel, iters={iters}: {int((got.cpu() != want).sum())} elements differ"
    assert torch.equal(_torch_pinv(g, iters).cpu(), want), f"torch, iters={iters}"
    # the heads in reversed order (head 0's scale is then 0.45; the maxima are still 1, from the last head)
    Ar, sr, permr = _scaled_perms(rev)
    assert torch.equal(Ar, A.flip(0))
    got_r = engine.nystrom_pinv(Ar.to(gpu_device), iters)
    assert torch.equal(got_r.cpu(), _expected(sr, permr, iters)) and torch.equal(got_r, got.flip(0))


# ---------------------------------------------------------------- 2. against float64
def _layer(seed, residual=True, landmarks=M):
    from moc_amd.nystrom import NystromAttention
    torch.manual_seed(seed)
    return NystromAttention(dim=512, dim_head=D, heads=H, num_landmarks=landmarks, pinv_iterations=6, residual=residual,
                            dropout=0.1).eval()


def _tokens(seed, n):
    return F.layer_norm(HB.randn(seed, 1, n, 512), (512,))


def _layer_attn2(n, sharpen=1.0):
    """attn2 [8, 256, 256] of the test layer on n tokens, as forward_fused forms it (CPU, fp32); q_l times `sharpen`."""
    attn, x = _layer(6000), _tokens(6100 + n, n)
    if n % M > 0:
        x = F.pad(x, (0, 0, M - (n % M), 0), value=0)
    with torch.no_grad():
        qkv = attn.to_qkv(x)[0]
        l = qkv.shape[0] // M
        means = qkv[:, :1024].reshape(M, l, 1024).sum(dim=1) / l
        q_l = (means[:, :512] * attn.scale).reshape(M, H, D).transpose(0, 1) * sharpen
        k_l = means[:, 512:].reshape(M, H, D).transpose(0, 1)
        return (q_l @ k_l.transpose(-1, -2)).softmax(dim=-1).contiguous()


CASES = {
    "layer n=257": lambda: _layer_attn2(257),
    "layer n=1025": lambda: _layer_attn2(1025),
    "layer n=4100": lambda: _layer_attn2(4100),
    "layer n=4100 sharp": lambda: _layer_attn2(4100, sharpen=30.0),
    "layer n=256": lambda: _layer_attn2(256),
    "softmax(3 randn)": lambda: (3 * HB.randn(7200, H, M, M)).softmax(dim=-1),
    "softmax(20 I + randn)": lambda: (20 * torch.eye(M) + HB.randn(7201, H, M, M)).softmax(dim=-1),
}


@functools.lru_cache(maxsize=None)
def _inputs():
    return {name: make().float().contiguous() for name, make in CASES.items()}


@functools.lru_cache(maxsize=None)
def _errors(iters, dev):
    """{case: (e_torch, e_kernel, max|ref|)} for every case at this iteration count, computed once."""
    from moc_amd import engine
    out = {}
    for name, x in _inputs().items():
        ref = _torch_pinv(x.double(), iters)
        g = x.to(dev)
        keep = g.clone()
        got = engine.nystrom_pinv(g, iters)
        assert torch.equal(g, keep), "attn2 was written"
        assert torch.isfinite(got).all(), name
        out[name] = (float((_torch_pinv(g, iters).double().cpu() - ref).abs().max()),
                     float((got.double().cpu() - ref).abs().max()), float(ref.abs().max()))
    return out


@pytest.mark.parametrize("iters", [1, 6])
@pytest.mark.parametrize("case", list(CASES))
def test_pinv_matches_float64(gpu_device, case, iters):
    table = _errors(iters, str(gpu_device))
    R = max(e_t / top for e_t, _, top in table.values())
    e_torch, e_kernel, top = table[case]
    bound = max(4 * e_torch, 4 * R * top, 2.0 ** -20 * top)
    print(f"pinv {case} iters={iters}: torch fp32 {e_torch:.3e}  kernel {e_kernel:.3e}  max|ref| {top:.3e}  (R {R:.3e}, bound {bound:.3e})")
    assert e_kernel <= bound and e_kernel <= 1e-4 * top, (case, iters, e_kernel, e_torch, R, top)


# ---------------------------------------------------------------- 3. isolation and determinism
def test_pinv_stays_inside_its_buffers_and_is_deterministic(gpu_device):
    from moc_amd import _lib, engine
    dev, h, pad = gpu_device, _lib.lib(), 4096
    A = _inputs()["layer n=1025"].to(dev)
    keep = A.clone()
    nbytes = h.moc_nystrom_pinv_workspace(H, M)
    assert nbytes >= 5 * H * M * M * 4
    for iters in (0, 1, 6):                                           # the init writes Z itself, the last product from either Z buffer
        ws = torch.full((nbytes + 2 * pad,), 0xA5, dtype=torch.uint8, device=dev)
        Z = torch.full((H * M * M + 2 * pad,), 7.25, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        rc = h.moc_nystrom_pinv(A.data_ptr(), H, M, iters, Z.data_ptr() + 4 * pad, ws.data_ptr() + pad, nbytes, None)
        torch.cuda.synchronize()
        assert rc == 0, h.moc_last_error()
        assert bool((ws[:pad] == 0xA5).all()) and bool((ws[pad + nbytes:] == 0xA5).all()), "workspace written out of bounds"
        assert bool((Z[:pad] == 7.25).all()) and bool((Z[pad + H * M * M:] == 7.25).all()), "Z written out of bounds"
        assert torch.equal(A, keep), "A was written"
        Zv = Z[pad:pad + H * M * M].view(H, M, M)
        first, second = engine.nystrom_pinv(A, iters), engine.nystrom_pinv(A, iters)
        assert torch.equal(first, second) and torch.equal(Zv, first)
    assert torch.equal(A, keep)


# ---------------------------------------------------------------- 4. the layer and the model
CAP = 1e-4


def _judge(what, fused, torch32, ref):
    """_judge of tests/test_gpu_nystrom.py with the factor 4 of section 2; the cap both absolute and relative to max|ref|."""
    ref = ref.double().cpu()
    e_torch = float((torch32.double().cpu() - ref).abs().max())
    e_fused = float((fused.double().cpu() - ref).abs().max())
    top = float(ref.abs().max())
    floor = 2.0 ** -20 * top
    print(f"nystrom pinv {what}: torch fp32 {e_torch:.3e}  fused + fused_pinv {e_fused:.3e}  (floor {floor:.3e}, max|ref| {top:.3e})")
    assert torch.isfinite(fused).all(), what
    assert e_fused <= max(4 * e_torch, floor) and e_fused <= CAP * min(1.0, top), (what, e_fused, e_torch, floor)


@pytest.fixture
def pinv_calls(monkeypatch):
    from moc_amd import engine
    calls = []
    real = engine.nystrom_pinv
    monkeypatch.setattr(engine, "nystrom_pinv", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


@functools.lru_cache(maxsize=None)
def _layer_ref(n):
    with torch.no_grad():
        return copy.deepcopy(_layer(6000)).double()(_tokens(6100 + n, n).double())


@pytest.mark.parametrize("n", [1, 257, 1025, 4100])
def test_layer_with_fused_pinv_matches_float64(gpu_device, pinv_calls, n):
    attn, x = _layer(6000).to(gpu_device), _tokens(6100 + n, n).to(gpu_device)
    with torch.no_grad():
        plain = attn(x)
        attn.fused = True
        attn(x)
        assert not pinv_calls
        attn.fused_pinv = True
        got = attn(x)
    assert len(pinv_calls) == 1, "one pseudo-inverse per layer forward"
    assert got.shape == plain.shape == (1, n, 512)
    _judge(f"layer n={n}", got, plain, _layer_ref(n))


def test_fused_pinv_alone_in_gradient_mode_and_for_other_layers_calls_nothing(gpu_device, pinv_calls):
    dev = gpu_device
    attn, x = _layer(6000).to(dev), _tokens(6100 + 257, 257).to(dev)
    with torch.no_grad():
        plain = attn(x)
        attn.fused_pinv = True                                                # without `fused`: the plain path, bit for bit
        assert torch.equal(attn(x), plain)
    attn.fused = True
    got = attn(x)                                                             # gradient mode, parameters require grad
    assert got.grad_fn is not None and torch.equal(got.detach(), plain)
    with torch.no_grad():
        other = _layer(1, landmarks=128).to(dev)                              # 128 landmarks
        want = other(x)
        other.fused = other.fused_pinv = True
        assert torch.equal(other(x), want)
    assert not pinv_calls
    with torch.no_grad():
        attn(x)
    assert len(pinv_calls) == 1


def _model64(model, data):
    """(logits, Y_prob) of a float64 copy: TransMIL.forward restated without its `data.float()`."""
    m = copy.deepcopy(model).double()
    h = m._fc1(data.double().unsqueeze(0))
    n = h.shape[1]
    side = int(math.ceil(math.sqrt(n)))
    h = torch.cat([h, h[:, :side * side - n]], dim=1)
    h = torch.cat((m.cls_token.expand(1, -1, -1), h), dim=1)
    h = m.layer2(m.pos_layer(m.layer1(h), side, side))
    logits = m._fc2(m.norm(h)[:, 0])
    return logits, F.softmax(logits, dim=1)


def test_transmil_with_fused_pinv_matches_float64(gpu_device, pinv_calls):
    from moc_amd.model_mil import TransMIL
    rows = 600
    torch.manual_seed(6500)
    cpu_model = TransMIL(n_classes=3, size_arg="conch").eval()
    data = HB.randn(6600 + rows, rows, 512)
    with torch.no_grad():
        ref_logits, ref_prob = _model64(cpu_model, data)
        model, g = copy.deepcopy(cpu_model).to(gpu_device), data.to(gpu_device)
        plain = model(g)
        model.fused_pinv = True
        assert all(torch.equal(a, b) for a, b in zip(model(g)[:3], plain[:3]))            # without `fused`: nothing
        model.fused = True
        assert not pinv_calls
        got = model(g)
    assert len(pinv_calls) == 2                                               # one per layer
    _judge(f"TransMIL rows={rows} logits", got[0], plain[0], ref_logits)
    _judge(f"TransMIL rows={rows} Y_prob", got[1], plain[1], ref_prob)
    assert got[3] is None and got[4] is None
