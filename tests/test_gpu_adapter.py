"""The fused adapter forward on the GPU (moc_adapter_logits, engine.adapter_logits, forward_fused of Conch_CLIP_Ada /
Conch_MOE_CLIP_Ada): row logits against float64, the reference's fixtures, gradients against dense float64 autograd,
determinism / isolation, and the absence of dense intermediates.

Tolerances are measured, not chosen: in the same test the module's own torch fp32 path on the GPU is compared with the
float64 evaluation, and the fused path is allowed twice that error (another summation order), never more than the
project's 1e-4."""
import contextlib
import copy
import ctypes
import io

import numpy as np
import pytest
import torch

import helpers as H
import helpers_baselines as HB

pytestmark = pytest.mark.gpu

CAP = 1e-4


def _unit(v):
    return v / v.norm(dim=-1, keepdim=True)


def _classifier(seed, C):
    return _unit(HB.randn(seed, C, 512)).t().contiguous()                    # [512, C], unit columns


def _build(E, C, seed, topj=10, router=False):
    import moc_amd.model_adapters as A
    torch.manual_seed(seed)
    cls = _classifier(seed + 1, C)
    if E == 1:
        return A.Conch_CLIP_Ada(num_classes=C, classifier_tensor=cls, topj=topj)
    rt = HB.randn(seed + 2, 512, E) * 0.05 if router else None
    return A.Conch_MOE_CLIP_Ada(ada_num=E, topj=topj, classifier_tensor=cls, router_tensor=rt)


def _experts(model):
    if hasattr(model, "adapter"):
        return [model.adapter]
    return [getattr(model, f"adapter_{i}") for i in range(model.ada_num)]


def _formulas(model, x):
    """Row logits [N, C] by the formulas of the kernel's contract, on the module's own layers (any dtype / device)."""
    nets, r, Wc = _experts(model), model.clip_ratio, model.classifier
    if len(nets) == 1:
        return _unit(nets[0](x) * r + x * (1 - r)) @ Wc
    f = _unit(x)
    w = torch.softmax(model.ada_router.gate(f), dim=-1)
    s = _unit(sum(w[:, e:e + 1] * nets[e](f) for e in range(len(nets))))
    return _unit(s * r + f * (1 - r)) @ Wc


def _to(model, device=None, dtype=None):
    m = copy.deepcopy(model).to(device=device, dtype=dtype)
    m.classifier = model.classifier.to(device=device, dtype=dtype)
    return m


def _kernel_logits(model, x):
    from moc_amd import engine
    nets = _experts(model)
    gate = model.ada_router.gate.weight if len(nets) > 1 else None
    return engine.adapter_logits(x, [n[0].weight for n in nets], [n[2].weight for n in nets], gate, model.classifier,
                                 model.clip_ratio)


# N: one row, below / at / one past a 64-row workgroup, ragged tails, several workgroups; C: 2, odd, 30, the limit;
# E: clip mode and two to eight experts; rows off the unit sphere (x 3) and on it
ROW_CASES = [(1, 2, 1, 3.0), (6, 3, 2, 1.0), (63, 2, 5, 3.0), (64, 30, 1, 1.0), (65, 64, 3, 3.0), (257, 3, 8, 1.0),
             (1000, 2, 1, 3.0), (1000, 30, 2, 0.0), (4097, 2, 5, 3.0), (4097, 64, 1, 0.0)]


@pytest.mark.parametrize("N,C,E,scale", ROW_CASES)
def test_row_logits_match_float64(gpu_device, N, C, E, scale):
    dev = torch.device("cuda:0")
    model = _build(E, C, 7000 + N + C + E)
    x = HB.randn(7100 + N, N, 512)
    x = _unit(x) if scale == 0.0 else x * scale                               # scale 0.0 stands for unit rows
    with torch.no_grad():
        ref = _formulas(_to(model, dtype=torch.float64), x.double())
        gm = _to(model, device=dev)
        xg = x.to(dev)
        e_torch = float((_formulas(gm, xg).double().cpu() - ref).abs().max())
        got = _kernel_logits(gm, xg)
    assert got.shape == (N, C) and got.dtype == torch.float32
    e_kernel = float((got.double().cpu() - ref).abs().max())
    print(f"adapter row logits N={N} C={C} E={E} scale={scale}: torch fp32 {e_torch:.3e}  kernel {e_kernel:.3e}")
    assert e_kernel <= min(2 * e_torch, CAP), (e_kernel, e_torch)


def test_zero_row_gives_nan_as_torch_does(gpu_device):
    dev = torch.device("cuda:0")
    for E in (1, 3):
        model = _to(_build(E, 2, 7300 + E), device=dev)
        x = HB.randn(7301, 70, 512).to(dev)
        x[5] = 0
        with torch.no_grad():
            ref, got = _formulas(model, x), _kernel_logits(model, x)
        assert torch.isnan(ref[5]).all() and torch.isnan(got[5]).all()
        assert torch.isfinite(got[:5]).all() and torch.isfinite(got[6:]).all()


# ---------------------------------------------------------------- the reference's own outputs and gradients
def _fixture_run(name, fused, counter=None):
    import moc_amd.model_adapters as A
    i = [c[0] for c in HB.BASELINE_CASES].index(name)
    _, kind, kw, N, label = HB.BASELINE_CASES[i]
    seed = 4000 + 17 * i
    dev = torch.device("cuda:0")
    with contextlib.redirect_stdout(io.StringIO()):
        cls, kwargs = HB.build_case(A, kind, kw, seed, device=dev)
        model = cls(**kwargs).to(dev)
        model.fused = fused
        return HB.run_case(model, kind, N, label, seed, device=dev)


@pytest.fixture
def kernel_calls(monkeypatch):
    from moc_amd import engine
    calls, real = [], engine.adapter_logits
    monkeypatch.setattr(engine, "adapter_logits", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


@pytest.mark.parametrize("name", ["clip", "clip_short", "moe", "moe_router"])
def test_fused_forward_matches_reference_fixtures(gpu_device, kernel_calls, name):
    got = _fixture_run(name, True)
    assert len(kernel_calls) == 1, "forward_fused did not reach the kernel"
    HB.check_case(got, H.golden("baselines"), name, atol=5e-5)


def test_fused_switch_gate_falls_back_bit_for_bit(gpu_device, kernel_calls):
    a, b = _fixture_run("moe_switch", False), _fixture_run("moe_switch", True)
    assert not kernel_calls
    assert a.keys() == b.keys()
    for k in a:
        assert (np.asarray(a[k]) == np.asarray(b[k])).all(), k


def test_fused_falls_back_where_the_kernel_does_not_apply(gpu_device, kernel_calls):
    dev = torch.device("cuda:0")
    model = _to(_build(1, 2, 7400), device=dev)
    model.fused = True
    x = HB.randn(7401, 90, 512).to(dev)
    big = HB.randn(7402, 90, 516).to(dev)
    plain = copy.deepcopy(model)
    plain.classifier, plain.fused = model.classifier, False
    for feat in (x.clone().requires_grad_(True), x.half(), big[:, :512], big.view(-1)[1:1 + 90 * 512].view(90, 512)):
        m, p = model, plain
        if feat.dtype == torch.float16:
            m, p = _to(model, dtype=torch.float16), _to(plain, dtype=torch.float16)
            m.fused = True
        assert torch.equal(m(feat), p(feat))
    model.classifier = model.classifier.double()
    with pytest.raises(RuntimeError):                                         # the torch path's own dtype error, not a kernel call
        model(x)
    assert not kernel_calls


# ---------------------------------------------------------------- gradients against dense float64 autograd
GRAD_CASES = [(1, 3, 300, 10, False), (3, 2, 257, 8, False), (5, 2, 130, 10, True)]      # E, C, N, topj, frozen router


@pytest.mark.parametrize("E,C,N,topj,router", GRAD_CASES)
def test_fused_gradients_match_dense_float64_autograd(gpu_device, kernel_calls, E, C, N, topj, router):
    model = _build(E, C, 7500 + E, topj=topj, router=router)
    if router:
        model.ada_router.gate.weight.requires_grad = False
    x = HB.randn(7600 + E, N, 512)
    for k in range(C):                                                        # topj signal rows per class
        rows = torch.arange(topj) * C + k + 3
        x[rows] = 4.0 * model.classifier[:, k] * 512 ** 0.5 + HB.randn(7700 + k, topj, 512)
    wsum = torch.arange(1, C + 1, dtype=torch.float64) * 0.5

    m64 = _to(model, dtype=torch.float64)
    l64 = _formulas(m64, x.double())
    top = l64.detach().topk(topj + 1, dim=0)[0]
    assert float((top[topj - 1] - top[topj]).min()) >= 1e-3, "near-tie at the pooling boundary: pick another seed"
    p64 = l64.topk(topj, dim=0)[0].mean(0, keepdim=True)
    (p64 * wsum).sum().backward()
    ref = {n: p.grad for n, p in m64.named_parameters()}

    dev = torch.device("cuda:0")
    outs = {}
    for fused in (False, True):
        m = _to(model, device=dev)
        m.fused = fused
        pooled = m(x.to(dev))
        (pooled * wsum.float().to(dev)).sum().backward()
        outs[fused] = (pooled.detach().double().cpu(), {n: p.grad for n, p in m.named_parameters()})
    assert len(kernel_calls) == 1
    rel = lambda a, b: float((a - b).abs().max()) / float(b.abs().max())
    e_torch, e_fused = rel(outs[False][0], p64.detach()), rel(outs[True][0], p64.detach())
    print(f"adapter pooled E={E}: torch fp32 {e_torch:.3e}  fused {e_fused:.3e}")
    assert e_fused <= min(2 * e_torch, CAP), ("pooled", e_fused, e_torch)
    for n, g in ref.items():
        gt, gf = outs[False][1][n], outs[True][1][n]
        if g is None:
            assert gt is None and gf is None, n
            continue
        e_torch, e_fused = rel(gt.double().cpu(), g), rel(gf.double().cpu(), g)
        print(f"adapter grad E={E} {n}: torch fp32 {e_torch:.3e}  fused {e_fused:.3e}")
        assert e_fused <= min(2 * e_torch, CAP), (n, e_fused, e_torch)


# ---------------------------------------------------------------- determinism and isolation
def test_kernel_is_deterministic_and_stream_safe(gpu_device):
    dev = torch.device("cuda:0")
    model = _to(_build(3, 3, 7800), device=dev)
    x = HB.randn(7801, 777, 512).to(dev)
    a, b = _kernel_logits(model, x), _kernel_logits(model, x)
    assert torch.equal(a, b)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = _kernel_logits(model, x)
    side.synchronize()
    assert torch.equal(a, c)
    model.adapter_0[0].weight.data.mul_(1.5)                                  # invisible to _version: the image must be rebuilt
    d = _kernel_logits(model, x)
    assert not torch.equal(a, d)
    with torch.no_grad():
        assert float((d - _formulas(model, x)).abs().max()) < CAP


@pytest.mark.parametrize("E,C,N", [(1, 2, 65), (5, 64, 130)])
def test_kernel_stays_inside_its_buffers(gpu_device, E, C, N):
    from moc_amd import _lib
    dev = torch.device("cuda:0")
    model = _to(_build(E, C, 7900 + E), device=dev)
    x = HB.randn(7901, N, 512).to(dev)
    h = _lib.lib()
    nbytes, pad = h.moc_adapter_workspace(N, 512, 128, E, C), 4096
    assert nbytes == E * 768 * 1024 + C * 2048
    ws = torch.full((nbytes + 2 * pad,), 0xA5, dtype=torch.uint8, device=dev)
    out = torch.full((N * C + 2 * pad,), 7.25, dtype=torch.float32, device=dev)
    nets = _experts(model)
    arr = lambda ts: ctypes.cast((ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts]), ctypes.c_void_p)
    gate = model.ada_router.gate.weight if E > 1 else None
    torch.cuda.synchronize()
    rc = h.moc_adapter_logits(x.data_ptr(), N, 512, arr([n[0].weight for n in nets]), arr([n[2].weight for n in nets]), 128, E,
                              _lib.ptr(gate), model.classifier.data_ptr(), C, ctypes.c_float(model.clip_ratio),
                              out.data_ptr() + 4 * pad, ws.data_ptr() + pad, nbytes, None)
    torch.cuda.synchronize()
    assert rc == 0, h.moc_last_error()
    assert bool((ws[:pad] == 0xA5).all()) and bool((ws[pad + nbytes:] == 0xA5).all()), "workspace written out of bounds"
    assert bool((out[:pad] == 7.25).all()) and bool((out[pad + N * C:] == 7.25).all()), "logits written out of bounds"
    assert torch.equal(out[pad:pad + N * C].view(N, C), _kernel_logits(model, x))


def test_fused_forward_forms_no_dense_intermediates(gpu_device, kernel_calls):
    from moc_amd import _lib
    dev = torch.device("cuda:0")
    N, E, C = 4097, 5, 2
    model = _to(_build(E, C, 8000), device=dev)
    model.fused = True
    x = HB.randn(8001, N, 512).to(dev)
    model(x[:100].contiguous())                                               # library handles, first-use allocations
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    pooled = model(x)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before                         # the bag itself is part of `before`
    assert len(kernel_calls) == 2 and pooled.shape == (1, C)
    budget = N * C * 4 + _lib.lib().moc_adapter_workspace(N, 512, 128, E, C) + (8 << 20)
    assert extra < budget < N * 512 * E * 4, (extra, budget)
