"""TransMIL's PPEG on the GPU (moc_ppeg_forward, moc_ppeg_backward; engine.ppeg_forward / ppeg_backward;
model_mil.PPEGFused, PPEG.fused, TransMIL.fused_ppeg): the two entries against float64 autograd of PPEG itself on the CPU,
exact impulses, what they write, determinism, another stream, which path a call takes, and the model.

The judging rule is that of tests/test_gpu_nystrom_conv.py: in the same test torch's fp32 path on the GPU and the kernels are
each compared with the float64 evaluation; the kernels' error may be at most max(f x torch's error, 2^-20 x max|reference|)
and never more than 1e-4 x max(1, max|reference|).  f = 2 for an entry alone, f = 4 for the model.  Both errors are printed.

Shapes: the kernels work on tiles of 4 x 4 positions that read the 10 x 10 around them, and the backward leaves one partial
sum per run of tiles, at most H W / 128 of them.  (1, 1), (2, 2), (3, 3) are all halo; (7, 7) is exactly one full window and
(8, 8) one past it; (17, 17) is TransMIL's 257-row square, ragged in both axes; (33, 33) and (40, 40) have several partial
blocks (8 and 12) whose runs of tiles end inside a tile row; (5, 40) and (40, 5) catch a swapped H and W.  No tile side
exceeds 16, so no larger side is needed.  The impulse positions on the 20 x 20 square are the sequence's ends, the first
position with a full window, and either side of a tile's and a partial block's edge.

The closed forms of the impulse tests are tests/test_ppeg_cpu.py's, checked there against float64 autograd."""
import copy
import functools

import pytest
import torch

import helpers_baselines as HB
from test_gpu_nystrom_train import _logits64, _model, _model_grads
from test_ppeg_cpu import IMPULSES, grid, impulse_backward, impulse_forward, merged_table, ppeg_autograd

pytestmark = pytest.mark.gpu

DIM = 512
ENTRIES = ("ppeg_forward", "ppeg_backward")
ATTENTION = ("nystrom_landmark_values", "nystrom_token_values", "nystrom_pinv", "nystrom_landmark_values_lse",
             "nystrom_landmark_backward", "nystrom_token_backward", "nystrom_conv_backward", "nystrom_pinv_iterates",
             "nystrom_pinv_backward")
GRADS = ("proj.weight", "proj.bias", "proj1.weight", "proj1.bias", "proj2.weight", "proj2.bias")


def _judge(what, fused, torch32, ref, f):
    """The rule of the module docstring; prints both errors."""
    ref = ref.double().cpu()
    top = float(ref.abs().max())
    e_torch = float((torch32.double().cpu() - ref).abs().max())
    e_fused = float((fused.double().cpu() - ref).abs().max())
    floor = 2.0 ** -20 * top
    print(f"ppeg {what}: max|ref| {top:.3e}  torch fp32 {e_torch:.3e}  fused {e_fused:.3e}  (floor {floor:.3e})")
    assert fused.shape == ref.shape and torch.isfinite(fused).all(), what
    assert e_fused <= max(f * e_torch, floor) and e_fused <= 1e-4 * max(1.0, top), (what, e_fused, e_torch, floor)


@functools.lru_cache(maxsize=None)
def _module():
    """A seeded PPEG(512) on the CPU; never modified."""
    from moc_amd.model_mil import PPEG
    torch.manual_seed(9100)
    return PPEG(DIM).eval()


@functools.lru_cache(maxsize=None)
def _grid_module():
    """The same with every parameter rounded to multiples of 2^-10."""
    m = copy.deepcopy(_module())
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(grid(p))
    return m


def _params(m):
    return (m.proj.weight, m.proj.bias, m.proj1.weight, m.proj1.bias, m.proj2.weight, m.proj2.bias)


@functools.lru_cache(maxsize=None)
def _case(H, W):
    """(x, dout) in fp32 and the float64 (out, dx, {name: gradient}), all on the CPU."""
    n = 1 + H * W
    x, dout = HB.randn(9200 + 50 * H + W, 1, n, DIM), HB.randn(9300 + 50 * H + W, 1, n, DIM)
    return (x, dout), ppeg_autograd(copy.deepcopy(_module()).double(), x.double(), H, W, dout.double())


def _run(m, x, H, W, dout):
    """(out, dx, {name: gradient}) from the two entries, with module m's parameters."""
    from moc_amd import engine
    w7, b7, w5, b5, w3, b3 = [p.detach() for p in _params(m)]
    out = engine.ppeg_forward(x, H, W, w7, b7, w5, b5, w3, b3)
    dx, dw7, db7, dw5, db5, dw3, db3 = engine.ppeg_backward(x, H, W, w7, w5, w3, dout)
    return out, dx, dict(zip(GRADS, (dw7, db7, dw5, db5, dw3, db3)))


SHAPES = [(1, 1), (2, 2), (3, 3), (7, 7), (8, 8), (17, 17), (33, 33), (40, 40), (5, 40), (40, 5)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_entries_match_float64_autograd(gpu_device, H, W):
    (x, dout), (ref_out, ref_dx, ref) = _case(H, W)
    m, x, dout = copy.deepcopy(_module()).to(gpu_device), x.to(gpu_device), dout.to(gpu_device)
    keep = [t.clone() for t in (x, dout) + tuple(p.detach() for p in _params(m))]
    out, dx, got = _run(m, x, H, W, dout)
    assert all(torch.equal(a, b) for a, b in zip((x, dout) + tuple(p.detach() for p in _params(m)), keep)), "an input was written"
    assert out.shape == x.shape and dx.shape == x.shape and out.dtype == dx.dtype == torch.float32
    assert torch.equal(out[0, 0], x[0, 0]) and torch.equal(dx[0, 0], dout[0, 0]), "the class-token row is a copy"
    t_out, t_dx, t = ppeg_autograd(m, x, H, W, dout)
    what = f"entry {H}x{W}"
    _judge(what + " out", out, t_out, ref_out, 2)
    _judge(what + " dx", dx, t_dx, ref_dx, 2)
    for k in GRADS:                                                           # each convolution's own window of G, own bias
        assert got[k].shape == ref[k].shape and got[k].dtype == torch.float32, k
        _judge(what + " d" + k, got[k], t[k], ref[k], 2)


def _impulse(py, px):
    return (37 * py + 11 * px + 5) % DIM, (-0.5 if (py + px) % 2 else 2.0)


@pytest.mark.parametrize("py,px", IMPULSES)
def test_a_gradient_impulse_gives_the_table_exactly(gpu_device, py, px):
    H = W = 20
    c, a = _impulse(py, px)
    m = _grid_module()
    w = merged_table(m.proj.weight.detach(), m.proj1.weight.detach(), m.proj2.weight.detach())
    x = grid(HB.randn(9400, 1, 1 + H * W, DIM))
    dout = torch.zeros_like(x)
    dout[0, 1 + py * W + px, c] = a
    want_dx, G, db = impulse_backward(x, H, W, w, py, px, c, a)
    window = (min(H, py + 4) - max(0, py - 3)) * (min(W, px + 4) - max(0, px - 3))
    assert 0 < int((want_dx != 0).sum()) <= window and 0 < int((G != 0).sum()) <= window     # (a rounded value may be zero)
    dev = gpu_device
    _, dx, got = _run(copy.deepcopy(m).to(dev), x.to(dev), H, W, dout.to(dev))
    assert bool((dx.cpu() == want_dx).all()), "dx is not the table around the impulse"
    assert bool((got["proj.weight"].cpu()[:, 0] == G).all()), "dw7 is not the x values around the impulse"
    assert bool((got["proj1.weight"].cpu()[:, 0] == G[:, 1:6, 1:6]).all()) and bool((got["proj2.weight"].cpu()[:, 0] == G[:, 2:5, 2:5]).all())
    for k in ("proj.bias", "proj1.bias", "proj2.bias"):
        assert bool((got[k].cpu() == db).all()), k


@pytest.mark.parametrize("py,px", IMPULSES)
def test_an_input_impulse_gives_the_table_exactly(gpu_device, py, px):
    from moc_amd import engine
    H = W = 20
    c, a = _impulse(py, px)
    m = _grid_module()
    w7, b7, w5, b5, w3, b3 = [p.detach() for p in _params(m)]
    want = impulse_forward(H, W, merged_table(w7, w5, w3), (b7 + b5) + b3, py, px, c, a, torch.float32)
    x = torch.zeros(1, 1 + H * W, DIM)
    x[0, 1 + py * W + px, c] = a
    out = engine.ppeg_forward(x.to(gpu_device), H, W, *[p.to(gpu_device) for p in (w7, b7, w5, b5, w3, b3)])
    assert bool((out.cpu() == want).all()), "out is not bias + the table around the impulse"


def test_a_zero_gradient_gives_exact_zeros(gpu_device):
    H, W = 17, 17
    (x, dout), _ = _case(H, W)
    _, dx, got = _run(copy.deepcopy(_module()).to(gpu_device), x.to(gpu_device), H, W, torch.zeros_like(dout).to(gpu_device))
    assert not dx.any() and not any(bool(g.any()) for g in got.values())


def test_entries_are_deterministic(gpu_device):
    H, W = 40, 40
    (x, dout), _ = _case(H, W)
    m, x, dout = copy.deepcopy(_module()).to(gpu_device), x.to(gpu_device), dout.to(gpu_device)
    (a_out, a_dx, a), (b_out, b_dx, b) = _run(m, x, H, W, dout), _run(m, x, H, W, dout)
    assert torch.equal(a_out, b_out) and torch.equal(a_dx, b_dx) and all(torch.equal(a[k], b[k]) for k in GRADS)


def test_entries_work_on_another_stream(gpu_device):
    H, W = 17, 17
    (x, dout), _ = _case(H, W)
    m, x, dout = copy.deepcopy(_module()).to(gpu_device), x.to(gpu_device), dout.to(gpu_device)
    want_out, want_dx, want = _run(m, x, H, W, dout)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=gpu_device)
    with torch.cuda.stream(side):
        out, dx, got = _run(m, x, H, W, dout)
    side.synchronize()
    assert torch.equal(out, want_out) and torch.equal(dx, want_dx) and all(torch.equal(got[k], want[k]) for k in GRADS)


@pytest.mark.parametrize("H,W", [(1, 1), (33, 33)])
def test_entries_stay_inside_their_buffers(gpu_device, H, W):
    from moc_amd import _lib
    dev, h, pad = gpu_device, _lib.lib(), 4096                                # pad: floats (or bytes of the workspace)
    (x, dout), _ = _case(H, W)
    m, x, dout = copy.deepcopy(_module()).to(dev), x.to(dev), dout.to(dev)
    w7, b7, w5, b5, w3, b3 = [p.detach() for p in _params(m)]
    inputs = (x, dout, w7, b7, w5, b5, w3, b3)
    keep = [t.clone() for t in inputs]
    want_out, want_dx, want = _run(m, x, H, W, dout)
    nbytes = h.moc_ppeg_backward_workspace(H, W, DIM)
    assert 0 < nbytes <= 2 << 20 if H * W < 1024 else 0 < nbytes < H * W * DIM * 4

    def band(numel):
        return torch.full((numel + 2 * pad,), 7.25, dtype=torch.float32, device=dev)

    def inside(t, like):
        return t[pad:pad + like.numel()].view(like.shape)

    def untouched(t, like):
        return bool((t[:pad] == 7.25).all()) and bool((t[pad + like.numel():] == 7.25).all())

    ws = torch.full((nbytes + 2 * pad,), 0xA5, dtype=torch.uint8, device=dev)
    out, dx = band(x.numel()), band(x.numel())
    g = {k: band(want[k].numel()) for k in GRADS}
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr() + 4 * pad                                      # noqa: E731
    rc = h.moc_ppeg_forward(x.data_ptr(), H, W, DIM, w7.data_ptr(), b7.data_ptr(), w5.data_ptr(), b5.data_ptr(), w3.data_ptr(),
                            b3.data_ptr(), p(out), None)
    assert rc == 0, h.moc_last_error()
    rc = h.moc_ppeg_backward(x.data_ptr(), H, W, DIM, w7.data_ptr(), w5.data_ptr(), w3.data_ptr(), dout.data_ptr(), p(dx),
                             p(g["proj.weight"]), p(g["proj.bias"]), p(g["proj1.weight"]), p(g["proj1.bias"]),
                             p(g["proj2.weight"]), p(g["proj2.bias"]), ws.data_ptr() + pad, nbytes, None)
    assert rc == 0, h.moc_last_error()
    torch.cuda.synchronize()
    assert bool((ws[:pad] == 0xA5).all()) and bool((ws[pad + nbytes:] == 0xA5).all()), "workspace written out of bounds"
    assert untouched(out, x) and untouched(dx, x), "out or dx written out of bounds"
    assert all(untouched(g[k], want[k]) for k in GRADS), "a gradient tensor written out of bounds"
    assert all(torch.equal(a, b) for a, b in zip(inputs, keep)), "an input was written"
    # every element inside is overwritten: 7.25 nowhere unless the result itself is 7.25 there, and the results are the wrappers'
    assert torch.equal(inside(out, x), want_out) and torch.equal(inside(dx, x), want_dx)
    assert all(torch.equal(inside(g[k], want[k]), want[k]) for k in GRADS)


# ---------------------------------------------------------------- which path a call takes
@pytest.fixture
def calls(monkeypatch):
    from moc_amd import engine
    seen = {}
    for name in ENTRIES + ATTENTION:
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


def _step(m, x, H, W, G):
    """(output, {name: gradient}) of sum(m(x, H, W) * G) with respect to x and every parameter."""
    m.zero_grad(set_to_none=True)
    x = x.detach().requires_grad_(True)                                       # (keeps the strides of a non-contiguous x)
    out = m(x, H, W)
    (out * G).sum().backward()
    grads = {"x": x.grad}
    grads.update({k: p.grad.clone() for k, p in m.named_parameters()})
    return out.detach(), grads


def test_which_path_a_call_takes(gpu_device, calls, monkeypatch):
    dev, H, W = gpu_device, 17, 17
    (x, G), _ = _case(H, W)
    m, gx, gG = copy.deepcopy(_module()).to(dev), x.to(dev), G.to(dev)

    def unchanged(mod, xx, gg, hh=H, ww=W):
        """The same step with the switch off and on: equal bits, and no entry call."""
        mod.fused = False
        want_out, want = _step(mod, xx, hh, ww, gg)
        mod.fused = True
        got_out, got = _step(mod, xx, hh, ww, gg)
        return (not any(calls.values()) and torch.equal(got_out, want_out) and sorted(got) == sorted(want)
                and all(torch.equal(got[k], want[k]) for k in want))

    m.fused = False
    _step(m, gx, H, W, gG)
    assert not any(calls.values())                                            # switch off: the torch code
    assert unchanged(copy.deepcopy(_module()), x, G)                          # on the CPU
    wide = torch.zeros(1, 1 + H * W, DIM + 8, device=dev)
    wide[:, :, :DIM] = gx
    assert not wide[:, :, :DIM].is_contiguous() and unchanged(m, wide[:, :, :DIM], gG)          # a strided x
    assert unchanged(m, torch.cat([gx, gx.flip(1)]), torch.cat([gG, gG]))     # a batch of 2
    assert unchanged(copy.deepcopy(m).double(), gx.double(), gG.double())     # fp64 parameters
    m.fused = True
    with torch.no_grad():                                                     # no_grad: one forward call, nothing kept
        quiet = m(gx, H, W)
    assert calls["ppeg_forward"] == 1 and calls["ppeg_backward"] == 0 and quiet.grad_fn is None
    _reset(calls)

    def boom(*a, **k):
        raise AssertionError("a convolution's own forward was called")
    for conv in (m.proj, m.proj1, m.proj2):
        monkeypatch.setattr(conv, "forward", boom)
    out, grads = _step(m, gx, H, W, gG)                                       # a training step never enters the convolutions
    assert calls["ppeg_forward"] == 1 and calls["ppeg_backward"] == 1
    assert torch.equal(out, quiet), "the training forward differs from the no-grad forward"
    assert sorted(grads) == sorted(("x",) + GRADS)
    assert all(torch.isfinite(g).all() and g.any() for g in grads.values())


# ---------------------------------------------------------------- the model
DATA_SEED, ROWS = 9500, 600                                                   # a 25 x 25 square


@functools.lru_cache(maxsize=None)
def _model_ref():
    data = HB.randn(DATA_SEED, ROWS, 512)
    m64 = copy.deepcopy(_model()).double()
    logits = _logits64(m64, data.double())
    return logits.detach(), _model_grads(m64, logits)


@pytest.mark.parametrize("attention", [False, True])
def test_transmil_trains_with_the_fused_ppeg_and_matches_float64(gpu_device, calls, attention):
    data = HB.randn(DATA_SEED, ROWS, 512)
    ref_logits, ref = _model_ref()
    model, g = copy.deepcopy(_model()).to(gpu_device), data.to(gpu_device)
    plain_logits = model(g)[0]
    plain = _model_grads(model, plain_logits)
    assert not any(calls.values())
    model.fused_ppeg = True
    if attention:
        model.fused = model.fused_pinv = model.fused_train = model.fused_conv = model.fused_pinv_train = True
    logits = model(g)[0]
    got = _model_grads(model, logits)
    assert calls["ppeg_forward"] == 1 and calls["ppeg_backward"] == 1, calls
    assert any(calls[k] for k in ATTENTION) == attention, calls                # a switch of its own
    assert sorted(got) == sorted(ref) == sorted(plain)
    what = "TransMIL, all switches" if attention else "TransMIL, fused_ppeg alone"
    _judge(f"{what}: logits", logits.detach(), plain_logits.detach(), ref_logits, 4)
    for k in ("pos_layer.proj.weight", "pos_layer.proj1.weight", "pos_layer.proj2.weight", "pos_layer.proj.bias",
              "pos_layer.proj1.bias", "pos_layer.proj2.bias", "layer1.attn.to_qkv.weight", "_fc1.0.weight"):
        _judge(f"{what}: d{k}", got[k], plain[k], ref[k], 4)
