"""fp32 bags on the bf16 matrix cores: every fp32-bag forward multiplies a row by W1 as the six products of their three
bf16 terms (moc_meta_forward.hip fwd_split4 / fwd_mfma6; the W1 image holds moc_split3 of W1).  Needs an MI355X: run with -m gpu.

Stated bound: against a float64 product of the same rows, the pre-activations (read back through the hidden layer,
relu(x W1^T + b1)) are within 1e-6 absolute on values up to 1 (relative above; 2e-6 at D = 1024) and within twice the error of an fp32 fused-multiply-add chain
over each quarter of the columns folded as ((p0 + p1) + p2) + p3 -- the rounding of the fp32-MFMA forward this replaced."""
import numpy as np
import pytest
import torch

from moc_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(gpu_device):
    return gpu_device


def _rne_bf16(x32):
    u = x32.view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def _bf16_f32(h):
    return (h.astype(np.uint32) << 16).view(np.float32)


def expected_image(W1):
    """moc_split3<false> of W1 [H, D] in the image's [nt][kk][term][lane][8] order, as uint16."""
    W1 = np.ascontiguousarray(W1, dtype=np.float32)
    Hh, D = W1.shape
    hi = _rne_bf16(W1)
    r1 = (W1 - _bf16_f32(hi)).astype(np.float32)
    mid = _rne_bf16(r1)
    lo = _rne_bf16((r1 - _bf16_f32(mid)).astype(np.float32))
    out = np.zeros(Hh * D * 3, dtype=np.uint16)
    h, d = np.meshgrid(np.arange(Hh), np.arange(D), indexing="ij")
    lane = (((d & 31) >> 3) << 4) | (h & 15)
    off = (((h >> 4) * (D // 32) + (d >> 5)) * 3 * 64 + lane) * 8 + (d & 7)
    for t, v in enumerate((hi, mid, lo)):
        out[(off + t * 64 * 8).ravel()] = v.ravel()
    return out


def _image_u16(meta, D):
    return meta.w1_image[:64 * D * 3 * 2].cpu().numpy().view(np.uint16)


def test_truncating_split_is_exact_for_tiny_and_large_magnitudes():
    """The row split (fwd_split4): x0 = x with its low 16 bits cleared, x1 the same of x - x0, x2 = (x - x0) - x1; the
    three are bf16 values and x0 + x1 + x2 == x, for normal fp32 values of any size whose terms stay normal."""
    rng = np.random.default_rng(3)
    n = 200_000                                                            # |x| in [2^-100, 2^101): every term normal
    x = (rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n) * np.exp2(rng.integers(-100, 101, n))).astype(np.float32)
    x = np.concatenate([x, np.float32([1.0, -1.0, 3.4e38, -3.4e38, 1e-20, 7.0e-31, 0.0, 1 + 2.0 ** -23])])
    trunc = lambda v: (v.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    x0 = trunc(x)
    r = (x - x0).astype(np.float32)
    x1 = trunc(r)
    x2 = (r - x1).astype(np.float32)
    assert np.array_equal(trunc(x2), x2)                                   # the third term is a bf16 value too
    assert np.array_equal(x0.astype(np.float64) + x1 + x2, x.astype(np.float64))


def _h1_of(dev, D, n_slides, rows, seed, scale=1.0):
    from moc_amd import engine as E, main_moc as M
    torch.manual_seed(seed)
    model = M.senet(D, 4).to(dev)
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n_slides * rows, D, generator=g) * scale).to(dev)
    b = E.CompactBatch(n_slides, n_slides * rows, rows, D, torch.float32, 2, 3, rows, 1, dev, X=x)
    b.n_sel.fill_(rows)
    b.set_layout([i * rows for i in range(n_slides + 1)])
    meta = E.MetaState(model)
    E.meta_forward(b, meta, 0, n_slides, 0, keep_hidden=True)
    torch.cuda.synchronize()
    t, _ = b.meta_ws()
    W1 = model.model[0].weight.detach().cpu().numpy()
    b1 = model.model[0].bias.detach().cpu().numpy()
    return x.cpu().numpy(), W1, b1, t["H1"][:n_slides * rows].cpu().numpy(), meta


def _fp32_chain(x, W1):
    """The replaced kernel's rounding: an fp32 fma chain per quarter of the columns, ((p0 + p1) + p2) + p3."""
    D = x.shape[1]
    tot = None
    for q in range(4):
        acc = np.zeros((x.shape[0], W1.shape[0]), dtype=np.float32)
        for k in range(q * D // 4, (q + 1) * D // 4):
            acc = (acc.astype(np.float64) + np.outer(x[:, k].astype(np.float64), W1[:, k].astype(np.float64))).astype(np.float32)
        tot = acc if tot is None else (tot + acc).astype(np.float32)
    return tot


@pytest.mark.parametrize("D", [256, 512, 1024])
@pytest.mark.parametrize("train", [True, False])
def test_fp32_forward_error_bound_against_float64(dev, D, train):
    """training: one slide (the sixteen-wave kernel); evaluation: four slides of 1,024 rows (the 128-row kernel)."""
    n_slides, rows = (1, 300) if train else (4, 1024)
    x, W1, b1, h1, _ = _h1_of(dev, D, n_slides, rows, 11 + D)
    pre64 = x.astype(np.float64) @ W1.T.astype(np.float64) + b1.astype(np.float64)
    ref = np.maximum(pre64, 0.0)
    err = np.abs(h1.astype(np.float64) - ref)
    assert float(np.abs(pre64).max()) > 1.0                                 # O(1) pre-activations
    bound = 1e-6 * max(1.0, D / 512)                                        # (fp32 rounding grows with D: the replaced kernel
    assert float((err / np.maximum(np.abs(pre64), 1.0)).max()) <= bound, float(err.max())      # reached 1.3e-6 at D = 1024)
    old = np.maximum((_fp32_chain(x, W1) + b1).astype(np.float32).astype(np.float64), 0.0)
    old_err = np.abs(old - ref)
    assert float(err.max()) <= 2 * float(old_err.max()), (float(err.max()), float(old_err.max()))
    assert float(err.mean()) <= 2 * float(old_err.mean()), (float(err.mean()), float(old_err.mean()))


@pytest.mark.parametrize("scale", [2.0 ** -6, 0.3, 5.0, 32.0])
@pytest.mark.parametrize("D", [256, 512])
@pytest.mark.parametrize("train", [True, False])
def test_fp32_forward_error_bound_at_scale(dev, D, train, scale):
    """The bound above with rows times `scale` and b1 as initialised.  It is relative above 1 already and 1e-6 absolute
    below; that form is kept, and the absolute part takes the factor max(1, scale) for the product term -- the rounding
    of x W1^T grows with the products' size, not with that of a pre-activation that cancels or that b1 dominates:
    |error| <= 1e-6 max(|pre|, max(1, scale)).  The "within twice the fp32 chain" clause stays as it is."""
    n_slides, rows = (1, 300) if train else (4, 1024)
    x, W1, b1, h1, _ = _h1_of(dev, D, n_slides, rows, 11 + D, scale=scale)
    pre64 = x.astype(np.float64) @ W1.T.astype(np.float64) + b1.astype(np.float64)
    ref = np.maximum(pre64, 0.0)
    err = np.abs(h1.astype(np.float64) - ref)
    bound = 1e-6 * max(1.0, D / 512)
    worst = float((err / np.maximum(np.abs(pre64), max(1.0, scale))).max())
    old = np.maximum((_fp32_chain(x, W1) + b1).astype(np.float32).astype(np.float64), 0.0)
    old_err = np.abs(old - ref)
    print(f"scale {scale:g}: max |pre| {float(np.abs(pre64).max()):.3g}, error {float(err.max()):.3e} (fp32 chain {float(old_err.max()):.3e}), "
          f"worst / bound {worst / bound:.3f}")
    assert worst <= bound, float(err.max())
    assert float(err.max()) <= 2 * float(old_err.max()), (float(err.max()), float(old_err.max()))
    assert float(err.mean()) <= 2 * float(old_err.mean()), (float(err.mean()), float(old_err.mean()))


@pytest.mark.parametrize("D", [256, 512, 1024])
def test_w1_image_is_the_three_term_split_after_the_image_kernel(dev, D):
    _, W1, _, _, meta = _h1_of(dev, D, 1, 64, 5)
    assert np.array_equal(_image_u16(meta, D), expected_image(W1))


def test_w1_image_stays_the_three_term_split_through_the_tile_step(dev):
    """The training steps rewrite W1 and its image in the step kernel: after a pass of them (and a second pass on the same
    work arrays) the image is still moc_split3 of the W1 the steps left behind, bit for bit."""
    from moc_amd import engine, main_moc as M
    Cc, D, j, K = 2, 512, 400, 10
    W, We = synth.make_bank(1234, D, Cc)
    M.set_classifier_bank(W.to(dev), We.to(dev))
    bags = [synth.make_bag_device(4321 + i, 3000, D, We, Cc, i % Cc, dev, torch.float32) for i in range(6)]
    res = M.ResidentBags(bags, [i % Cc for i in range(6)], dev)
    torch.manual_seed(0)
    model = M.senet(D, 4).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
    bank = M._bank_for(res.X, dev)
    plan = res.train_plan(Cc, Cc + 4, j, K, [])
    batch, lab = plan["batch"], plan["labels"]
    m, kept = engine.draw_row_masks(batch.total)
    batch.set_mask(m, kept)
    batch.phase_a(bank)
    meta = engine.MetaState(model, opt)
    W0 = model.model[0].weight.detach().clone()
    for _ in range(2):
        engine.train_steps(batch, meta, lab, 0, 6, 15)
        torch.cuda.synchronize()
        W1 = model.model[0].weight.detach().cpu().numpy()
        assert np.array_equal(_image_u16(meta, D), expected_image(W1))
    assert not torch.equal(W0, model.model[0].weight.detach())              # (the steps did move W1)
