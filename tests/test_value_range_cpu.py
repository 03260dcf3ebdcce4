"""The CPU half of the value-range tests (test_gpu_value_range.py): the inputs' preconditions and the float64 helpers of
helpers_value_range.py, with no GPU.

Reference noise of the gradient task (helpers_value_range.grad_case: C = 2, D = 256, slides of 300 and 120 rows, bank seed
9, bag seeds 372 / 373, model seed 3), max|g32 - g64| / max|g64| over both slides and both storages, as
`python -m pytest tests/test_value_range_cpu.py -k noise -s` prints it:

    scale   fp32 rows (slide 0, 1)   bf16 rows (slide 0, 1)
    2^-6    1.4e-5, 1.7e-6           2.1e-6, 4.4e-6
    1/8     4.6e-7, 1.3e-6           3.6e-7, 2.8e-6
    5       2.2e-7, 4.9e-7           1.3e-7, 7.0e-7
    32      1.5e-6, 6.7e-7           3.4e-6, 6.0e-7
    200     6.2e-2, 6.1e-2           5.3e-2, 4.4e-2     (the reference's own cancellation in 1 - p: losses 5e-7 and 1e-7)

At 200 the measured rule is therefore loose by construction; it is not tightened by hand.
"""
import numpy as np
import pytest
import torch

import helpers as H
import helpers_value_range as V

DTYPES = [torch.float32, torch.bfloat16]


def test_power_of_two_scaling_is_exact_in_storage_and_fp16_downscaling_is_not():
    """What the exact GPU checks rest on: 2^s X is X with another exponent in fp32 and bf16 storage over the whole tested
    range of s, and in fp16 storage for upscaling (subnormals included) -- while DOWNscaling fp16 rounds low bits of small
    elements away, which is why the fp16 checks only scale up."""
    from moc_amd import synth
    W, We = synth.make_bank(9, 256, 2)
    x = synth.make_bag(72, 300, 256, We, 2, label=1)
    for dtype, scales in ((torch.float32, V.POW2_WIDE), (torch.bfloat16, V.POW2_WIDE), (torch.float16, V.POW2_F16)):
        xs = x.to(dtype)
        for s in scales:
            y = V.scaled_pow2(xs, s)
            assert y.dtype == dtype and torch.isfinite(y.to(torch.float32)).all()
    x16 = x.to(torch.float16)
    assert int((x16.to(torch.float32).abs() < 2.0 ** -14).sum()) > 0, "the fp16 input holds subnormal elements"
    with pytest.raises(AssertionError, match="not exact"):
        V.scaled_pow2(x16, -7)


def test_next_pow2_and_row_factors():
    assert V.next_pow2([0.3, 1.0, 1.0001, 5.0, 23.0, 0.25]).tolist() == [0.5, 1.0, 2.0, 8.0, 32.0, 0.25]
    f = V.row_factors(300, 1)
    assert f.shape == (300, 1) and 0.01 <= float(f.min()) < 0.05 and 10.0 < float(f.max()) <= 30.0


def test_stats64_is_the_oracles_keys_in_float64():
    from moc_amd import synth
    C = 3
    W, We = synth.make_bank(5, 256, C)
    We = We.clone()
    We[:, :C] *= 0.5                                                  # W_ext[:, :C] != W: logits come from W
    x = synth.make_bag(6, 50, 256, We, C, label=2) * 5.0
    st = V.stats64(x, W, We, C)
    assert st.shape == (2 * C + 3, 50) and st.dtype == torch.float64
    xd = x.double()
    lge = torch.cat([xd @ W.double(), (xd @ We.double())[:, C:]], 1)
    keys = H.selector_keys(lge, C)
    assert torch.equal(st[:C].t(), lge[:, :C])
    assert torch.allclose(st[C:2 * C].t(), keys["softmax"], atol=1e-15, rtol=0)
    assert torch.equal(st[2 * C], keys["gap"][:, 0]) and torch.equal(st[2 * C + 1], -keys["lowbg"][:, 0])
    assert torch.equal(st[2 * C + 2], lge[:, C:].max(1)[0])
    assert torch.allclose(V.softmax64(st[:C].float()), st[C:2 * C], atol=1e-6, rtol=0)
    # degree one / degree zero
    st2 = V.stats64(x * 4.0, W, We, C)
    rows = V.degree_one_rows(C)
    assert torch.equal(st2[rows], st[rows] * 4.0) and not torch.allclose(st2[C:2 * C], st[C:2 * C])


def test_select_rule_takes_lowest_rows_on_ties():
    """The restated rule on test_select_ties_take_lowest_rows' keys, all four selectors."""
    N, C, j = 300, 2, 50
    lge = torch.zeros(N, C + 4)
    lge[:, 0] = torch.arange(N).float() % 7
    lge[:, 1] = -lge[:, 0]
    lge[:, 2:] = 1.0
    k = H.selector_keys(lge, C)
    st = torch.cat([lge[:, :C].t(), k["softmax"].t(), k["gap"].t(), lge[:, C:].sum(1, keepdim=True).t(), lge[:, C:].max(1, keepdim=True)[0].t()], 0)
    only_top = V.select_rule(st, C, j, ("delta_softmax", "delta_diff", "bottomk"))
    exp = set()
    for c in range(C):
        exp.update(sorted(range(N), key=lambda i: (-float(lge[i, c]), i))[:j])
    assert only_top == sorted(exp)
    assert V.select_rule(st, C, j, ("topk", "delta_softmax", "delta_diff")) == list(range(j))        # equal background: the first j rows
    assert V.boundary_ties(st, C, j) == 2 * C + 2
    assert V.select_rule(st, C, N + 5) == list(range(N))
    z = torch.zeros(2 * C + 3, 4)
    z[0] = torch.tensor([-1.0, -0.0, 0.0, -0.0])                      # -0 ties with +0: rows 1 and 2, not row 2 alone
    z[1] = torch.tensor([3.0, 2.0, 1.0, 0.0])
    assert V.select_rule(z, C, 2, ("delta_softmax", "delta_diff", "bottomk")) == [0, 1, 2]
    assert V.select_rule(z, C, 1, ("delta_softmax", "delta_diff", "bottomk")) == [0, 1]


def test_crafted_inputs():
    from moc_amd import synth
    W, We = synth.make_bank(3, 256, 2)
    r = V.repeated_rows(4, 256, We, 2)
    assert r.shape == (100, 256) and torch.equal(r, r[:1].expand(100, 256)) and float(r.abs().max()) > 0
    z = V.zero_block_slide(5, 100, 256, We, 2)
    assert z.shape == (147, 256) and not z[:40].any() and not z[-7:].any() and bool(z[40:140].abs().sum(1).min() > 0)
    Wu, Weu = V.unequal_bank(7, 256, 2)
    n = Weu.norm(dim=0)
    assert abs(float(n[0]) - 0.25) < 1e-6 and abs(float(n[-1]) - 1.5) < 1e-6 and torch.equal(Weu[:, :2], Wu)
    sl = V.slot_ranges([3, 4], torch.tensor([1, 0, 1, 0, 0, 0, 1], dtype=torch.uint8))
    assert [(o, n, k.tolist()) for o, n, k in sl] == [(0, 2, [0, 2]), (3, 1, [3])]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("scale", sorted(set(V.GRAD_SCALES + V.FWD_SCALES)))
def test_gradient_task_preconditions(dtype, scale):
    """In float64: every class's K-th and (K+1)-th mixed scores differ by more than 1000 times max|mixed32 - mixed64| (the
    pooled set cannot differ between two correct fp32 implementations), and every pooled row's pre-activations are farther
    from zero than 2e-6 max(1, scale) (no ReLU of a pooled row flips)."""
    case = V.grad_case(dtype, scale)
    for s_i, (gap, noise, relu) in enumerate(V.grad_case_margins(case)):
        print(f"scale {scale:g} {dtype} slide {s_i}: top-K gap {gap:.3e}, mixed noise {noise:.3e}, ReLU margin {relu:.3e}")
        assert gap > 1000.0 * noise, (s_i, gap, noise)
        assert relu > 2e-6 * max(1.0, scale), (s_i, relu)
        assert case.ref[s_i].pred == case.ref32[s_i].pred
    assert all(np.isfinite(r.loss) and all(np.isfinite(g).all() for g in r.grads) for r in case.ref + case.ref32)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_reference_noise_measured(dtype):
    """Prints the table of the module docstring; asserts only what the measured rule needs of it: below scale 200 the
    reference's fp32 run is within 1e-4 of its float64 run, relative to the largest gradient."""
    for scale in V.GRAD_SCALES:
        case = V.grad_case(dtype, scale)
        noise = V.grad_noise(case)
        print(f"scale {scale:g} {dtype}: max|g32 - g64| / max|g64| per slide {['%.1e' % v for v in noise]}; "
              f"loss64 {[('%.3e' % r.loss) for r in case.ref]}")
        if scale < 200.0:
            assert max(noise) < 1e-4


def test_measured_rule_is_the_base_tolerance_plus_four_times_the_reference_noise():
    t64 = np.array([1.0, -2.0, 0.0])
    t32 = t64 + np.array([2.0 ** -23, -3 * 2.0 ** -22, 0.0])
    a = V.measured_allowed(2e-6, 1e-4, t32, t64)
    assert np.allclose(a, 2e-6 + 1e-4 * np.abs(t64) + 4 * 3 * 2.0 ** -22, rtol=1e-12, atol=0)
