"""Adam's update as moc_amd/csrc/moc_step_shared.h states it -- torch's single-tensor Adam with coupled L2, operation by
operation, each rounded to fp32 on its own, coefficients formed in double and cast once -- restated in numpy float32
(helpers.adam_coef32 / adam_ops32), against the textbook update in float64 (helpers.adam_f64).  No GPU here: this file
measures how far the restatement is from float64 in helpers.adam_err_units' units, on the inputs test_gpu_adam.py gives
moc_adam_step; helpers.ADAM_MEASURED records that and helpers.ADAM_BOUND, twice it, is what the GPU tests allow.  It then
shows that the bound is not delicate: each wrong update of helpers.ADAM_VARIANTS misses it by more than a thousand times."""
import itertools
import math

import numpy as np
import pytest
import torch

import helpers as H

DS = (256, 1024)


def _cases():
    return itertools.product(DS, H.ADAM_HP, H.ADAM_STEPS, H.ADAM_GRAD_SCALES)


def _errors(D, hp, t, gs, variant=None, got=None):
    p, m, v, g = H.adam_inputs(D, t)
    if got is None:
        got = H.adam_ops32(p, m, v, g, H.adam_coef32(*hp, t, gs))
    return H.adam_err_units(*got, p, m, v, g, H.adam_f64(p, m, v, g, *hp, t, gs, variant=variant))


def test_measured_error_of_the_restatement_against_float64(capsys):
    worst = np.zeros(3)
    for D, hp, t, gs in _cases():
        worst = np.maximum(worst, _errors(D, hp, t, gs))
    with capsys.disabled():
        print(f"\nadam_ops32 against adam_f64, largest error in units (exp_avg, exp_avg_sq, parameter): "
              f"ADAM_MEASURED = ({worst[0]:.2f}, {worst[1]:.2f}, {worst[2]:.2f})")
    # the recorded constants are this measurement (to the two decimals they are written with), the bound twice it
    assert all(abs(w - r) <= 0.0051 for w, r in zip(worst, H.ADAM_MEASURED)), (tuple(worst), H.ADAM_MEASURED)
    assert H.ADAM_BOUND == tuple(math.ceil(2 * r) for r in H.ADAM_MEASURED)
    assert all(1 <= b <= 100 for b in H.ADAM_BOUND), H.ADAM_BOUND      # a few units, as the operation count says


def test_inputs_keep_every_intermediate_zero_or_normal():
    """... so that no comparison hinges on denormal handling; and the inputs have the blocks they are said to have.  The
    GPU test steps a second time, from the state the first step left: there (1 - beta2) g g may be denormal in a few
    elements whose parameter the first step moved next to zero -- but only added to an exp_avg_sq that absorbs it whole,
    so a device that flushed it would still write the same bits."""
    tiny = np.float32(1e-37)
    for D, hp, t, gs in _cases():
        p, m, v, g0 = H.adam_inputs(D, t)
        sevenths = np.arange(0, p.size, 7)
        sevenths = sevenths[(sevenths < H.ADAM_V0_BLOCK.start) | (sevenths >= H.ADAM_V0_BLOCK.stop)]
        assert p.size == H.adam_numel(D) and not g0[sevenths].any() and np.count_nonzero(g0) > p.size // 2
        assert all(not g0[b].any() and not m[b].any() and not v[b].any() for b in H.adam_zero_blocks(D))
        assert not v[H.ADAM_V0_BLOCK].any() and g0[H.ADAM_V0_BLOCK].all() and p.all()
        assert (t == 1) == (not m.any() and not v.any())
        for step in (t, t + 1):
            wd, omb1, b2, omb2, eps, nss, bc2s, gsc = H.adam_coef32(*hp, step, gs)
            g = g0 * gsc
            wp = wd * p
            ge = g + wp
            if step == t:           # the crafted state: neither sum cancels by more than 5/3 (a rounding's worth of slack)
                lerp = (np.float64(hp[1]) * m, (1.0 - hp[1]) * ge.astype(np.float64))
                for a, b in ((g.astype(np.float64), wp.astype(np.float64)), lerp):
                    assert (np.abs(a) + np.abs(b) <= (5.0 / 3 + 1e-5) * np.abs(a + b)).all(), (D, hp, t, gs)
            d = ge - m
            s = omb1 * d
            sq1 = omb2 * ge
            sq = sq1 * ge
            vb = v * b2
            p, m, v = H.adam_ops32(p, m, v, g0, (wd, omb1, b2, omb2, eps, nss, bc2s, gsc))
            num = nss * m
            for name, x in (("g*scale", g), ("wd*p", wp), ("g", ge), ("g-m", d), ("(1-b1)(g-m)", s), ("(1-b2)g", sq1),
                            ("(1-b2)g*g", sq), ("m'", m), ("v'", v), ("-step*m'", num), ("p'", p)):
                ok = (x == 0) | (np.abs(x) >= tiny)
                if step == t + 1 and name == "(1-b2)g*g":
                    ok |= (vb + sq == vb) & (vb >= tiny)
                assert ok.all() and np.isfinite(x).all(), (D, hp, step, gs, name, x[~ok][:4])


# where each wrong update differs at all: the bias corrections are 1 to fp32 at large t, the weight-decay variants need wd > 0
_VARIANT_STEPS = {"no_wd": H.ADAM_STEPS, "decoupled_wd": H.ADAM_STEPS, "eps_in_root": H.ADAM_STEPS,
                  "no_bc1": (1, 2, 7), "no_bc2": (1, 2, 7)}


@pytest.mark.parametrize("variant", H.ADAM_VARIANTS)
def test_each_wrong_update_misses_the_bound_a_thousandfold(variant):
    """The restatement measured against a float64 update that is wrong in one respect: for every hyper-parameter set in
    which the variant is a different update, at one of the steps where it is, some unit's error is >= 1000 x its bound."""
    for D, hp in itertools.product(DS, H.ADAM_HP):
        if variant in ("no_wd", "decoupled_wd") and hp[4] == 0.0:
            continue
        ratio = max(max(e / b for e, b in zip(_errors(D, hp, t, 1.0, variant=variant), H.ADAM_BOUND))
                    for t in _VARIANT_STEPS[variant])
        assert ratio >= 1000.0, (variant, D, hp, ratio)
    # ... while the right update is inside it everywhere
    for D, hp, t, gs in _cases():
        assert all(e <= b for e, b in zip(_errors(D, hp, t, gs), H.ADAM_BOUND))


@pytest.mark.parametrize("hp", H.ADAM_HP)
def test_coefficients_against_a_direct_float64_evaluation(hp):
    from decimal import Decimal, getcontext
    getcontext().prec = 60
    lr, b1, b2, eps, wd = hp
    for t in H.ADAM_STEPS:
        k = H.adam_coef32(*hp, t, 1.0 / 3)
        assert all(type(x) is np.float32 for x in k) and len(k) == 8
        # 1 - beta^t and the square root in 60 digits, from the doubles the optimizer holds: the fp32 coefficient is the
        # nearest float to within the double evaluation's own error (a relative 1e-12 is a 1e-5th of an fp32 ulp)
        bc1 = 1 - Decimal(b1) ** t
        bc2 = 1 - Decimal(b2) ** t
        assert float(k[5]) == pytest.approx(float(-(Decimal(lr) / bc1)), rel=2.0 ** -24, abs=0)
        assert float(k[6]) == pytest.approx(float(bc2.sqrt()), rel=2.0 ** -24, abs=0)
        assert k[5] == np.float32(-(lr / (1.0 - b1 ** t))) and k[6] == np.float32(math.sqrt(1.0 - b2 ** t))
        assert (k[0], k[1], k[2], k[3], k[4], k[7]) == tuple(np.float32(x) for x in (wd, 1.0 - b1, b2, 1.0 - b2, eps, 1.0 / 3))
    assert H.adam_coef32(*hp, 100000)[5] == np.float32(-lr) and H.adam_coef32(*hp, 100000)[6] == np.float32(1.0)
    assert H.adam_coef32(*hp, 1000)[5] == np.float32(-lr) and H.adam_coef32(*hp, 1000)[6] < np.float32(1.0)
    assert H.adam_coef32(lr, 0.0, b2, eps, wd, 1)[5] == np.float32(-lr)      # beta1 = 0 at t = 1: -lr exactly


@pytest.mark.parametrize("hp", H.ADAM_HP)
def test_torch_cpu_adam_stays_within_the_bound_of_the_restatement(hp):
    """torch.optim.Adam(foreach=False) on the CPU over 40 steps: every one of its steps, taken from the state it is in, is
    within the bound of the float64 update AND of adam_ops32 from that state -- which ties the restatement to the
    reference's optimiser without claiming its bits (its vectorised kernels fuse: a last bit of exp_avg differs in a
    good part of the elements)."""
    lr, b1, b2, eps, wd = hp
    # A state that evolves over 40 steps cannot be crafted element by element as adam_inputs is, so cancellation is kept
    # out by construction: |p| in [0.5, 2) (40 steps move it by 0.12 at most: no sign change), and a gradient that keeps
    # its sign -- p's, at magnitudes over nine decades, in one half of the elements; the other sign, at 0.1 ... 1 (five
    # times wd |p| and more), in the other half.  Then g + wd p has g's sign in every step and exp_avg never opposes it.
    n = 20000
    rng = np.random.default_rng(77)
    sign = rng.choice([-1.0, 1.0], n)
    p0 = (sign * rng.uniform(0.5, 2.0, n)).astype(np.float32)
    along = np.arange(n) < n // 2
    par = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([par], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    n_diff = 0
    for t in range(1, 41):
        g = np.where(along, sign * 10.0 ** rng.uniform(-9.0, 0.0, n), -sign * 10.0 ** rng.uniform(-1.0, 0.0, n)).astype(np.float32)
        g[t % 7::7] = 0.0
        par.grad = torch.from_numpy(g.copy())
        opt.step()
        st = opt.state[par]
        got = (par.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy())
        assert int(st["step"]) == t
        ref = H.adam_f64(p, m, v, g, *hp, t)
        ops = H.adam_ops32(p, m, v, g, H.adam_coef32(*hp, t))
        err64 = H.adam_err_units(*got, p, m, v, g, ref)
        ref.p, ref.m, ref.v = (a.astype(np.float64) for a in ops)
        err32 = H.adam_err_units(*got, p, m, v, g, ref)
        assert all(e <= b for e, b in zip(err64, H.ADAM_BOUND)), (t, err64)
        assert all(e <= b for e, b in zip(err32, H.ADAM_BOUND)), (t, err32)
        n_diff += int((got[1] != ops[1]).sum())
        p, m, v = got                                       # the next step starts from torch's own state
    print(f"elements of exp_avg in which torch's CPU Adam and adam_ops32 differed, over 40 steps: {n_diff} of {40 * p0.size}")
