"""Adam's update on the GPU at the precision moc_amd/csrc/moc_step_shared.h states it: adam_update() -- inlined by the
narrow and the wide one-launch step, the tile-record step, the two forms of the three-launch step and moc_adam_step -- is
torch's single-tensor Adam with coupled L2 operation by operation, each rounded on its own, with the coefficients of
adam_coef().  helpers.adam_ops32 / adam_coef32 restate that in numpy float32 and every kernel's parameters and moments must
equal it BIT FOR BIT; independently they must lie within helpers.ADAM_BOUND of the textbook update in float64
(helpers.adam_f64, in helpers.adam_err_units' units; the bound is measured by test_adam_restatement_cpu.py, which also
shows that dropping the weight decay, either bias correction, or moving eps under the root misses it a thousandfold).

A: moc_adam_step (engine.adam_step) takes the gradient as an input: crafted values (helpers.adam_inputs), three
   hyper-parameter sets, t = 1 ... 100000, three gradient scales.
B: the five step kernels at test_gpu_step_lds.py's shapes, each asserting its mode and path first: the gradient of a
   slide comes from moc_train_grad at the same state (the same launches short of the update), the step from
   moc_train_steps, over three slides in a row, so that the state carried forward is the state written.

The float64 bound in B.  The constants of helpers.ADAM_BOUND are measured on A's inputs, in which no sum of the update
cancels by more than 5/3.  B's gradients are what the slides give: at t = 1 (zero moments, so exp_avg' = (1 - b1) g and
exp_avg_sq' = (1 - b2) g g) the decay term wd p (some 1e-6) cancels against gradients of that size in a few elements, and
the one rounding of g + wd p is then hundreds to ten thousands of ulps of g g: on these shapes the restatement ITSELF is
520 ... 51,000 units of exp_avg_sq and up to 17 units of the parameter from float64 in steps 1 to 3 (the same figures on
the CPU with autograd's gradients; from t = 1000 on it is at most 2.8 and 1.2, inside the bound; every case prints its
own).  So in B an element may be off float64 by helpers.ADAM_BOUND
units or by twice the restatement's own distance from float64 at that element, whichever is larger -- the rule that
made the constants (twice the float64 error of the restatement on the inputs used), applied to B's inputs element by
element; never less than the constants, and computed from the float64 comparison, not from what the kernel wrote."""
import ctypes as C_

import numpy as np
import pytest
import torch

import helpers as H
from test_gpu_fp32_terms import expected_image

pytestmark = pytest.mark.gpu

RECORDS, FULL = 1000001, 1000002      # MOC_TILE_PATH_RECORDS / MOC_TILE_PATH_FULL
NAMES = ("parameters", "exp_avg", "exp_avg_sq")


@pytest.fixture(scope="module")
def dev(gpu_device):
    return gpu_device


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_bits(got, exp, what):
    for name, a, b in zip(NAMES, got, exp):
        diff = _bits(a) != _bits(b)
        assert not diff.any(), (f"{what}: {name} differ from adam_ops32 in {int(diff.sum())} of {diff.size} elements, first at "
                                f"{int(np.flatnonzero(diff)[0])}: {a[diff][0]!r} for {b[diff][0]!r}")


def _write(meta, p, m, v, g, step):
    """the flat arrays into the learner's tensors in place (None: left alone), every step counter to `step`"""
    o, st = 0, meta.optimizer.state
    for par, grad in zip(meta.params, meta.grads):
        n = par.numel()
        for dst, src in ((par.data, p), (st[par]["exp_avg"], m), (st[par]["exp_avg_sq"], v), (grad, g)):
            if src is not None:
                dst.copy_(torch.from_numpy(np.array(src[o:o + n], dtype=np.float32)).view_as(dst))
        st[par]["step"].fill_(step)
        o += n
    meta.refresh()


def _read(meta):
    torch.cuda.synchronize()
    st = meta.optimizer.state
    flat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).cpu().numpy()
    return (flat(meta.params), flat([st[q]["exp_avg"] for q in meta.params]), flat([st[q]["exp_avg_sq"] for q in meta.params]))


def _steps(meta):
    return [int(meta.optimizer.state[q]["step"]) for q in meta.params]


def _adam_kw(hp):
    return dict(lr=hp[0], betas=(hp[1], hp[2]), eps=hp[3], weight_decay=hp[4])


# ------------------------------------------------------------------ A: moc_adam_step, the gradient given
@pytest.mark.parametrize("hp", H.ADAM_HP, ids=lambda hp: "lr%g_b%g_%g_eps%g_wd%g" % hp)
@pytest.mark.parametrize("D", [256, 1024])
def test_adam_step_is_the_restatement_bit_for_bit(dev, D, hp):
    from moc_amd import engine as E, main_moc as M
    torch.manual_seed(0)
    model = M.senet(D, 4).to(dev)
    meta = E.MetaState(model, torch.optim.Adam(model.parameters(), **_adam_kw(hp)), need_grads=True)
    assert sum(q.numel() for q in meta.params) == H.adam_numel(D)
    worst = np.zeros(3)
    for t in H.ADAM_STEPS:
        p, m, v, g = H.adam_inputs(D, t)
        for gs in H.ADAM_GRAD_SCALES:
            what = f"D {D} t {t} grad_scale {gs:.4g}"
            _write(meta, p, m, v, g, t - 1)
            E.adam_step(meta, grad_scale=gs)
            got = _read(meta)
            exp = H.adam_ops32(p, m, v, g, H.adam_coef32(*hp, t, gs))
            _assert_bits(got, exp, what)                                     # all four tensors, first and last elements included
            err = H.adam_err_units(*got, p, m, v, g, H.adam_f64(p, m, v, g, *hp, t, gs))
            worst = np.maximum(worst, err)
            assert all(e <= b for e, b in zip(err, H.ADAM_BOUND)), (what, err, H.ADAM_BOUND)
            assert _steps(meta) == [t] * 4 and meta.c.step == t, what
            for blk in H.adam_zero_blocks(D):                                # g = m = v = 0: the weight-decay term alone
                moved = _bits(got[0][blk]) != _bits(p[blk])
                assert moved.all() if hp[4] > 0 else not moved.any(), what
                assert not got[1][blk].any() and not got[2][blk].any() if hp[4] == 0 else got[2][blk].all()
            E.adam_step(meta, grad_scale=gs)                                 # ... and again, from what the first call wrote
            _assert_bits(_read(meta), H.adam_ops32(*exp, g, H.adam_coef32(*hp, t + 1, gs)), what + ", second call")
            assert _steps(meta) == [t + 1] * 4 and meta.c.step == t + 1, what
    print(f"moc_adam_step D {D} {hp}: largest error against float64 in units (exp_avg, exp_avg_sq, parameter) "
          f"{worst[0]:.2f} {worst[1]:.2f} {worst[2]:.2f}; bound {H.ADAM_BOUND}")


# ------------------------------------------------------------------ B: the five step kernels
F32, BF16 = torch.float32, torch.bfloat16
OTHER = H.ADAM_HP[2]                     # (3e-4, .8, .99, 1e-6, 1e-2)
# kernel, (C, K, D), storage, tile records, mask of ones, mode (moc_train_runs_mode), what the step leaves in n_pair[0],
# the non-default hyper-parameters too
STEP_CASES = [
    ("narrow", (15, 4, 256), F32, False, True, 2, None, True),         # pool_w1_step_kernel at its largest LDS
    ("narrow", (2, 10, 1024), F32, False, True, 2, None, False),       # ... with its row stage full
    ("tiles", (15, 4, 256), F32, True, True, 1, RECORDS, True),        # pool_w1_step_tiles_kernel over the records
    ("tiles", (2, 10, 1024), F32, True, True, 1, FULL, False),         # ... pooling among the full scores
    ("three", (8, 8, 256), F32, False, False, 0, None, True),          # pool_step_kernel + w1_update_kernel
    ("three", (30, 10, 256), BF16, False, False, 0, None, False),      # topk_mean_kernel + finish_kernel + w1_update_kernel
    ("wide", (61, 8, 1024), F32, False, False, 2, None, False),        # pool_w1_step_wide_kernel in two chunks
    ("wide", (30, 10, 512), BF16, False, False, 2, None, True),        # ... in one
]


def _mode(batch):
    from moc_amd._lib import lib
    return int(lib().moc_train_runs_mode(C_.byref(batch.c), C_.byref(batch.meta_ws()[1])))


def _supported(C, K, D):
    from moc_amd._lib import lib
    return int(lib().moc_p2p_step_supported(C, K, D, H.GRAD_STEP_TOPJ))


def _grad(E, batch, meta, lab, slide):
    E.train_grad(batch, meta, lab, slide, 15)
    g = torch.cat([t.reshape(-1) for t in meta.grads]).cpu().numpy()
    return g, int(batch.meta_ws()[0]["n_pair"].cpu()[0])


def _assert_f64(got, exp, p, m, v, g, hp, t, what):
    """B's float64 bound (module docstring): per element, helpers.ADAM_BOUND units or twice the restatement's own distance
    from float64, whichever is larger.  -> the largest errors of `got` and of the restatement, in units"""
    ref = H.adam_f64(p, m, v, g, *hp, t)
    e_got = H.adam_err_elements(*got, p, m, v, g, ref)
    e_own = H.adam_err_elements(*exp, p, m, v, g, ref)
    for name, a, own, bound in zip(("exp_avg", "exp_avg_sq", "parameters"), e_got, e_own, H.ADAM_BOUND):
        bad = (a > bound) & (a > 2.0 * own)
        assert not bad.any(), (f"{what}: {name}: {int(bad.sum())} elements outside the float64 bound, worst {a[bad].max():.2f} units "
                               f"(bound {bound}; the restatement there {own[bad][a[bad].argmax()]:.2f})")
    return [float(a.max()) for a in e_got], [float(a.max()) for a in e_own]


@pytest.mark.parametrize("kernel,shape,dtype,tile_records,masked,mode,path,other", STEP_CASES,
                         ids=[f"{c[0]}-{'x'.join(map(str, c[1]))}" for c in STEP_CASES])
def test_step_kernels_apply_the_restatement_to_their_own_gradient(dev, kernel, shape, dtype, tile_records, masked, mode, path, other):
    from moc_amd import engine as E
    C, K, D = shape
    keep = E.TILE_RECORDS
    E.TILE_RECORDS = tile_records
    try:
        batch, lab, meta = H.grad_step_batch(dev, C, K, D, dtype, masked=masked, adam=_adam_kw(H.ADAM_HP[0]))
        assert _supported(C, K, D) == (0 if kernel == "three" else 1)
        assert _mode(batch) == mode
        p0 = _read(meta)[0]
        n, rng = p0.size, np.random.default_rng(40 + C)
        group = meta.optimizer.param_groups[0]
        for hp in ((H.ADAM_HP[0], OTHER) if other else (H.ADAM_HP[0],)):
            group.update(_adam_kw(hp))
            for t0 in (1, 1000):
                # exp_avg / exp_avg_sq at magnitudes like real moments (|m| ~ 1e-4, v ~ 1e-8 > 0); zero before the first step
                m0 = (1e-4 * rng.standard_normal(n)).astype(np.float32) if t0 > 1 else np.zeros(n, np.float32)
                v0 = (1e-8 * rng.uniform(0.25, 4.0, n)).astype(np.float32) if t0 > 1 else np.zeros(n, np.float32)
                _write(meta, p0, m0, v0, None, t0 - 1)
                for slide in range(len(H.GRAD_STEP_SIZES)):
                    t = t0 + slide
                    what = f"{kernel} step {shape} {hp} t {t} slide {slide}"
                    g, left = _grad(E, batch, meta, lab, slide)        # the gradient at the state the step starts from
                    if slide == 0:
                        again, _ = _grad(E, batch, meta, lab, slide)
                        assert np.array_equal(_bits(g), _bits(again)), what + ": the gradient-only launch is not deterministic"
                    assert (left == path) if path else (left not in (RECORDS, FULL)), (what, left)
                    p, m, v = _read(meta)                               # the state the last step wrote
                    E.train_steps(batch, meta, lab, slide, 1, 15)
                    got = _read(meta)
                    left = int(batch.meta_ws()[0]["n_pair"].cpu()[0])
                    assert (left == path) if path else (left not in (RECORDS, FULL)), (what, left)
                    exp = H.adam_ops32(p, m, v, g, H.adam_coef32(*hp, t))
                    _assert_bits(got, exp, what)
                    e_got, e_own = _assert_f64(got, exp, p, m, v, g, hp, t, what)
                    assert _steps(meta) == [t] * 4 and meta.c.step == t, what
                    assert g.any() and not np.array_equal(got[0], p), what
                    if dtype == F32:        # the W1 operand image the step keeps: still the three-term split of the stepped W1
                        image = meta.w1_image[:64 * D * 3 * 2].cpu().numpy().view(np.uint16)
                        assert np.array_equal(image, expected_image(got[0][:64 * D].reshape(64, D))), what + ": W1 image"
                    print(f"{what}: mode {mode}, n_pair[0] {left}; units from float64 (exp_avg, exp_avg_sq, parameter) "
                          f"{e_got[0]:.2f} {e_got[1]:.2f} {e_got[2]:.2f}, the restatement's {e_own[0]:.2f} {e_own[1]:.2f} {e_own[2]:.2f}")
    finally:
        E.TILE_RECORDS = keep
