"""Shared helpers for the parity tests (test-side only)."""
from __future__ import annotations

import itertools
import math
import os
import types

import numpy as np
import torch

from moc_amd import synth

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SELECTORS = ("topk", "delta_softmax", "delta_diff", "bottomk")

# fp32 tolerance stated by BASELINE.json:north_star ("within 1e-4 fp32")
ATOL = 1e-4
# a row may legitimately enter/leave a top-j set when its key is this close to the
# j-th key: fp32 dot products summed in a different order differ by ~1e-7 relative
KEY_BAND = 2e-6


def golden(name):
    return np.load(os.path.join(GOLDEN_DIR, name + ".npz"))


def discard_from_mask(dmask: int):
    return [n for k, n in enumerate(SELECTORS) if dmask >> k & 1]


def unpack_mask(bits, n):
    return torch.from_numpy(np.unpackbits(bits)[:n].astype(bool))


def unpack_masks(bits, sizes):
    out, off = [], 0
    for n in sizes:
        nb = (n + 7) // 8
        out.append(unpack_mask(bits[off:off + nb], n))
        off += nb
    return out


def selector_keys(logits_ext: torch.Tensor, C: int):
    """Key columns the four selectors rank rows by (larger = selected first).
    Returns dict name -> [N, ncols] fp32."""
    lg = logits_ext[:, :C]
    two = torch.topk(lg, 2, dim=1)[0]
    return {
        "top": lg,
        "softmax": torch.softmax(lg, dim=1),
        "gap": (two[:, 0] - two[:, 1]).abs().unsqueeze(1),
        "lowbg": (-logits_ext[:, C:].sum(dim=1)).unsqueeze(1),
    }


def assert_topj_set(got_idx, exp_idx, key_col: torch.Tensor, band=KEY_BAND, what=""):
    """got/exp: 1-D index collections for ONE key column.  They must agree except
    for rows whose key lies within `band` of the selection boundary."""
    got, exp = set(int(i) for i in got_idx), set(int(i) for i in exp_idx)
    assert len(got) == len(exp), f"{what}: |got|={len(got)} |exp|={len(exp)}"
    if got == exp:
        return
    boundary = min(float(key_col[i]) for i in exp)
    scale = max(1.0, abs(boundary))
    for i in got ^ exp:
        d = abs(float(key_col[i]) - boundary)
        assert d <= band * scale, f"{what}: row {i} differs, key margin {d:.3e}"


def ambiguous_rows(keys: dict, j: int, band=KEY_BAND):
    """Rows whose membership in some selector's top-j is within the tie band."""
    amb = set()
    for name, K in keys.items():
        n = K.size(0)
        if n <= j:
            continue
        for c in range(K.size(1)):
            col = K[:, c]
            srt = torch.sort(col, descending=True)[0]
            b = float(srt[j - 1])
            near = (col - b).abs() <= band * max(1.0, abs(b))
            amb.update(torch.nonzero(near).flatten().tolist())
    return amb


def make_args(C, j, K, discard=()):
    return types.SimpleNamespace(disable_tqdm=True, n_classes=C, topj=j, topk=K,
                                 discard_classifiers=list(discard), pretrain="conch",
                                 ablation_study="none")


class ListDataset:
    """Dataset protocol of the reference's split objects (dataset_generic.py:380-393)."""

    def __init__(self, bags, labels, repeat_num=None):
        self.bags, self.labels, self.repeat_num = bags, labels, repeat_num

    def real_len(self):
        return len(self.bags)

    def __len__(self):
        return self.repeat_num if self.repeat_num else len(self.bags)

    def __getitem__(self, idx):
        if idx >= len(self):
            raise IndexError
        k = idx % len(self.bags)
        x = self.bags[k]
        return x, self.labels[k], np.zeros((x.size(0), 2), dtype=np.int64), f"slide_{k}.h5"


class ListLoader:
    """batch_size=1 default-collate stand-in for torch DataLoader (main_moc.py:290-293)."""

    def __init__(self, bags, labels, repeat_num=None):
        self.dataset = ListDataset(bags, labels, repeat_num)

    def __iter__(self):
        ds = self.dataset
        for i in range(len(ds)):
            x, y, coords, path = ds[i]
            yield x.unsqueeze(0), torch.tensor([y]), torch.from_numpy(coords).unsqueeze(0), [path]

    def __len__(self):
        return len(self.dataset)


def seeded_senet(oracle, seed):
    torch.manual_seed(seed)
    return oracle.Senet(512, 4)


def flat_params(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu().numpy()


def flat_grads(model):
    return torch.cat([p.grad.detach().reshape(-1) for p in model.parameters()]).cpu().numpy()


def flat_state(opt, key):
    return torch.cat([opt.state[p][key].reshape(-1) for g in opt.param_groups
                      for p in g["params"]]).cpu().numpy()


def bank_and_bag(seed, N, C, label, D=512):
    W, We = synth.make_bank(seed, D, C)
    return W, We, synth.make_bag(seed + 500, N, D, We, C, label=label)


def assert_adam_params_close(got, exp, v_exp, step, grad_noise, lr=1e-3, base=2e-6, what="", beta2=0.999):
    """Parameters after `step` Adam steps.  Adam's update is lr*m_hat/(sqrt(v_hat)+eps):
    for an element whose gradient is comparable to the gradient noise between two
    correct fp32 implementations (`grad_noise`, absolute), the update is sign-like and
    may differ by up to lr per step; elsewhere the difference scales with
    grad_noise/|g|.  Bound each element accordingly."""
    got, exp, v_exp = (np.asarray(a, dtype=np.float64) for a in (got, exp, v_exp))
    v_hat = v_exp / (1.0 - beta2 ** step)
    allowed = base + lr * step * np.minimum(1.0, 4.0 * grad_noise / (np.sqrt(v_hat) + 1e-8))
    bad = np.abs(got - exp) > allowed
    assert not bad.any(), (f"{what}: {int(bad.sum())} params outside the Adam noise bound; worst "
                           f"{np.abs(got - exp)[bad].max():.3e} (allowed {allowed[bad].min():.3e})")


# ---- Adam's update at the precision moc_step_shared.h states it: test_adam_restatement_cpu.py, test_gpu_adam.py
# adam_update() is torch's single-tensor Adam with coupled L2, operation by operation, each operation rounded to fp32 on
# its own, with coefficients formed in double and cast once (adam_coef() in moc_meta.hip).  adam_coef32 / adam_ops32 restate
# exactly that in numpy float32 -- the BIT reference of the GPU tests (torch's CPU Adam is not: its vectorised kernels fuse);
# adam_f64 is the textbook update in float64, and adam_err_units measures a result against it in units that do not depend
# on the magnitudes.
ADAM_HP = ((1e-3, 0.9, 0.999, 1e-8, 1e-4), (3e-3, 0.9, 0.999, 1e-8, 0.0), (3e-4, 0.8, 0.99, 1e-6, 1e-2))   # lr, b1, b2, eps, wd
ADAM_STEPS = (1, 2, 7, 1000, 100000)
ADAM_GRAD_SCALES = (1.0, 1.0 / 8, 1.0 / 3)
ADAM_VARIANTS = ("no_wd", "no_bc1", "no_bc2", "eps_in_root", "decoupled_wd")
# The largest error of adam_ops32 against adam_f64 over adam_inputs(D, t) for D in (256, 1024), every ADAM_HP, ADAM_STEPS
# and ADAM_GRAD_SCALES, in adam_err_units' units (exp_avg, exp_avg_sq, parameter), as printed by
#   python -m pytest tests/test_adam_restatement_cpu.py -k measured -s
# The GPU tests' bound is twice that, rounded up to whole units: the factor covers a division or a square root that is
# faithfully rather than correctly rounded on the device.  Taken from this float64 comparison, never from a GPU run.
ADAM_MEASURED = (1.12, 5.13, 0.98)
ADAM_BOUND = tuple(int(np.ceil(2.0 * e)) for e in ADAM_MEASURED)


def adam_coef32(lr, beta1, beta2, eps, wd, step, grad_scale=1.0):
    """adam_coef(): the arithmetic in double (Python floats), one cast to fp32 each.
    -> (wd, one_minus_b1, beta2, one_minus_b2, eps, neg_step_size, bc2_sqrt, grad_scale)"""
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    return tuple(np.float32(x) for x in (wd, 1.0 - beta1, beta2, 1.0 - beta2, eps, -(lr / bc1), math.sqrt(bc2), grad_scale))


def adam_ops32(p, m, v, g, coef):
    """adam_update() on float32 arrays, every operation its own numpy operation on float32 operands (so nothing is kept
    wider than fp32 in between); `g * grad_scale` first, as every kernel that inlines it does.  -> (p', m', v')"""
    wd, one_minus_b1, beta2, one_minus_b2, eps, neg_step_size, bc2_sqrt, grad_scale = coef
    p, m, v, g = (np.asarray(a, dtype=np.float32) for a in (p, m, v, g))
    g = g * grad_scale
    g = g + wd * p
    m = m + one_minus_b1 * (g - m)
    v = v * beta2 + (one_minus_b2 * g) * g
    denom = np.sqrt(v) / bc2_sqrt + eps
    p = p + (neg_step_size * m) / denom
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


def adam_f64(p, m, v, g, lr, beta1, beta2, eps, wd, step, grad_scale=1.0, variant=None):
    """The textbook Adam step with coupled L2 in float64 (hyper-parameters as the Python floats they are; grad_scale as the
    fp32 value the C entry is handed).  `variant`: one of ADAM_VARIANTS, a WRONG update -- only to show what the bounds
    reject.  -> namespace p, m, v (the stepped values), g_abs (|g * grad_scale|), wd"""
    assert variant is None or variant in ADAM_VARIANTS
    p, m, v, g = (np.asarray(a, dtype=np.float64) for a in (p, m, v, g))
    g = g * float(np.float32(grad_scale))
    g_abs = np.abs(g)
    if variant == "decoupled_wd":
        p = p * (1.0 - lr * wd)
    elif variant != "no_wd":
        g = g + wd * p
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    m_hat = m if variant == "no_bc1" else m / (1.0 - beta1 ** step)
    v_hat = v if variant == "no_bc2" else v / (1.0 - beta2 ** step)
    denom = np.sqrt(v_hat + eps) if variant == "eps_in_root" else np.sqrt(v_hat) + eps
    return types.SimpleNamespace(p=p - lr * m_hat / denom, m=m, v=v, g_abs=g_abs, wd=wd)


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def adam_err_elements(got_p, got_m, got_v, p, m, v, g, ref64):
    """The error of every element of (got_p, got_m, got_v) against adam_f64's `ref64` from the state (p, m, v), in units of
      exp_avg ....... ulp of max(|m|, |g| + wd |p|)   (g: the scaled gradient)
      exp_avg_sq .... ulp of the float64 v'
      parameter ..... ulp(p) + 8 ulp(|p' - p|)
    -> (err_m, err_v, err_p), arrays.  (The ulp of zero is the smallest denormal: no unit is zero.)"""
    p64, m64 = np.asarray(p, dtype=np.float64), np.asarray(m, dtype=np.float64)
    unit_m = _ulp32(np.maximum(np.abs(m64), ref64.g_abs + ref64.wd * np.abs(p64)))
    unit_v = _ulp32(ref64.v)
    unit_p = _ulp32(p64) + 8.0 * _ulp32(ref64.p - p64)
    err = lambda got, ref, unit: np.abs(np.asarray(got, dtype=np.float64) - ref) / unit
    return err(got_m, ref64.m, unit_m), err(got_v, ref64.v, unit_v), err(got_p, ref64.p, unit_p)


def adam_err_units(got_p, got_m, got_v, p, m, v, g, ref64):
    """The largest of adam_err_elements per tensor -> (err_m, err_v, err_p), floats"""
    return tuple(float(e.max()) for e in adam_err_elements(got_p, got_m, got_v, p, m, v, g, ref64))


def adam_numel(D):
    return 64 * D + 64 + 4 * 64 + 4          # W1 [64, D], b1, W2 [4, 64], b2, flat in that order


ADAM_ZERO_BLOCK, ADAM_V0_BLOCK = slice(100, 164), slice(200, 264)


def adam_zero_blocks(D):
    """the blocks with g = m = v = 0: one in W1, one in W2, the last two elements of b2"""
    n = adam_numel(D)
    return (ADAM_ZERO_BLOCK, slice(64 * D + 64 + 8, 64 * D + 64 + 24), slice(n - 2, n))


_adam_inputs = {}


def _adam_cancels(a, b):
    """a + b, of opposite signs and within a factor of four of one another in magnitude"""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(a) / np.abs(b)
    return (a * b < 0) & (r > 0.25) & (r < 4.0)


def adam_inputs(D, t):
    """Crafted (p, m, v, g), flat over a senet(D, 4)'s four tensors, for Adam step `t`: magnitudes spread over nine decades
    (v: eighteen) with both signs, every seventh gradient exactly zero, blocks with g = m = v = 0 (there p moves by the
    weight-decay term alone), a block with v = 0 and g != 0; at t = 1 the moments are zero.
    Every intermediate of the update is then zero or a normal fp32 value -- the smallest non-zero square is
    (1 - beta2) (wd p)^2 >= 1e-3 * (1e-4 * 1e-9)^2 = 1e-29, far above 1e-37, unless g * grad_scale and wd * p cancel to
    their last bits, which test_adam_restatement_cpu.py checks they do not: denormal handling is not what these inputs
    are for.  Computed once per (D, t); read-only."""
    if (D, t) not in _adam_inputs:
        n = adam_numel(D)
        rng = np.random.default_rng([2024, D, t])

        def spread(lo, signed=True):
            x = 10.0 ** rng.uniform(lo, 0.0, n)
            return (x * rng.choice([-1.0, 1.0], n) if signed else x).astype(np.float32)
        p, m, v, g = spread(-9), spread(-9), spread(-18, signed=False), spread(-9)
        # No sum of the update cancels by more than (1 + 4) / (4 - 1) = 5/3 under any tested hyper-parameters: a sum that
        # cancels a thousandfold carries its operands' rounding a thousandfold into what follows (g * g, the update), and
        # the error in ulps of exp_avg_sq or of the update would then measure the input, not the arithmetic.
        #   g * grad_scale + wd * p: where the two oppose within a factor of four of one another, g takes p's sign
        #   beta1 * m + (1 - beta1) * g: where they do, m takes the other sign, or (if that opposes under other
        #   hyper-parameters) sixteen times the magnitude
        p64, wds = p.astype(np.float64), sorted({hp[4] for hp in ADAM_HP})
        for wd, gs in itertools.product(wds[1:], ADAM_GRAD_SCALES):
            g = np.where(_adam_cancels(g * np.float64(gs), wd * p64), -g, g)
        g[::7] = 0.0
        g[ADAM_V0_BLOCK] = np.where(g[ADAM_V0_BLOCK] == 0.0, np.copysign(np.float32(1e-3), p[ADAM_V0_BLOCK]), g[ADAM_V0_BLOCK])
        for blk in adam_zero_blocks(D):
            g[blk] = 0.0
        for _ in range(8):
            terms = [((1.0 - hp[1]) * (g * np.float64(gs) + wd * p64), hp[1])
                     for hp, wd, gs in itertools.product(ADAM_HP, wds, ADAM_GRAD_SCALES)]
            bad = lambda mm: np.any([_adam_cancels(a, b1 * mm) for a, b1 in terms], axis=0)
            bad_now, bad_flipped = bad(m.astype(np.float64)), bad(-m.astype(np.float64))
            m = np.where(bad_now & ~bad_flipped, -m, np.where(bad_now & bad_flipped, m * np.float32(16.0), m))
        v[ADAM_V0_BLOCK] = 0.0
        for blk in adam_zero_blocks(D):
            m[blk] = v[blk] = 0.0
        if t == 1:
            m[:] = 0.0
            v[:] = 0.0
        for a in (p, m, v, g):
            a.setflags(write=False)
        _adam_inputs[(D, t)] = (p, m, v, g)
    return _adam_inputs[(D, t)]


# ---- the gradient-only step (moc_train_grad) against autograd on the oracle: test_gpu_parity.py, test_gpu_step_lds.py
GRAD_STEP_TOPJ, GRAD_STEP_SIZES = 40, (700, 900, 800)
_grad_step_tasks = {}


def grad_step_task(C, K, D, dtype):
    """Bank, three slides in `dtype`, labels, and autograd's gradients of the oracle's loss for each slide (computed once
    per shape)."""
    from oracle import moc_oracle as O
    key = (C, K, D, dtype)
    if key not in _grad_step_tasks:
        W, We = synth.make_bank(600 + C, D, C)
        bags, labels = synth.make_slide_set(6600 + C, list(GRAD_STEP_SIZES), D, We, C)
        bags = [b.to(dtype) for b in bags]
        torch.manual_seed(9)
        ref = O.Senet(D, 4)
        exp = []
        for bag, label in zip(bags, labels):
            sr = O.slide_process(bag.to(torch.float32), W, We, C, GRAD_STEP_TOPJ, mask=None)
            pooled = O.pool_top(O.mix_train(ref(sr["selected_feat"]), sr), [K])[1][K]
            loss = torch.nn.functional.cross_entropy(pooled, torch.tensor([label]))
            grads = torch.autograd.grad(loss, list(ref.parameters()))
            exp.append(torch.cat([t.reshape(-1) for t in grads]).numpy())
        _grad_step_tasks[key] = (W, We, bags, labels, exp)
    return _grad_step_tasks[key]


def grad_step_batch(dev, C, K, D, dtype, masked=False, adam=None):
    """The task's slides as a batch after phase A, its labels on the device and a meta-learner initialised as the oracle's.
    masked: the batch carries a mask of ones -- the same rows, but a batch that trains, for which the engine allocates the
    forward's tile records (engine.TILE_RECORDS).  adam: keywords of a torch.optim.Adam over the model, which the
    meta-learner then steps (default: none, gradients only)."""
    from moc_amd import engine as E, main_moc as M
    W, We, bags, labels, _ = grad_step_task(C, K, D, dtype)
    torch.manual_seed(9)
    model = M.senet(D, 4).to(dev)
    M.set_classifier_bank(W.to(dev), We.to(dev))
    X, sz = M._pack(bags, dev, dtype)
    mask = torch.ones(sum(GRAD_STEP_SIZES), dtype=torch.uint8) if masked else None
    batch = E.SlideBatch(X, sz, C, C + 4, GRAD_STEP_TOPJ, K, [], mask=mask)
    batch.phase_a(E.Bank.get(M.zeroshot_weights, M.zeroshot_weights_ext, dtype, dev))
    lab = torch.tensor(labels, dtype=torch.int64, device=dev)
    opt = torch.optim.Adam(model.parameters(), **adam) if adam is not None else None
    return batch, lab, E.MetaState(model, opt, need_grads=True)


def grad_step_grads(batch, lab, meta):
    """moc_train_grad slide by slide -> (the flat gradients, what the step left in n_pair[0]) per slide"""
    from moc_amd import engine as E
    out = []
    for s_i in range(len(GRAD_STEP_SIZES)):
        E.train_grad(batch, meta, lab, s_i, 15)
        got = torch.cat([t.reshape(-1) for t in meta.grads]).cpu().numpy()
        out.append((got, int(batch.meta_ws()[0]["n_pair"].cpu()[0])))
    return out


def assert_grad_step_matches_autograd(got, C, K, D, dtype):
    for (g, _), exp in zip(got, grad_step_task(C, K, D, dtype)[4]):
        np.testing.assert_allclose(g, exp, atol=2e-6, rtol=1e-4)
