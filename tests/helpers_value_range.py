"""Inputs, float64 references and rules of the value-range tests (test_gpu_value_range.py, test_value_range_cpu.py):
rows and banks OFF the unit sphere.  Test-side only; nothing here needs a GPU.

Two kinds of check:
  * exact ones -- a row times 2^s is exact in its storage type, every product and every fp32 accumulation then scales
    exactly, so every statistic of degree one scales exactly, whatever the summation order: compared as bits;
  * bounded ones -- the project's unit-sphere tolerance (TIGHT and its multiples, helpers.ATOL, 2e-6 + 1e-4 |g| for
    gradients) carried to the scale by that exactness, or widened by a noise figure MEASURED ON THE REFERENCE ALONE
    (measured_allowed): four times the distance between the oracle run in float32 and the oracle run in float64."""
from __future__ import annotations

import copy
import types

import numpy as np
import torch

from moc_amd import synth

TIGHT = 2e-6                                   # test_gpu_parity.TIGHT: fp32 re-association noise on O(1) cosine logits
# multiples of TIGHT per statistic, as test_scores_and_row_stats_match_oracle has them: logits, gap, bg_sum, bg_max
TIGHT_MULT = {"logits": 1.0, "gap": 2.0, "bg_sum": 4.0, "bg_max": 1.0}
POW2_WIDE = (-20, -7, -1, 1, 6, 20)            # fp32 and bf16 storage: eight exponent bits, nothing near either end
POW2_F16 = (1, 4, 8)                           # fp16 storage: upscaling only (downscaling rounds subnormals away)
POW2_BANK = (-6, -1)
ODD_SCALES = (0.3, 5.0, 23.0)


def scaled_pow2(xs: torch.Tensor, s: int) -> torch.Tensor:
    """xs * 2^s in xs's own storage type; asserts that the scaling was exact (no overflow, nothing rounded away)."""
    y = (xs.to(torch.float32) * float(2.0 ** s)).to(xs.dtype)
    assert torch.equal(y.to(torch.float64), xs.to(torch.float64) * float(2.0 ** s)), f"2^{s} is not exact on this {xs.dtype} input"
    return y


def next_pow2(v):
    """The power of two at or above v (> 0), elementwise, float64."""
    v = np.asarray(v, dtype=np.float64)
    return np.exp2(np.ceil(np.log2(v)))


def row_factors(n: int, seed: int, lo=0.01, hi=30.0) -> torch.Tensor:
    """A different factor per row, log-uniform in [lo, hi], fp32 [n, 1]."""
    r = np.random.default_rng(seed)
    return torch.from_numpy(np.exp(r.uniform(np.log(lo), np.log(hi), n)).astype(np.float32)).unsqueeze(1)


def degree_one_rows(C: int):
    """Rows of the full statistics layout that are homogeneous of degree one in the bag row: logits, gap, bg_sum, bg_max."""
    return list(range(C)) + [2 * C, 2 * C + 1, 2 * C + 2]


def stats64(x: torch.Tensor, W: torch.Tensor, We: torch.Tensor, C: int) -> torch.Tensor:
    """The score pass's [2C+3, N] statistics (include/moc_hip.h: logits | softmax | gap | bg_sum | bg_max) of the rows x in
    float64: logits from W, background from W_ext[:, C:] (main_moc.py:336-337)."""
    x, W, We = x.to(torch.float64), W.to(torch.float64), We.to(torch.float64)
    lg = x @ W
    bg = (x @ We)[:, C:]
    two = torch.topk(lg, 2, dim=1)[0]
    return torch.cat([lg.t(), torch.softmax(lg, dim=1).t(), (two[:, 0] - two[:, 1]).abs().unsqueeze(0),
                      bg.sum(dim=1).unsqueeze(0), bg.max(dim=1)[0].unsqueeze(0)], 0)


def softmax64(logits32: torch.Tensor) -> torch.Tensor:
    """float64 softmax over dim 0 of fp32 logits [C, N] (the kernel's own logits: the check is of the softmax alone)."""
    return torch.softmax(logits32.to(torch.float64), dim=0)


def select_rule(st: torch.Tensor, C: int, j: int, discard=()):
    """The project's selection rule restated (test_gpu_parity.test_select_ties_take_lowest_rows; moc_select.hip): per key
    column the min(j, n) rows first in the order (key descending, row ascending), the union over the columns of every
    selector that is not discarded, ascending.  st: [2C+3, n] statistics of ONE slide's kept rows, full layout.  Key
    columns: the C logits (topk), the C softmax columns (delta_softmax), the gap (delta_diff), minus the background sum
    (bottomk: smallest background first).  -0 and +0 tie, as in the kernel's key (moc_key_desc)."""
    st = st.to(torch.float64)
    n = st.size(1)
    cols = []
    if "topk" not in discard:
        cols += [st[c] for c in range(C)]
    if "delta_softmax" not in discard:
        cols += [st[C + c] for c in range(C)]
    if "delta_diff" not in discard:
        cols.append(st[2 * C])
    if "bottomk" not in discard:
        cols.append(-st[2 * C + 1])
    chosen = set()
    for col in cols:
        v = col.tolist()
        chosen.update(sorted(range(n), key=lambda i: (-v[i], i))[:min(j, n)])
    return sorted(chosen)


def boundary_ties(st: torch.Tensor, C: int, j: int) -> int:
    """How many of select_rule's key columns have rows j and j+1 (in key order) on EQUAL keys: a tie across the boundary,
    which only the row order decides."""
    st = st.to(torch.float64)
    n = st.size(1)
    if n <= j:
        return 0
    cols = [st[c] for c in range(2 * C + 1)] + [-st[2 * C + 1]]
    hit = 0
    for col in cols:
        srt = torch.sort(col, descending=True)[0]
        hit += int(srt[j - 1] == srt[j])
    return hit


def keys_of(st: torch.Tensor, C: int) -> dict:
    """helpers.ambiguous_rows' key dict from one slide's [2C+3, n] statistics."""
    return {"top": st[:C].t(), "softmax": st[C:2 * C].t(), "gap": st[2 * C].unsqueeze(1), "lowbg": (-st[2 * C + 1]).unsqueeze(1)}


def slot_ranges(sizes, mask=None):
    """[(first slot, kept rows, kept row indices inside the slide)] per slide: slot base + t holds the t-th kept row."""
    out, off = [], 0
    for n in sizes:
        kept = torch.arange(n) if mask is None else torch.nonzero(mask[off:off + n].to(torch.bool)).flatten()
        out.append((off, len(kept), kept))
        off += n
    return out


def half_mask(total: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand(total, generator=g) > 0.5).to(torch.uint8)
    m[0] = 1                                         # (test_gpu_parity: the first slide keeps a row)
    return m


def repeated_rows(seed: int, D: int, We: torch.Tensor, C: int, n: int = 100) -> torch.Tensor:
    """ONE synthetic row, n times."""
    return synth.make_bag(seed, 1, D, We, C, label=0).repeat(n, 1).contiguous()


ZERO_HEAD, ZERO_TAIL = 40, 7


def zero_block_slide(seed: int, n_mid: int, D: int, We: torch.Tensor, C: int) -> torch.Tensor:
    """A slide whose first 40 and last 7 rows are all zeros, with n_mid ordinary rows between."""
    mid = synth.make_bag(seed, n_mid, D, We, C, label=1)
    return torch.cat([torch.zeros(ZERO_HEAD, D), mid, torch.zeros(ZERO_TAIL, D)]).contiguous()


def unequal_bank(seed: int, D: int, C: int):
    """A bank whose column norms run from 0.25 to 1.5 (every |w| < 2: the fp16 image takes it), W_ext[:, :C] == W."""
    _, We = synth.make_bank(seed, D, C)
    We = (We * torch.linspace(0.25, 1.5, We.size(1)).unsqueeze(0)).contiguous()
    assert float(We.abs().max()) < 2.0
    return We[:, :C].contiguous(), We


# ---- the measured rule: meta forward, pooling, cross entropy and gradients at scale, against the oracle in float64 ------
GRAD_C, GRAD_D, GRAD_K, GRAD_TOPJ = 2, 256, 10, 400          # topj above every slide: all rows selected, selection cannot differ
GRAD_SIZES, GRAD_LABELS = (300, 120), (1, 0)
GRAD_BANK_SEED, GRAD_BAG_SEED, GRAD_MODEL_SEED = 9, 372, 3     # (bag seed 72 misses the top-K precondition at 2^-6: 449 x the noise)
GRAD_SCALES = (2.0 ** -6, 1.0 / 8, 5.0, 32.0, 200.0)
FWD_SCALES = (2.0 ** -6, 0.3, 5.0, 32.0)
_grad_cases = {}


def _oracle_run(model, xs, labels, W, We, dt):
    from oracle import moc_oracle as O
    out = []
    params = list(model.parameters())
    W1, b1 = params[0].detach(), params[1].detach()
    for x, label in zip(xs, labels):
        x = x.to(dt)
        sr = O.slide_process(x, W.to(dt), We.to(dt), GRAD_C, GRAD_TOPJ, mask=None)
        assert sr["selected_index"] == list(range(x.size(0)))
        gates = model(sr["selected_feat"])
        mixed = O.mix_train(gates, sr)
        pooled = O.pool_top(mixed, [GRAD_K])[1][GRAD_K]
        loss = torch.nn.functional.cross_entropy(pooled, torch.tensor([label]))
        grads = torch.autograd.grad(loss, params)
        out.append(types.SimpleNamespace(
            gates=gates.detach().to(torch.float64).numpy(), mixed=mixed.detach().to(torch.float64).numpy(),
            pooled=pooled.detach().to(torch.float64).numpy()[0], loss=float(loss.detach()), pred=int(pooled.detach().argmax()),
            grads=[g.to(torch.float64).numpy() for g in grads], pre=(x @ W1.t() + b1).to(torch.float64).numpy()))
    return out


def grad_case(dtype: torch.dtype, scale: float):
    """Bank, two slides (rows times `scale`, rounded to `dtype`: the rounded rows ARE the input), labels, the meta-learner's
    initial state dict, and the oracle's forward, loss and autograd gradients per slide, run twice on the CPU: in float64
    (`ref`, double model and double inputs) and in float32 (`ref32`).  Computed once per (dtype, scale); read-only."""
    from oracle import moc_oracle as O
    key = (dtype, float(scale))
    if key not in _grad_cases:
        W, We = synth.make_bank(GRAD_BANK_SEED, GRAD_D, GRAD_C)
        xs = [(synth.make_bag(GRAD_BAG_SEED + i, n, GRAD_D, We, GRAD_C, label=GRAD_LABELS[i]) * np.float32(scale)).to(dtype)
              for i, n in enumerate(GRAD_SIZES)]
        torch.manual_seed(GRAD_MODEL_SEED)
        m32 = O.Senet(GRAD_D, 4)
        m64 = copy.deepcopy(m32).double()
        state = {k: v.clone() for k, v in m32.state_dict().items()}
        ref = _oracle_run(m64, xs, GRAD_LABELS, W, We, torch.float64)
        ref32 = _oracle_run(m32, xs, GRAD_LABELS, W, We, torch.float32)
        _grad_cases[key] = types.SimpleNamespace(W=W, We=We, xs=xs, labels=list(GRAD_LABELS), state=state, ref=ref, ref32=ref32,
                                                 scale=float(scale), dtype=dtype)
    return _grad_cases[key]


def measured_allowed(base_abs: float, base_rel: float, t32, t64):
    """The measured rule.  Allowed error of an output or gradient tensor, elementwise:
        base_abs + base_rel |t64|  +  4 max|t32 - t64|
    -- the project's existing tolerance for that output plus four times the reference's own fp32 noise on this very
    tensor (both oracle runs on the CPU: the measurement is of the reference alone).  Four: two independent fp32
    roundings of that size, times two for a different summation order."""
    t32, t64 = np.asarray(t32, dtype=np.float64), np.asarray(t64, dtype=np.float64)
    return base_abs + base_rel * np.abs(t64) + 4.0 * float(np.abs(t32 - t64).max())


def grad_noise(case):
    """max|g32 - g64| / max|g64| over the four gradient tensors together, per slide."""
    out = []
    for r32, r64 in zip(case.ref32, case.ref):
        g32, g64 = (np.concatenate([g.ravel() for g in r.grads]) for r in (r32, r64))
        out.append(float(np.abs(g32 - g64).max() / np.abs(g64).max()))
    return out


def grad_case_margins(case):
    """The preconditions' figures per slide: (smallest distance between a class's K-th and (K+1)-th mixed score,
    max|mixed32 - mixed64|, smallest |pre-activation| over the pooled rows' 64 hidden units), all from the float64 run."""
    out = []
    for r32, r64 in zip(case.ref32, case.ref):
        srt = -np.sort(-r64.mixed, axis=0)
        gap = float((srt[GRAD_K - 1] - srt[GRAD_K]).min())
        noise = float(np.abs(r32.mixed - r64.mixed).max())
        pooled_rows = np.unique(np.argsort(-r64.mixed, axis=0, kind="stable")[:GRAD_K].ravel())
        out.append((gap, noise, float(np.abs(r64.pre[pooled_rows]).min())))
    return out
