"""The tile-record step (pool_w1_step_tiles_kernel) releases the row requests once the winners are known: a class wave
ends with the winners' stores; the fourth wave forms the pooled means itself behind the barrier (lane c: class c, the
logits never pass through pooled_s) and the publishing workgroup's fourth wave stores the slide's outputs last.  The cases
also hold what ranks the candidates and sums the gradients to the same bits at the pair counts (20, 24, 25, 63), class
counts and ties where another form of those loops would change path.

Every comparison is bit for bit against the same passes with the tile records off (engine.TILE_RECORDS = False: the step
is pool_w1_step_kernel, which none of this touches): losses, predicted classes, pooled logits, pooled rows, selected
counts, parameters and both Adam moments.  A case that is not about the fall-back asserts the marker of the records path
on every pass -- the marker is the LAST step's of a pass, so every such case ends its slide list with a slide the records
serve.

Not here: a slide whose strongest mixed score is stored as -0.0.  It needs every other score of a class below zero and
the gates' products of one zero row all negative zeros, which was not built on the CPU for this file.  The chain of
additions that case would exercise starts at 0.f and adds exactly k values, with no padding term, as before."""
import numpy as np
import pytest
import torch

import helpers as H
from moc_amd import synth

pytestmark = pytest.mark.gpu

RECORDS, FULL = 1000001, 1000002      # MOC_TILE_PATH_RECORDS / MOC_TILE_PATH_FULL


@pytest.fixture(scope="module")
def dev(gpu_device):
    return gpu_device


def _passes(dev, tile_records, C, D, dtype, sizes, j, K, epochs, seed, plant=None):
    """`epochs` passes of main_moc.train over a resident split (labels i % C) with the tile-record step on or off ->
    everything a step leaves behind, as host arrays; and the selected-row counts of every pass."""
    from moc_amd import engine as E, main_moc as M
    keep = E.TILE_RECORDS
    E.TILE_RECORDS = tile_records
    try:
        W, We = synth.make_bank(seed, D, C)
        bags, labels = synth.make_slide_set(seed + 100, sizes, D, We, C)
        if plant is not None:
            bags = [plant(i, b_, We) for i, b_ in enumerate(bags)]
        M.set_classifier_bank(W.to(dev), We.to(dev))
        torch.manual_seed(seed)
        model = M.senet(D, 4).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
        res = M.ResidentBags([b_.to(dtype) for b_ in bags], labels, dev)
        args = H.make_args(C, j, K)
        torch.manual_seed(seed + 7)
        out = {"loss": [], "pred": [], "pooled": [], "topk": [], "path": [], "n_sel": []}
        for _ in range(epochs):
            M.train(model, res, opt, dev, args)
            torch.cuda.synchronize()
            batch = M.train.last[0]
            t = batch.meta_ws()[0]
            out["loss"].append(t["loss"].cpu().numpy().copy())
            out["pred"].append(t["pred"].cpu().numpy().copy())
            out["pooled"].append(t["pooled"].cpu().numpy().copy())
            out["topk"].append(t["topk_idx"].cpu().numpy().copy())
            out["path"].append(int(t["n_pair"].cpu()[0]))
            out["n_sel"].append(batch.n_sel.cpu().numpy().copy())
        out["params"] = H.flat_params(model)
        out["m"], out["v"] = H.flat_state(opt, "exp_avg"), H.flat_state(opt, "exp_avg_sq")
        return out
    finally:
        E.TILE_RECORDS = keep


def _same_bits(a, b, epochs):
    for e in range(epochs):
        np.testing.assert_array_equal(a["loss"][e], b["loss"][e], err_msg=f"pass {e}: losses")
        np.testing.assert_array_equal(a["pred"][e], b["pred"][e], err_msg=f"pass {e}: predicted classes")
        np.testing.assert_array_equal(a["pooled"][e], b["pooled"][e], err_msg=f"pass {e}: pooled logits")
        np.testing.assert_array_equal(a["topk"][e], b["topk"][e], err_msg=f"pass {e}: pooled rows")
        np.testing.assert_array_equal(a["n_sel"][e], b["n_sel"][e], err_msg=f"pass {e}: selected rows")
    for k in ("params", "m", "v"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert all(p not in (RECORDS, FULL) for p in a["path"])        # the reference: pool_w1_step_kernel leaves no marker


def _both(dev, C, D, dtype, sizes, j, K, epochs, seed, plant=None):
    a = _passes(dev, False, C, D, dtype, sizes, j, K, epochs, seed, plant)
    b = _passes(dev, True, C, D, dtype, sizes, j, K, epochs, seed, plant)
    _same_bits(a, b, epochs)
    return b


# ------------------------------------------------------------------ pairs, classes on the fourth wave, lengths of the sum
@pytest.mark.parametrize("C,K,D,dtype,sizes,j", [
    # P = 20, the benchmark's pair count: no class on the fourth wave, it only forms the two means
    (2, 10, 512, torch.float32, [2600, 1500, 2200], 300),
    (2, 10, 256, torch.float32, [1500, 2600, 1800], 300),
    (2, 10, 256, torch.bfloat16, [2200, 1500, 2600], 300),
    # P = 24, six whole groups of four pairs in the gradient sum; the fourth wave pools class 3 in front of the barrier
    (4, 6, 256, torch.float32, [1500, 1200, 1700, 1600], 150),
    # P = 25, one pair past them; wave 0 pools classes 0 and 4
    (5, 5, 256, torch.float32, [1500, 1800, 2100, 1600, 2000], 100),
    # P = 63, and a slide of 12 rows in front: k = S < K can only fall back, the marker is the last slide's
    (7, 9, 256, torch.float32, [12, 1500, 1700, 1900], 80),
    # sixteen means formed by the fourth wave after it has pooled classes 3, 7, 11, 15; no padding lane in the cross entropy
    (16, 3, 256, torch.float16, [1500, 1600, 1700, 1800], 40),
    # the mean of one value
    (2, 1, 256, torch.float32, [900, 700, 1100], 100),
    # the longest sum the plan gives this kernel
    (5, 12, 256, torch.float32, [1500, 1700, 2000, 1600], 100),
])
def test_step_release_gives_the_full_score_steps_bits(dev, C, K, D, dtype, sizes, j):
    epochs = 3 if len(sizes) <= 3 else 2
    b = _both(dev, C, D, dtype, sizes, j, K, epochs, 10200 + 16 * C + K + D)
    assert b["path"] == [RECORDS] * epochs, b["path"]
    if min(sizes) < K:
        assert all((n_ < K).any() for n_ in b["n_sel"]), "no slide with k = S < K"


# ------------------------------------------------------------------ ties
def _pairs(i, bag, We):
    """Every odd row repeats the row in front of it: where the mask keeps both, two candidates share their score word
    and only the row in the key's low half orders them."""
    out = bag.clone()
    out[1::2] = out[0::2][: out[1::2].size(0)]
    return out


def test_step_release_two_way_ties(dev):
    b = _both(dev, 2, 256, torch.float32, [2400, 1800, 2600], 300, 10, 3, 10900, plant=_pairs)
    assert b["path"] == [RECORDS] * 3, b["path"]


def _pass_masks(seed, sizes, epochs):
    """The keep flags of every slide in every pass as _passes(seed) will see them: main_moc.train draws, slide after
    slide, what `torch.rand(n) > 0.5` gives from the CPU generator (engine.draw_row_masks), seeded with seed + 7."""
    state = torch.get_rng_state()
    torch.manual_seed(seed + 7)
    masks = [[torch.rand(n) > 0.5 for n in sizes] for _ in range(epochs)]
    torch.set_rng_state(state)
    return masks


CUT = dict(C=2, K=2, D=256, j=300, seed=11100, epochs=2, sizes=[1500, 1200, 500])


def _cut_rows():
    """Four rows of CUT's last slide that every pass keeps, more than sixteen kept rows apart in every pass (four
    different tiles), and their places among the kept rows of each pass."""
    masks = [m[-1] for m in _pass_masks(CUT["seed"], CUT["sizes"], CUT["epochs"])]
    always = torch.stack(masks).all(0).nonzero().flatten().tolist()
    gap = (len(always) - 6) // 3                                   # always-kept rows apart: as many kept ones, or more
    rows = always[5::gap][:4]
    places = [[int(m[:r].sum()) for r in rows] for m in masks]
    assert gap > 16 and len(rows) == 4 and all(len({p // 16 for p in ps}) == 4 for ps in places), places
    return rows, places, masks


def _across_the_cut(i, bag, We):
    """CUT's last slide: few enough rows that topj selects every kept row, so a tile is sixteen consecutive kept rows.
    One dominant row A and, below it, THREE identical rows B in three other tiles (all class directions at once; every
    other row points away from them).  The group maxima are A, then three that tie: the K-th (second) largest is B's
    score, the candidates of a class are A and the three B -- and the second and the third place tie."""
    if i != len(CUT["sizes"]) - 1:
        return bag
    rows, _, _ = _cut_rows()
    s = We[:, :CUT["C"]].sum(1)
    out = bag - 0.5 * s
    out[rows[0]] = s + 0.1 * bag[rows[0]]
    out[rows[1:]] = s + 0.5 * bag[rows[1]]
    return torch.nn.functional.normalize(out, dim=1)


def test_step_release_tie_across_the_cut(dev):
    """k = 2 of four candidates whose second, third and fourth keys share the score word: ranks on the score words alone
    would give all three the same place, the whole keys (low word ~row) give the place to the smallest row."""
    p = CUT
    b = _both(dev, p["C"], p["D"], torch.float32, p["sizes"], p["j"], p["K"], p["epochs"], p["seed"], plant=_across_the_cut)
    assert b["path"] == [RECORDS] * p["epochs"], b["path"]
    _, places, masks = _cut_rows()
    for e in range(p["epochs"]):
        assert int(b["n_sel"][e][-1]) == int(masks[e].sum())       # every kept row selected: the tiles are the planted ones
        top = b["topk"][e].reshape(len(p["sizes"]), p["C"], p["K"])[-1]
        for c in range(p["C"]):
            assert top[c].tolist() == places[e][:2], (e, c, top[c], places[e])   # A, then the FIRST of the three


# ------------------------------------------------------------------ the fall-back: the fourth wave takes pooled_s from LDS
def _flat_top(i, bag, We):
    """Two hundred rows of ONE strong vector: the group maxima tie, the bound is void (T0 = 0), every record of the class
    is a candidate -- more than the list's sixty-four places."""
    out = bag.clone()
    v = torch.nn.functional.normalize(0.2 * bag[0] + 3.0 * We[:, 0], dim=0)
    out[5::out.size(0) // 200][:200] = v
    return out


def _sixteen(i, bag, We):
    """Sixteen consecutive rows that carry the class signal: one tile holds more than four of the pooled rows (rho >= T0)."""
    out = bag.clone()
    out[32:48] = torch.nn.functional.normalize(out[32:48] * 0.2 + 3.0 * We[:, 0], dim=1)
    return out


@pytest.mark.parametrize("plant", [_flat_top, _sixteen])
def test_step_release_falls_back_with_the_same_bits(dev, plant):
    b = _both(dev, 2, 256, torch.float32, [2600, 2200, 2400], 300, 10, 2, 11300, plant=plant)
    assert b["path"] == [FULL] * 2, b["path"]


# ------------------------------------------------------------------ batched runs
def _task(run, n, C, D, dtype):
    W, We = synth.make_bank(79 + C, D, C)                       # the runs share the classifier bank
    g = np.random.default_rng(1900 + run)
    sizes = [int(v) for v in g.integers(1200, 2600, size=n)]
    bags, labels = synth.make_slide_set(11700 + 41 * run, sizes, D, We, C)
    return W, We, [b_.to(dtype) for b_ in bags], labels


def _alone(dev, run, n, C, D, dtype, j, K, epochs, lr):
    """Run `run` by main_moc.train, its steps by pool_w1_step_kernel (tile records off)."""
    from moc_amd import engine as E, main_moc as M
    keep = E.TILE_RECORDS
    E.TILE_RECORDS = False
    try:
        W, We, bags, labels = _task(run, n, C, D, dtype)
        M.set_classifier_bank(W.to(dev), We.to(dev))
        torch.manual_seed(400 + run)
        model = M.senet(D, 4).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=1e-4)
        res = M.ResidentBags(bags, labels, dev)
        args = H.make_args(C, j, K)
        torch.manual_seed(7300 + run)                           # the run's mask stream
        losses = []
        for _ in range(epochs):
            M.train(model, res, opt, dev, args)
            torch.cuda.synchronize()
            losses.append(M.train.last[0].meta_ws()[0]["loss"].cpu().numpy().copy())
        return H.flat_params(model), H.flat_state(opt, "exp_avg"), H.flat_state(opt, "exp_avg_sq"), losses
    finally:
        E.TILE_RECORDS = keep


@pytest.mark.parametrize("per_run_adam", [False, True])
def test_step_release_in_three_batched_runs(dev, per_run_adam):
    from moc_amd import main_moc as M
    R, n, C, D, dtype, j, K, epochs = 3, 3, 2, 256, torch.float32, 300, 10, 2
    lrs = [1e-3 * (1 + r) if per_run_adam else 1e-3 for r in range(R)]
    alone = [_alone(dev, r, n, C, D, dtype, j, K, epochs, lrs[r]) for r in range(R)]
    models, opts, splits, gens = [], [], [], []
    for r in range(R):
        W, We, bags, labels = _task(r, n, C, D, dtype)
        M.set_classifier_bank(W.to(dev), We.to(dev))
        torch.manual_seed(400 + r)
        model = M.senet(D, 4).to(dev)
        models.append(model)
        opts.append(torch.optim.Adam(model.parameters(), lr=lrs[r], weight_decay=1e-4))
        splits.append(M.ResidentBags(bags, labels, dev))
        g = torch.Generator()
        g.manual_seed(7300 + r)
        gens.append(g)
    args = H.make_args(C, j, K)
    losses = []
    for _ in range(epochs):
        rs = M.train_runs(models, splits, opts, dev, args, generators=gens, per_run_adam=per_run_adam)
        torch.cuda.synchronize()
        losses.append(rs.losses().cpu().numpy().copy())
    assert rs.mode == 1 and len(rs.groups) == 1                 # one lockstep chain of tile-record steps
    assert int(rs.last[0].meta_ws()[0]["n_pair"].cpu()[0]) == RECORDS   # (batched: the largest code of any step)
    for r in range(R):
        p, m, v, ls = alone[r]
        np.testing.assert_array_equal(H.flat_params(models[r]), p, err_msg=f"run {r}: parameters")
        np.testing.assert_array_equal(H.flat_state(opts[r], "exp_avg"), m, err_msg=f"run {r}: exp_avg")
        np.testing.assert_array_equal(H.flat_state(opts[r], "exp_avg_sq"), v, err_msg=f"run {r}: exp_avg_sq")
        for e in range(epochs):
            np.testing.assert_array_equal(losses[e][r], ls[e], err_msg=f"run {r} pass {e}: losses")
