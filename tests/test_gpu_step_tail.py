"""The tile-record step's tail (pool_w1_step_tiles_kernel): list positions by ballot, the pooled mean from one LDS read,
the cross entropy's butterflies by DPP, and the fourth wave forming dz / dh of the pairs under its own round trip.

Every comparison is bit for bit against the same passes with the tile records off (engine.TILE_RECORDS = False: the step
is pool_w1_step_kernel, which none of this touches): losses, pooled logits, pooled rows, parameters and both Adam
moments.  A case that is not about the fall-back asserts the path marker of the records path -- it must not pass by
ranking the full scores inside the kernel.  The marker is the LAST step's of a pass, so every such case ends its slide
list with a slide the records serve."""
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


def _passes(dev, tile_records, C, D, dtype, sizes, j, K, epochs, seed, discard=(), plant=None):
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
        args = H.make_args(C, j, K, discard)
        torch.manual_seed(seed + 7)
        out = {"loss": [], "pred": [], "pooled": [], "topk": [], "path": [], "n_sel": [], "labels": labels}
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


def _both(dev, C, D, dtype, sizes, j, K, epochs, seed, discard=(), plant=None):
    a = _passes(dev, False, C, D, dtype, sizes, j, K, epochs, seed, discard, plant)
    b = _passes(dev, True, C, D, dtype, sizes, j, K, epochs, seed, discard, plant)
    _same_bits(a, b, epochs)
    return b


# ------------------------------------------------------------------ class counts, pairs per wave, small k
@pytest.mark.parametrize("C,K,D,dtype,sizes,j,discard", [
    # class counts: odd ones leave padding lanes in the butterflies, C >= 4 leaves no wave without a class to pool; the
    # label (i % C) takes every class position.  (Shapes the step plan gives the tile-record kernel: C * K * D <= 20,480
    # and the LDS of the narrow step, which ends at 62 pairs for sixteen classes.)
    (2, 10, 512, torch.float32, [2600, 1500, 3000], 300, ()),
    (3, 10, 256, torch.bfloat16, [2000, 2600, 1500], 200, ()),
    (5, 8, 256, torch.float32, [1500, 1800, 2100, 1600, 2000], 100, ()),
    (7, 9, 256, torch.float32, [1500, 1700, 12, 1900, 1600, 2100, 1800], 80, ()),   # P = 63; the slide of 12 rows: k = S < K
    (16, 3, 256, torch.float16, [1500 + 100 * (i % 4) for i in range(16)], 40, ()),  # sixteen logits: no padding lane (P = 48)
    # small k: K = 1; slides of a tile or two with S < K in front of one the records serve
    (2, 1, 256, torch.float16, [900, 700, 1100], 100, ()),
    (2, 1, 256, torch.float32, [900, 700, 12], 100, ()),        # ... and a slide of ONE tile that the records serve (K = 1 only)
    (2, 10, 512, torch.float32, [40, 18, 9, 1500], 400, ()),
    (5, 12, 256, torch.float32, [1500, 12, 1700, 2000, 1600], 100, ()),              # a long chain of the pooled sum; P = 60
    # the dz selection (use_bits)
    (2, 10, 512, torch.bfloat16, [2500, 1500, 2000], 300, ("delta_diff",)),
    (4, 5, 256, torch.float32, [1500, 1200, 1700, 1600], 150, ("topk",)),
    (3, 10, 256, torch.float32, [1800, 1500, 2200], 200, ("delta_softmax", "bottomk")),
])
def test_step_tail_gives_the_full_score_steps_bits(dev, C, K, D, dtype, sizes, j, discard):
    """(The marker proves the records path for the LAST slide of every pass only: a step overwrites it.  The slides in
    front of it are random ones of the same kind, and the small ones -- S < K -- can only fall back.)"""
    epochs = 3 if len(sizes) <= 8 else 2
    b = _both(dev, C, D, dtype, sizes, j, K, epochs, 8200 + 16 * C + K, discard)
    assert set(b["labels"]) == set(range(C))                      # the label takes every class position
    assert b["path"] == [RECORDS] * epochs, b["path"]
    n_sel = np.concatenate(b["n_sel"])
    assert ((((n_sel + 15) // 16) * 4) % 64 != 0).any()           # a last sixty-four of records that is not full
    if min(sizes) < 100 and K > 1:
        assert (n_sel < K).any(), "no slide with k = S < K"
    if sizes[-1] == 12:
        assert all(0 < s_[-1] <= 16 for s_ in b["n_sel"]), b["n_sel"]       # the last step's slide: a single tile


def _pass_masks(seed, sizes, epochs):
    """The keep flags of every slide in every pass as _passes(seed) will see them: main_moc.train draws, slide after slide,
    what `torch.rand(n) > 0.5` gives from the CPU generator (engine.draw_row_masks), seeded with seed + 7."""
    state = torch.get_rng_state()
    torch.manual_seed(seed + 7)
    masks = [[torch.rand(n) > 0.5 for n in sizes] for _ in range(epochs)]
    torch.set_rng_state(state)
    return masks


def _one_to_four_per_tile(masks):
    """Rows of a slide such that under EVERY one of `masks` (one per pass) each tile of sixteen kept rows holds at least one
    and at most four of them.  Greedy, rows kept in all passes first; the result is checked."""
    tile = [torch.where(m, (torch.cumsum(m.long(), 0) - 1) // 16, torch.full_like(m, -1, dtype=torch.long)).tolist() for m in masks]
    count = [[0] * (int(m.sum() + 15) // 16) for m in masks]
    rows = []
    n = masks[0].numel()
    for everywhere in (True, False):
        for i in range(n):
            ts = [(e, tile[e][i]) for e in range(len(masks)) if tile[e][i] >= 0]
            if i in rows or not ts or (everywhere and len(ts) < len(masks)):
                continue
            if any(count[e][t] == 0 for e, t in ts) and all(count[e][t] < 4 for e, t in ts):
                rows.append(i)
                for e, t in ts:
                    count[e][t] += 1
    assert all(1 <= c <= 4 for cs in count for c in cs), count
    return sorted(rows)


P64 = dict(C=4, K=16, D=256, j=300, seed=8800, epochs=3, sizes=[1734, 1700, 502])


def _sixteen_tiles(i, bag, We):
    """The last slide of P64: few enough rows that topj selects every kept row -- sixteen tiles, one per group, 64 records
    per class -- and one to four DOMINANT rows in every tile of every pass (all class directions at once; the other rows
    point away from them).  Then every group maximum is a dominant row, T0 is the smallest of them and no tile's fifth
    score reaches it: sixteen pooled rows per class from the records, with every record of the class a candidate at most."""
    if i != len(P64["sizes"]) - 1:
        return bag
    masks = [m[i] for m in _pass_masks(P64["seed"], P64["sizes"], P64["epochs"])]
    assert all(240 < int(m.sum()) <= 256 for m in masks), [int(m.sum()) for m in masks]
    s = We[:, :P64["C"]].sum(1)
    out = bag - 0.5 * s
    dom = _one_to_four_per_tile(masks)
    out[dom] = s + 0.3 * bag[dom]
    return torch.nn.functional.normalize(out, dim=1)


def test_step_tail_sixty_four_pairs(dev):
    """P = 64: every lane of the fourth wave owns a pair, the pooled sum is sixteen values long, all 64 ranked lanes leave
    operands.  The step plan gives the tile-record kernel ONE such shape, C = 4, K = 16 at D = 256 (C = 8, K = 8 and
    C = 16, K = 4 need 164 KiB of the narrow step's LDS and take another step).  With K = 16 the bound is the smallest of
    the sixteen group maxima, which on a random slide admits more than the list's 64 candidates: the last slide is built
    so that the records serve it (_sixteen_tiles)."""
    p = P64
    b = _both(dev, p["C"], p["D"], torch.float32, p["sizes"], p["j"], p["K"], p["epochs"], p["seed"], plant=_sixteen_tiles)
    masks = _pass_masks(p["seed"], p["sizes"], p["epochs"])
    for e in range(p["epochs"]):
        assert int(b["n_sel"][e][-1]) == int(masks[e][-1].sum())  # every kept row selected: the tiles are the planted ones
    assert b["path"] == [RECORDS] * p["epochs"], b["path"]


# ------------------------------------------------------------------ record counts: keys per lane
def _spread(bag, We):
    """Five groups of rows, one for each selector that can choose rows of its own (largest logit of class 0, of
    class 1, largest softmax of either, smallest background mass; the largest gaps are among the softmax's), shuffled, so
    that the selected rows are MORE than 3,072 of the 4,080 the selectors can name together.  Random slides stay near
    half of that: their selectors agree on most rows."""
    g = torch.Generator().manual_seed(4321)
    n = bag.size(0) // 5
    w0, w1, bg = We[:, 0], We[:, 1], We[:, 2:].sum(1)
    dirs = [3.0 * w0 + 2.5 * w1, 2.5 * w0 + 3.0 * w1, 0.5 * w0 - w1, 0.5 * w1 - w0, -0.5 * bg]
    out = bag.clone()
    for q, d_ in enumerate(dirs):
        out[q * n:(q + 1) * n] = d_ / d_.norm() + 0.15 * bag[q * n:(q + 1) * n]
    out = torch.nn.functional.normalize(out, dim=1)
    return out[torch.randperm(out.size(0), generator=g)]


@pytest.mark.parametrize("last", [16, 12])
def test_step_tail_twelve_and_sixteen_keys_per_lane(dev, last):
    """Slides whose selected rows need twelve (2,049 .. 3,072 rows) and sixteen (more) record keys per lane, each of them
    once as the LAST slide of the passes, whose marker is the one that is read.  In the first pass the host does not know
    the counts yet and every slide takes the bound's instantiation (680 x 6 rows: sixteen keys, the sixty-fours past the
    slide's records skipped)."""
    sizes, j, K = ([20, 9000, 8000] if last == 16 else [20, 8000, 9000]), 680, 10
    wide = sizes.index(8000)
    b = _both(dev, 2, 256, torch.float32, sizes, j, K, 3, 9100, plant=lambda i, bag, We: _spread(bag, We) if i == wide else bag)
    assert b["path"] == [RECORDS] * 3, b["path"]
    for e in range(3):
        s = b["n_sel"][e]
        assert 3072 < s[wide] <= 4096, s                           # VQ = 16
        assert 2048 < s[3 - wide] <= 3072, s                       # VQ = 12


# ------------------------------------------------------------------ ties
def _pairs(i, bag, We):
    """Every odd row repeats the row in front of it: where the mask keeps both, two records share their score word and
    only the row index in the key's low half orders them.  (Two-way ties, mostly inside a tile, are what the records
    path can hold: many-way ties make group maxima tie across the K-th place, the bound is void and the step falls back
    -- _few_values below.)"""
    out = bag.clone()
    out[1::2] = out[0::2][: out[1::2].size(0)]
    return out


@pytest.mark.parametrize("C,K,D,dtype,sizes,j", [
    (2, 10, 256, torch.float32, [2400, 1800, 3000], 300),
    (3, 8, 256, torch.bfloat16, [2000, 2600, 1600], 200),
])
def test_step_tail_with_tied_scores(dev, C, K, D, dtype, sizes, j):
    b = _both(dev, C, D, dtype, sizes, j, K, 3, 9300 + C, plant=_pairs)
    assert b["path"] == [RECORDS] * 3, b["path"]


# ------------------------------------------------------------------ candidates at the list's limit: the fall-back
def _flat_top(i, bag, We):
    """Two hundred rows of ONE strong vector: the group maxima tie, the bound is void (T0 = 0), every record of the class
    is a candidate -- more than the list's sixty-four places."""
    out = bag.clone()
    v = torch.nn.functional.normalize(0.2 * bag[0] + 3.0 * We[:, 0], dim=0)
    out[5::out.size(0) // 200][:200] = v
    return out


def _few_values(i, bag, We):
    """Every row one of eight rows: a class's scores take eight values, hundreds of keys share each score word."""
    return bag[torch.arange(bag.size(0)) % 8].clone()


def _sixteen(i, bag, We):
    """Sixteen consecutive rows that carry the class signal: one tile holds more than four of the pooled rows."""
    out = bag.clone()
    out[32:48] = torch.nn.functional.normalize(out[32:48] * 0.2 + 3.0 * We[:, 0], dim=1)
    return out


@pytest.mark.parametrize("plant", [_flat_top, _sixteen, _few_values])
def test_step_tail_falls_back_with_the_same_bits(dev, plant):
    b = _both(dev, 2, 512, torch.float32, [3000, 2500, 2800], 400, 10, 2, 9500, plant=plant)
    assert b["path"] == [FULL] * 2, b["path"]


# ------------------------------------------------------------------ batched runs
def _task(run, n, C, D, dtype):
    W, We = synth.make_bank(77 + C, D, C)                       # the runs share the classifier bank
    g = np.random.default_rng(900 + run)
    sizes = [int(v) for v in g.integers(1500, 3000, size=n)]
    bags, labels = synth.make_slide_set(9700 + 41 * run, sizes, D, We, C)
    return W, We, [b_.to(dtype) for b_ in bags], labels


def _alone(dev, run, n, C, D, dtype, j, K, epochs, discard, lr):
    """Run `run` by main_moc.train, its steps by pool_w1_step_kernel (tile records off)."""
    from moc_amd import engine as E, main_moc as M
    keep = E.TILE_RECORDS
    E.TILE_RECORDS = False
    try:
        W, We, bags, labels = _task(run, n, C, D, dtype)
        M.set_classifier_bank(W.to(dev), We.to(dev))
        torch.manual_seed(300 + run)
        model = M.senet(D, 4).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=1e-4)
        res = M.ResidentBags(bags, labels, dev)
        args = H.make_args(C, j, K, discard)
        torch.manual_seed(7100 + run)                           # the run's mask stream
        losses = []
        for _ in range(epochs):
            M.train(model, res, opt, dev, args)
            torch.cuda.synchronize()
            losses.append(M.train.last[0].meta_ws()[0]["loss"].cpu().numpy().copy())
        return H.flat_params(model), H.flat_state(opt, "exp_avg"), H.flat_state(opt, "exp_avg_sq"), losses
    finally:
        E.TILE_RECORDS = keep


@pytest.mark.parametrize("R,n,C,D,dtype,j,K,discard,per_run_adam", [
    (3, 3, 2, 512, torch.float32, 300, 10, (), False),                  # three runs: tail workgroups
    (4, 3, 2, 256, torch.float32, 200, 10, ("delta_diff",), False),     # four: tail_inside, ONE column block does both
    (4, 3, 4, 256, torch.bfloat16, 150, 5, (), False),                  # ... and no wave without a class
    (4, 3, 5, 256, torch.float32, 100, 6, (), False),
    (3, 3, 3, 256, torch.float32, 200, 10, (), True),                   # Adam coefficients per run
])
def test_step_tail_in_batched_runs(dev, R, n, C, D, dtype, j, K, discard, per_run_adam):
    from moc_amd import main_moc as M
    epochs = 2
    lrs = [1e-3 * (1 + r) if per_run_adam else 1e-3 for r in range(R)]
    alone = [_alone(dev, r, n, C, D, dtype, j, K, epochs, discard, lrs[r]) for r in range(R)]
    models, opts, splits, gens = [], [], [], []
    for r in range(R):
        W, We, bags, labels = _task(r, n, C, D, dtype)
        M.set_classifier_bank(W.to(dev), We.to(dev))
        torch.manual_seed(300 + r)
        model = M.senet(D, 4).to(dev)
        models.append(model)
        opts.append(torch.optim.Adam(model.parameters(), lr=lrs[r], weight_decay=1e-4))
        splits.append(M.ResidentBags(bags, labels, dev))
        g = torch.Generator()
        g.manual_seed(7100 + r)
        gens.append(g)
    args = H.make_args(C, j, K, discard)
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
