"""Sensitivity sweeps on the GPU: moc_topk_mean_multi gives, per K, the bits of moc_topk_mean at that K (pooled, indices,
counts) and agrees with a float64 top-K mean; the pooling mirrors give the same tensors from one launch for a multi-entry
list; evaluation_sweep / zs_evaluation_sweep return, cell by cell, the floats of evaluation() / zs_evaluation(); the
command line writes the same numbers.

Thirty-class splits hold 30 slides, not 12: evaluation()'s multi-class AUC needs every class among the slides (sklearn
refuses otherwise, as in the reference), so a 12-slide split has no evaluation() to compare with."""
import json

import numpy as np
import pandas as pd
import pytest
import torch

import helpers as H
from moc_amd import synth
from oracle import moc_oracle as O

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(scope="module")
def dev(gpu_device):
    return gpu_device


# ------------------------------------------------------------------ 1. the kernel against moc_topk_mean
# empty, len < K, the lane-count edges, one candidate list's worth, the sampled bound (> 4096); then 2,000 equal keys (the
# candidate list overflows: the exact fall-back) and a segment of +-0.0 and negative keys
LENS = [0, 1, 3, 63, 64, 65, 257, 5000, 2000, 70]
SEG_EQUAL, SEG_ZEROS = 8, 9
K_LISTS = [[1], [64], [1, 5, 10, 50, 64], [10, 1, 64, 10]]
BOUNDARIES = (1, 5, 10, 50, 64)


def _columns(C, seed, smallest):
    """[C, sum(LENS)] keys with |key| <= 0.2 (see the float64 bound below); exact ties planted across every K boundary of
    the two long random segments, in the direction that is ranked first."""
    g = torch.Generator().manual_seed(seed)
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    keys = (torch.rand((C, int(off[-1])), generator=g) - 0.5) * 0.4
    for s in (6, 7):
        for c in range(C):
            seg = keys[c, off[s]:off[s + 1]]
            order = torch.argsort(seg, descending=not smallest, stable=True)
            for b in BOUNDARIES:                       # ranks b-1 and b (0-based) hold one value: the lower row must win
                seg[order[b]] = seg[order[b - 1]]
            seg[order[2]] = seg[order[3]] = seg[order[1]]
    keys[:, off[SEG_EQUAL]:off[SEG_EQUAL + 1]] = 0.125
    z = keys[:, off[SEG_ZEROS]:off[SEG_ZEROS + 1]]
    z[:, 0::3] = 0.0
    z[:, 1::3] = -0.0
    z[:, 2::3] = -z[:, 2::3].abs()
    return keys, torch.from_numpy(off)


def _expect64(keys, vals, off, K, smallest):
    """float64 mean of the values of the first min(K, len) rows by key (ties: lower row first) -> [n_seg, C]."""
    C = vals.size(0)
    out = torch.full((len(LENS), C), float("nan"), dtype=torch.float64)
    for s, n in enumerate(LENS):
        if n == 0:
            continue
        for c in range(C):
            kc = keys[c if keys.size(0) > 1 else 0, off[s]:off[s + 1]]
            order = torch.argsort(kc, descending=not smallest, stable=True)[:min(K, n)]
            out[s, c] = vals[c, off[s]:off[s + 1]][order].double().mean()
    return out


@pytest.mark.parametrize("mode", ["same", "distinct", "shared"])
@pytest.mark.parametrize("C", [1, 2, 30])
def test_multi_is_topk_mean_per_k(dev, C, mode):
    from moc_amd import engine as E
    for smallest in (False, True):
        keys, off = _columns(C, 100 + C, smallest)
        if mode == "same":
            vals = keys
        else:
            g = torch.Generator().manual_seed(7 + C)
            vals = (torch.rand(keys.shape, generator=g) - 0.5) * 0.4
            if mode == "shared":
                keys = keys[:1].contiguous()
        kd = keys.to(dev)
        vd = kd if mode == "same" else vals.to(dev)
        seg = off.to(dev)
        shared = mode == "shared"
        single = {K: E.topk_mean(kd, vd, K, smallest=smallest, key_shared=shared, want_idx=True, seg_off=seg)
                  for K in BOUNDARIES}
        nonempty = torch.tensor([n > 0 for n in LENS], device=dev)
        for Ks in K_LISTS:
            pooled, idx, cnt = E.topk_mean_multi(kd, vd, Ks, smallest=smallest, key_shared=shared, want_idx=True, seg_off=seg)
            assert tuple(pooled.shape) == (len(Ks), len(LENS), C) and tuple(idx.shape) == (len(LENS), C, max(Ks))
            assert torch.equal(cnt, single[max(Ks)][2]) and cnt[0].eq(0).all()
            assert torch.equal(idx[nonempty], single[max(Ks)][1][nonempty]) and idx[0].eq(-1).all()
            for i, K in enumerate(Ks):
                p1, i1, c1 = single[K]
                # (bit patterns: an empty segment pools to NaN in both, and NaN != NaN)
                assert torch.equal(pooled[i].view(torch.int32), p1.view(torch.int32)), (C, mode, smallest, Ks, K)
                assert torch.isnan(pooled[i, 0]).all()
                assert torch.equal(idx[nonempty][..., :K], i1[nonempty]) and torch.equal(cnt.clamp(max=K), c1)
                # both kernels could be wrong together: a float64 mean.  |value| <= 0.2, so every partial sum is below 16
                # (ulp 9.5e-7): 64 sequential additions err by at most 64 x 4.8e-7 on the sum, 4.8e-7 on the mean -- inside 1e-6
                want = _expect64(keys, vals, off, K, smallest)
                got = pooled[i].cpu().double()
                assert (got[1:] - want[1:]).abs().max().item() <= 1e-6
        # ties: the lower row wins (the planted pairs are adjacent ranks of one value)
        i64 = single[64][1].cpu()
        for s in (6, 7):
            for c in range(C):
                kc = keys[c if not shared else 0, off[s]:off[s + 1]]
                rows = i64[s, c].long()
                kv = kc[rows]
                same_key = kv[1:] == kv[:-1]
                assert same_key.sum() >= len(BOUNDARIES) - 1 and (rows[1:][same_key] > rows[:-1][same_key]).all()
        # the all-equal segment: rows 0 .. 63 in order (the fall-back ranks over all keys)
        assert torch.equal(i64[SEG_EQUAL, 0], torch.arange(64, dtype=torch.int32))


def test_multi_segment_lengths_given(dev):
    """seg_len given: segments with slack behind them, the slack filled with keys that would win."""
    from moc_amd import engine as E
    C = 3
    keys, off = _columns(C, 55, False)
    pad = 37
    off2 = torch.tensor([int(off[s]) + pad * s for s in range(len(LENS) + 1)], dtype=torch.int64)
    wide = torch.full((C, int(off2[-1])), 9.0)
    for s, n in enumerate(LENS):
        wide[:, off2[s]:off2[s] + n] = keys[:, off[s]:off[s + 1]]
    kd, wd = keys.to(dev), wide.to(dev)
    lens = torch.tensor(LENS, dtype=torch.int32, device=dev)
    Ks = [1, 5, 10, 50, 64]
    a = E.topk_mean_multi(kd, kd, Ks, want_idx=True, seg_off=off.to(dev))
    b = E.topk_mean_multi(wd, wd, Ks, want_idx=True, seg_off=off2.to(dev), seg_len=lens)
    c = E.topk_mean_multi(kd, kd, Ks, want_idx=True, seg_off=off.to(dev), seg_len=lens)
    for x in (b, c):
        assert torch.equal(a[0].view(torch.int32), x[0].view(torch.int32)) and torch.equal(a[1], x[1]) and torch.equal(a[2], x[2])


# ------------------------------------------------------------------ 2. the pooling mirrors
@pytest.mark.parametrize("N, C", [(1000, 2), (300, 30)])
def test_pool_with_a_list_is_the_single_calls(dev, N, C, monkeypatch):
    from moc_amd import engine as E, patch_selection_classifier as P
    g = torch.Generator().manual_seed(N + C)
    ext = torch.randn((N, C + 4), generator=g).to(dev)
    lg = ext[:, :C].contiguous()
    calls = {"multi": 0}
    orig = E.topk_mean_multi

    def counted(*a, **k):
        calls["multi"] += 1
        return orig(*a, **k)
    monkeypatch.setattr(E, "topk_mean_multi", counted)
    funcs = [(P.topj_pooling, lg, {}), (P.delta_softmax_classifier_pooling, lg, {}), (P.delta_diff_classifier_pooling, lg, {}),
             (P.bottomk_irrel_classifier_pooling, ext, {"coords_list": C})]
    js = [1, 5, 10, 50]
    for f, x, kw in funcs:
        calls["multi"] = 0
        preds, pooled = f(x, js, **kw)
        assert calls["multi"] == 1, f.__name__
        p3, pooled3, idx3 = f(x, js, return_indices=True, **kw)
        _, _, idx_ref = f(x, [50], return_indices=True, **kw)
        assert torch.equal(idx3, idx_ref) and tuple(idx3.shape) == (50, C)
        for j in js:
            # bottomk ranks among the `bottomk` rows of least background, by default max(topj): pin it for the single calls
            kw1 = dict(kw, bottomk=50) if f is P.bottomk_irrel_classifier_pooling else kw
            p1, q1 = f(x, [j], **kw1)
            for got in (pooled[j], pooled3[j]):
                assert got.shape == q1[j].shape and torch.equal(got, q1[j]), (f.__name__, j)
            assert torch.equal(preds[j], p1[j]) and torch.equal(p3[j], p1[j])
        # an entry above 64: the loop, as before
        calls["multi"] = 0
        preds, pooled = f(x, [1, 100], **kw)
        assert calls["multi"] == 0
        kw1 = dict(kw, bottomk=100) if f is P.bottomk_irrel_classifier_pooling else kw
        for j in (1, 100):
            assert torch.equal(pooled[j], f(x, [j], **kw1)[1][j])


# ------------------------------------------------------------------ 3. / 4. the sweeps against evaluation / zs_evaluation
TOPJS, TOPKS = (5, 40, 400), (1, 10, 64)
DISCARDS = ((), ("delta_softmax",), ("topk", "bottomk"))
# (C, storage, D, slides)
CASES = [(2, "fp32", 512, 12), (2, "bf16", 512, 12), (2, "fp16", 512, 12), (3, "fp32", 512, 12),
         (30, "bf16", 512, 30), (30, "bf16", 1024, 30)]
IDS = [f"C{c[0]}-{c[1]}-D{c[2]}" for c in CASES]
_splits = {}


def _split(case, dev):
    """The case's bank, slides (300 .. 2,000 rows), model and resident split: built once, never changed."""
    from moc_amd import main_moc as M
    if case not in _splits:
        C, st, D, n = case
        W, We = synth.make_bank(40 + C, D, C)
        sizes = [int(v) for v in np.random.default_rng(C * 1000 + D).integers(300, 2001, size=n)]
        sizes[0], sizes[1] = 300, 2000
        bags, labels = synth.make_slide_set(4000 + C, sizes, D, We, C, confusion=0.3)
        torch.manual_seed(17 + C)
        model = M.senet(D, 4).to(dev)
        with torch.no_grad():                   # gates away from 0 / 1: every term of the mix matters
            model.model[2].weight.mul_(3.0)
        _splits[case] = (W.to(dev), We.to(dev), bags, labels, model, M.ResidentBags(bags, labels, dev, dtype=DT[st]), W, We)
    s = _splits[case]
    M.set_classifier_bank(s[0], s[1])
    return s


def _cells():
    return [(j, k, d) for j in TOPJS for d in DISCARDS for k in TOPKS]


def _reference(case, dev):
    from moc_amd import main_moc as M
    _, _, _, _, model, res, _, _ = _split(case, dev)
    return {(j, k, d): M.evaluation(model, res, dev, H.make_args(case[0], j, k, d)) for j, k, d in _cells()}


def _assert_cells(got, ref):
    assert set(got) == set(ref)
    for key in ref:
        for f in ("loss", "acc", "auc"):
            assert got[key][f] == ref[key][f], (key, f, got[key][f], ref[key][f])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_evaluation_sweep_is_evaluation_cell_by_cell(dev, case, monkeypatch):
    from moc_amd import main_moc as M
    _, _, _, _, model, res, _, _ = _split(case, dev)
    ref = _reference(case, dev)
    args = H.make_args(case[0], 10, 10, ())
    got = M.evaluation_sweep(model, res, dev, args, TOPJS, TOPKS, DISCARDS)
    assert len(got) == 27
    _assert_cells(got, ref)
    # reversed order: the score pass's statistics survive every tail
    rev = M.evaluation_sweep(model, res, dev, args, TOPJS[::-1], TOPKS[::-1], DISCARDS[::-1])
    _assert_cells(rev, ref)
    assert (args.topj, args.topk, args.discard_classifiers) == (10, 10, []) and res.repeat_num == res.real_len()
    # discard_sets=None: the one of args
    one = M.evaluation_sweep(model, res, dev, H.make_args(case[0], 10, 10, ("delta_softmax",)), (40,), (10,))
    assert list(one) == [(40, 10, ("delta_softmax",))] and one[(40, 10, ("delta_softmax",))] == ref[(40, 10, ("delta_softmax",))]
    # evaluation() itself is as it was after a sweep used its cached batch
    assert M.evaluation(model, res, dev, H.make_args(case[0], 10, 10, ())) == \
        M.evaluation_sweep(model, res, dev, args, (10,), (10,))[(10, 10, ())]
    # at least three chunks
    row_bytes = case[2] * res.X.element_size()
    monkeypatch.setattr(M, "MAX_BATCH_BYTES", (sum(res.sizes) * row_bytes) // 4)
    assert len(M._chunks(res.sizes, case[2], res.X.element_size())) >= 3
    _assert_cells(M.evaluation_sweep(model, res, dev, args, TOPJS, TOPKS, DISCARDS), _reference(case, dev))


def test_evaluation_sweep_against_the_oracle(dev):
    from moc_amd import main_moc as M
    case = CASES[0]
    _, _, bags, labels, model, res, W, We = _split(case, dev)
    j, k, d = 40, 64, ("delta_softmax",)
    got = M.evaluation_sweep(model, res, dev, H.make_args(2, 10, 10, ()), (5, j), (1, k), [(), d])[(j, k, d)]
    ref_model = O.Senet(case[2], 4)
    ref_model.load_state_dict({n: v.detach().cpu() for n, v in model.state_dict().items()})
    want = O.evaluation(ref_model, bags, labels, W, We, 2, j, k, discard=d)
    assert abs(got["loss"] - want["loss"]) <= 1e-4 and got["acc"] == want["acc"] and abs(got["auc"] - want["auc"]) <= 0.002


def test_sweeps_refuse(dev):
    from moc_amd import main_moc as M, patch_selection_classifier as P
    _, _, bags, labels, model, res, _, _ = _split(CASES[0], dev)
    args = H.make_args(2, 10, 10, ())
    with pytest.raises(AssertionError, match="64"):
        M.evaluation_sweep(model, res, dev, args, (10,), (65,))
    with pytest.raises(AssertionError, match="64"):
        M.zs_evaluation_sweep(res, dev, args, (1, 65))
    with pytest.raises(AssertionError, match="resident"):
        M.evaluation_sweep(model, H.ListLoader(bags, labels), dev, args, (10,), (10,))
    seeded = M.ResidentBags(bags[:2], labels[:2], dev, loader_seed_draw=True)
    with pytest.raises(AssertionError, match="loader_seed_draw"):
        M.evaluation_sweep(model, seeded, dev, args, (10,), (10,))
    with pytest.raises(AssertionError, match="four fused"):
        M.zs_evaluation_sweep(res, dev, args, (1,), pooling_funcs=(lambda *a, **k: None,))
    assert M.ZS_POOLING_FUNCS == (P.topj_pooling, P.delta_softmax_classifier_pooling, P.delta_diff_classifier_pooling,
                                  P.bottomk_irrel_classifier_pooling)


@pytest.mark.parametrize("case", [CASES[0], CASES[4]], ids=[IDS[0], IDS[4]])
def test_zs_sweep_is_zs_evaluation_cell_by_cell(dev, case, monkeypatch):
    from moc_amd import main_moc as M
    _, _, _, _, _, res, _, _ = _split(case, dev)
    got = M.zs_evaluation_sweep(res, dev, H.make_args(case[0], 10, 10, ()), TOPKS)
    assert len(got) == 12
    for f in M.ZS_POOLING_FUNCS:
        for k in TOPKS:
            want = M.zs_evaluation(res, dev, H.make_args(case[0], 10, k, ()), pooling_func=f)
            assert got[(f.__name__, k)] == want, (f.__name__, k, got[(f.__name__, k)], want)
    sub = M.zs_evaluation_sweep(res, dev, H.make_args(case[0], 10, 10, ()), (64, 1), pooling_funcs=M.ZS_POOLING_FUNCS[2:])
    assert list(sub) == [("delta_diff_classifier_pooling", 64), ("delta_diff_classifier_pooling", 1),
                         ("bottomk_irrel_classifier_pooling", 64), ("bottomk_irrel_classifier_pooling", 1)]
    assert all(sub[key] == got[key] for key in sub)
    # a bank whose extended foreground columns are NOT zeroshot_weights: bottomk ranks the extended ones (a pass of its own)
    s = _split(case, dev)
    We2 = s[1].clone()
    We2[:, 0] = -We2[:, 0]
    monkeypatch.setattr(M, "zeroshot_weights_ext", We2)
    got2 = M.zs_evaluation_sweep(res, dev, H.make_args(case[0], 10, 10, ()), (10,))
    for f in M.ZS_POOLING_FUNCS:
        assert got2[(f.__name__, 10)] == M.zs_evaluation(res, dev, H.make_args(case[0], 10, 10, ()), pooling_func=f), f.__name__


# ------------------------------------------------------------------ 5. the command line
def test_cli_writes_the_in_process_numbers(dev, tmp_path):
    from moc_amd import main_moc as M, run_moc, sweep as S
    torch.manual_seed(5)
    model = M.senet(512, 4)
    with torch.no_grad():
        model.model[2].weight.mul_(3.0)
    ckpt = tmp_path / "m.pt"
    torch.save(model.state_dict(), ckpt)
    out = tmp_path / "sens"
    ev, zs = S.cli(["--ckpt", str(ckpt), "--topjs", "5,40", "--topks", "1,10,64", "--discard_sets", "none", "topk+bottomk", "--zs",
                    "--synthetic", "12", "--shot", "2", "--split", "test", "--out", str(out), "--disable_tqdm"])
    assert len(ev) == 12 and len(zs) == 12
    doc = json.load(open(out / "sensitivity.json"))
    df = pd.read_csv(out / "sensitivity.csv", float_precision="round_trip")
    assert len(df) == 24 and (df["kind"] == "eval").sum() == 12
    assert doc["args"]["topjs"] == [5, 40] and doc["args"]["discard_sets"] == ["none", "topk+bottomk"]
    # the in-process calls on the same split
    ra = run_moc.get_args([])
    ra.synthetic, ra.shot, ra.disable_tqdm = 12, 2, True
    loader = run_moc.prepare(ra, dev)[2]
    model = model.to(dev)
    for j in (5, 40):
        for k in (1, 10, 64):
            for d in ((), ("topk", "bottomk")):
                want = M.evaluation(model, loader, dev, H.make_args(ra.n_classes, j, k, d))
                assert doc["evaluation"][f"topj={j},topk={k},discard={S.discard_name(d)}"] == want == ev[(j, k, d)]
                row = df[(df["kind"] == "eval") & (df["topj"] == j) & (df["topk"] == k) & (df["discard"] == S.discard_name(d))]
                assert len(row) == 1 and row["auc"].item() == want["auc"] and row["loss"].item() == want["loss"]
    for f in M.ZS_POOLING_FUNCS:
        for k in (1, 10, 64):
            want = M.zs_evaluation(loader, dev, H.make_args(ra.n_classes, 10, k, ()), pooling_func=f)
            assert doc["zero_shot"][f"{f.__name__},topk={k}"] == want
    # --zs alone: no checkpoint
    ev2, zs2 = S.cli(["--zs", "--topks", "10", "--synthetic", "12", "--shot", "2", "--split", "test", "--out", str(tmp_path / "z"),
                      "--disable_tqdm"])
    assert ev2 is None and zs2[("topj_pooling", 10)] == zs[("topj_pooling", 10)]
    assert "evaluation" not in json.load(open(tmp_path / "z" / "sensitivity.json"))
