"""Bank sweeps on the GPU: moc_scores_banks writes, for every bank of a set, bit for bit the statistics and flags that
moc_scores writes over a batch with that bank alone (and agrees with a float64 product); zs_evaluation_banks,
zs_evaluation_sweep_banks and evaluation_banks return, bank by bank, the Python floats of zs_evaluation /
zs_evaluation_sweep / evaluation under that bank; `sweep --banks` writes the numbers of one `sweep` run per bank."""
import json

import numpy as np
import pandas as pd
import pytest
import torch

import helpers as H
from moc_amd import engine, synth
from moc_amd import main_moc as M
from moc_amd.engine import Bank, BankSet, SlideBatch

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
TIGHT = 2e-6      # the parity suite's bound: fp32 re-association noise on O(1) cosine logits


@pytest.fixture(scope="module")
def dev(gpu_device):
    return gpu_device


# ------------------------------------------------------------------ 1. the kernel against moc_scores, bit for bit
# one row, the tile size and its neighbours, two tiles + 1, several tiles, more rows than one workgroup's first sweep
SIZES = [1, 15, 16, 17, 33, 300, 1000]


def _unit_columns(D, n, g):
    w = torch.randn((D, n), generator=g)
    return (w / w.norm(dim=0, keepdim=True)).contiguous()       # |w| <= 1 < 2: fp16 storage takes them


def _banks(D, C, n, seed):
    """n banks of C classes whose widths differ inside one set: Ce = C+1, C+4, 16, C+4; W is not W_ext[:, :C]."""
    g = torch.Generator().manual_seed(seed)
    ces = [C + 1, C + 4, 16, C + 4][:n]
    return [(_unit_columns(D, C, g), _unit_columns(D, ce, g)) for ce in ces]


def _ways(total, seed):
    """(name, sizes, x_starts, mask): unmasked; a drawn mask (kept lists, short first and last tiles); one slide twice."""
    starts = [0]
    for n in SIZES:
        starts.append(starts[-1] + n)
    g = torch.Generator().manual_seed(seed)
    mask = (torch.rand(total, generator=g) > 0.5).to(torch.uint8)
    mask[0] = 1                                              # (the one-row slide keeps its row)
    twice = SIZES + [SIZES[4]]
    return [("unmasked", SIZES, None, None), ("masked", SIZES, None, mask),
            ("twice", twice, starts[:-1] + [starts[4]], None)]


def _expect64(X, sizes, x_starts, mask, W, We, C):
    """float64 statistics [2C+3, slots] of the kept rows in slot order + the number of kept rows per slide."""
    xs = x_starts
    if xs is None:
        xs, o = [], 0
        for n in sizes:
            xs.append(o)
            o += n
    Wcat = torch.cat([W, We[:, C:]], 1).double()
    cols, o = [], 0
    for st, n in zip(xs, sizes):
        rows = X[st:st + n].double()
        if mask is not None:
            rows = rows[mask[o:o + n].bool()]
        lg = rows @ Wcat
        fg, bgc = lg[:, :C], lg[:, C:]
        top2 = fg.topk(2, dim=1)[0]
        cols.append((o, torch.cat([fg, torch.softmax(fg, 1), (top2[:, 0] - top2[:, 1]).abs()[:, None],
                                   bgc.sum(1, keepdim=True), bgc.max(1, keepdim=True)[0]], 1).t()))
        o += n
    return cols


@pytest.mark.parametrize("C", [2, 3])
@pytest.mark.parametrize("D", [256, 512, 1024])
@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
def test_scores_banks_bits_of_moc_scores(dev, dt, D, C):
    dtype = DT[dt]
    gmax = engine.lib().moc_scores_banks_max(D, engine._dtype_code(dtype))
    assert gmax == {256: (4, 3), 512: (4, 3), 1024: (2, 1)}[D][0 if dt == "fp32" else 1]
    g = torch.Generator().manual_seed(100 * D + C)
    total = sum(SIZES)
    Xh = torch.randn((total, D), generator=g)
    Xh = (Xh / Xh.norm(dim=1, keepdim=True)).to(dtype)
    X = Xh.to(dev)
    banks = _banks(D, C, gmax, seed=7 * D + C)
    for name, sizes, x_starts, mask in _ways(total, seed=D + C):
        # moc_scores per bank, once: arrays pre-filled with the bank's own sentinel
        refs = []
        for b, (W, We) in enumerate(banks):
            ref = SlideBatch(X, sizes, C, We.size(1), 1, 1, mask=mask, x_starts=x_starts)
            ref.stats.fill_(-1000.0 - b)
            ref.sel_flag.fill_(0x40 + b)
            ref.scores(Bank(W, We, dtype, dev))
            refs.append((ref.stats.clone(), ref.sel_flag.clone()))
            # ... and the float64 product on the kept rows
            for o, exp in _expect64(Xh, sizes, x_starts, mask, W, We, C):
                got = ref.stats[:, o:o + exp.size(1)].double().cpu()
                tol = torch.tensor([TIGHT] * (2 * C) + [2 * TIGHT, 4 * TIGHT, TIGHT], dtype=torch.float64)[:, None]
                err = (got - exp).abs()
                assert bool((err <= tol).all()), (name, b, float(err.max()))
        for G in range(1, gmax + 1):
            parent = SlideBatch(X, sizes, C, banks[0][1].size(1), 1, 1, mask=mask, x_starts=x_starts)
            bs = BankSet(banks[:G], dtype, dev)
            assert bs.passes == [(0, G)]
            views = parent.scores_banks(bs)                    # (builds the views)
            for b, v in enumerate(views):
                v.stats.fill_(-1000.0 - b)
                v.sel_flag.fill_(0x40 + b)
            again = parent.scores_banks(bs)
            assert all(a is v for a, v in zip(again, views))
            for b, v in enumerate(views):
                assert (v.C, v.Ce) == (C, banks[b][1].size(1))
                assert torch.equal(v.stats, refs[b][0]), (name, G, b, "stats")
                assert torch.equal(v.sel_flag, refs[b][1]), (name, G, b, "sel_flag")


# ------------------------------------------------------------------ 3. the Python floats of the per-bank calls
CASES = [(2, "fp32"), (3, "fp32"), (2, "bf16"), (3, "bf16")]
IDS = [f"C{c}-{s}" for c, s in CASES]
D_SPLIT = 512
TOPKS = (1, 10, 64)
_splits = {}


def _split(case, dev):
    """The case's five banks (widths C+4, C+1, 16, C+2, C+4; bank 3's W_ext[:, :C] is not its W), 12 slides of 200 .. 500
    rows planted from bank 0, five models and the resident split: built once, never changed."""
    if case not in _splits:
        C, st = case
        W0, We0 = synth.make_bank(60 + C, D_SPLIT, C)
        g = torch.Generator().manual_seed(600 + C)
        banks = [(W0, We0)]
        for b, ce in enumerate([C + 1, 16, C + 2, C + 4], start=1):
            fg = We0[:, :C] + 0.05 * b * _unit_columns(D_SPLIT, C, g)
            fg = fg / fg.norm(dim=0, keepdim=True)
            bg = _unit_columns(D_SPLIT, ce - C, g)
            n_old = min(4, ce - C)
            bg[:, :n_old] = We0[:, C:C + n_old]
            We = torch.cat([fg, bg], 1).contiguous()
            W = fg.clone().contiguous()
            if b == 3:                                   # bottomk ranks the extended foreground columns: another image
                e = fg + 0.1 * _unit_columns(D_SPLIT, C, g)
                We[:, :C] = e / e.norm(dim=0, keepdim=True)
            banks.append((W, We))
        sizes = [int(v) for v in np.random.default_rng(C * 77).integers(200, 501, size=12)]
        bags, labels = synth.make_slide_set(7000 + C, sizes, D_SPLIT, We0, C, confusion=0.3)
        models = []
        for m in range(5):
            torch.manual_seed(23 + C + m)
            model = M.senet(D_SPLIT, 4).to(dev)
            with torch.no_grad():                        # gates away from 0 / 1: every term of the mix matters
                model.model[2].weight.mul_(3.0)
            models.append(model)
        _splits[case] = ([(W.to(dev), We.to(dev)) for W, We in banks], bags, labels, models,
                         M.ResidentBags(bags, labels, dev, dtype=DT[st]))
    return _splits[case]


def _globals_kept(fn):
    """Runs fn() with the module's bank globals set to two marker tensors: they are the same objects afterwards."""
    w, we = torch.zeros(2, 2), torch.zeros(2, 3)
    M.zeroshot_weights, M.zeroshot_weights_ext = w, we
    out = fn()
    assert M.zeroshot_weights is w and M.zeroshot_weights_ext is we
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_zs_evaluation_banks_is_zs_evaluation_per_bank(dev, case):
    banks, _, _, _, res = _split(case, dev)
    C = case[0]
    assert engine.plan_bank_passes(D_SPLIT, DT[case[1]], 5) == ([(0, 4), (4, 1)] if case[1] == "fp32" else [(0, 3), (3, 2)])
    assert not M._ext_is_fg(*banks[3]) and M._ext_is_fg(*banks[1])
    for f in M.ZS_POOLING_FUNCS:
        args = H.make_args(C, 10, 10, ())
        got = _globals_kept(lambda: M.zs_evaluation_banks(res, dev, args, banks, pooling_func=f))
        assert len(got) == 5
        for g, (W, We) in enumerate(banks):
            M.set_classifier_bank(W, We)
            want = M.zs_evaluation(res, dev, H.make_args(C, 10, 10, ()), pooling_func=f)
            assert got[g] == want, (f.__name__, g, got[g], want)
    assert res.repeat_num == res.real_len() or res.repeat_num is None


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_zs_sweep_banks_is_zs_sweep_per_bank(dev, case):
    banks, _, _, _, res = _split(case, dev)
    C = case[0]
    got = _globals_kept(lambda: M.zs_evaluation_sweep_banks(res, dev, H.make_args(C, 10, 10, ()), banks, TOPKS))
    assert len(got) == 5
    for g, (W, We) in enumerate(banks):
        M.set_classifier_bank(W, We)
        want = M.zs_evaluation_sweep(res, dev, H.make_args(C, 10, 10, ()), TOPKS)
        assert list(got[g]) == list(want)
        assert got[g] == want, (g, got[g], want)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_evaluation_banks_is_evaluation_per_bank(dev, case, monkeypatch):
    banks, _, _, models, res = _split(case, dev)
    C = case[0]

    def reference(ms, discard):
        out = []
        for g, (W, We) in enumerate(banks):
            M.set_classifier_bank(W, We)
            out.append(M.evaluation(ms[g], res, dev, H.make_args(C, 40, 10, discard)))
        return out

    for ms, discard in ((models[:1], ()), (models, ()), (models, ("delta_softmax",))):
        want = reference(ms * 5 if len(ms) == 1 else ms, discard)
        got = _globals_kept(lambda: M.evaluation_banks(ms[0] if len(ms) == 1 else ms, res, dev, H.make_args(C, 40, 10, discard), banks))
        assert got == want, (len(ms), discard, got, want)
    # the (topj, topk, discard) table per bank, and at least three chunks
    want = []
    for g, (W, We) in enumerate(banks):
        M.set_classifier_bank(W, We)
        want.append(M.evaluation_sweep(models[g], res, dev, H.make_args(C, 10, 10, ()), (5, 40), TOPKS, [(), ("topk", "bottomk")]))
    got = M.evaluation_sweep_banks(models, res, dev, H.make_args(C, 10, 10, ()), banks, (5, 40), TOPKS, [(), ("topk", "bottomk")])
    assert got == want
    monkeypatch.setattr(M, "MAX_BATCH_BYTES", (sum(res.sizes) * D_SPLIT * res.X.element_size()) // 4)
    assert len(M._chunks_banks(res.sizes, D_SPLIT, res.X.element_size(), 5, C)) >= 3
    assert M.evaluation_sweep_banks(models, res, dev, H.make_args(C, 10, 10, ()), banks, (5, 40), TOPKS, [(), ("topk", "bottomk")]) == want
    assert M.zs_evaluation_banks(res, dev, H.make_args(C, 10, 10, ()), banks) == \
        [M.zs_evaluation_sweep_banks(res, dev, H.make_args(C, 10, 10, ()), banks, (10,), M.ZS_POOLING_FUNCS[:1])[g][("topj_pooling", 10)]
         for g in range(5)]


def test_bank_forms_refuse(dev):
    banks, bags, labels, models, res = _split(CASES[0], dev)
    args = H.make_args(2, 10, 10, ())
    other_c = synth.make_bank(3, D_SPLIT, 3)
    wide = synth.make_bank(4, D_SPLIT, 2, n_bg=15)
    for call in (lambda b, ld=res: M.zs_evaluation_banks(ld, dev, args, b),
                 lambda b, ld=res: M.zs_evaluation_sweep_banks(ld, dev, args, b, (10,)),
                 lambda b, ld=res: M.evaluation_banks(models[0], ld, dev, args, b)):
        with pytest.raises(AssertionError, match="different C"):
            call(banks[:1] + [tuple(t.to(dev) for t in other_c)])
        with pytest.raises(AssertionError, match="at most 16.*zs_evaluation"):
            call(banks[:1] + [tuple(t.to(dev) for t in wide)])
        with pytest.raises(AssertionError, match="resident"):
            call(banks, H.ListLoader(bags, labels))
        with pytest.raises(AssertionError, match="loader_seed_draw"):
            call(banks, M.ResidentBags(bags[:2], labels[:2], dev, loader_seed_draw=True))
    with pytest.raises(AssertionError, match="64"):
        M.zs_evaluation_sweep_banks(res, dev, args, banks, (1, 65))
    with pytest.raises(AssertionError, match="one per bank"):
        M.evaluation_banks(models[:2], res, dev, args, banks)


# ------------------------------------------------------------------ 4. the command line
def test_cli_banks_writes_the_numbers_of_one_sweep_per_bank(dev, tmp_path, monkeypatch):
    from moc_amd import run_moc, sweep as S
    C = 2
    names = ["plain", "short", "full"]
    bank_args, banks = [], []
    for b, (name, n_bg) in enumerate(zip(names, (4, 1, 14))):
        W, We = synth.make_bank(1234 + 10 * b, 512, C, n_bg=n_bg)
        torch.save(W, tmp_path / f"{name}_W.pt")
        torch.save(We, tmp_path / f"{name}_We.pt")
        bank_args.append(f"{name}={tmp_path / (name + '_W.pt')},{tmp_path / (name + '_We.pt')}")
        banks.append((W, We))
    ckpts = []
    for m in range(3):
        torch.manual_seed(5 + m)
        model = M.senet(512, 4)
        with torch.no_grad():
            model.model[2].weight.mul_(3.0)
        torch.save(model.state_dict(), tmp_path / f"m{m}.pt")
        ckpts.append(str(tmp_path / f"m{m}.pt"))
    common = ["--topjs", "5,40", "--topks", "1,10", "--discard_sets", "none", "topk+bottomk", "--zs",
              "--synthetic", "12", "--shot", "2", "--split", "test", "--disable_tqdm"]
    out = tmp_path / "banks"
    ev, zs = S.cli(["--ckpt"] + ckpts + ["--banks"] + bank_args + ["--out", str(out)] + common)
    assert list(ev) == names and list(zs) == names
    summary = pd.read_csv(out / "bank_summary.csv", float_precision="round_trip")
    assert list(summary.columns) == ["bank", "kind", "topj", "topk", "discard", "loss", "acc", "auc"] and len(summary) == 3 * 16
    # one plain sweep per bank: the bank is what run_moc.prepare sets for a generated split
    real_set = M.set_classifier_bank
    for g, name in enumerate(names):
        monkeypatch.setattr(M, "set_classifier_bank", lambda W, We, g=g: real_set(banks[g][0].to(dev), banks[g][1].to(dev)))
        S.cli(["--ckpt", ckpts[g], "--out", str(tmp_path / f"one_{name}")] + common)
        monkeypatch.setattr(M, "set_classifier_bank", real_set)
        a = json.load(open(out / name / "sensitivity.json"))
        b = json.load(open(tmp_path / f"one_{name}" / "sensitivity.json"))
        assert a["evaluation"] == b["evaluation"] and len(a["evaluation"]) == 8
        assert a["zero_shot"] == b["zero_shot"] and len(a["zero_shot"]) == 8
        da = pd.read_csv(out / name / "sensitivity.csv", float_precision="round_trip")
        db = pd.read_csv(tmp_path / f"one_{name}" / "sensitivity.csv", float_precision="round_trip")
        pd.testing.assert_frame_equal(da, db, check_exact=True)
        rows = summary[summary["bank"] == name].drop(columns="bank").reset_index(drop=True)
        pd.testing.assert_frame_equal(rows, da, check_exact=True)
    # one checkpoint for all banks
    ev1, _ = S.cli(["--ckpt", ckpts[0], "--banks"] + bank_args + ["--out", str(tmp_path / "one_ckpt")] + common)
    assert ev1["plain"] == ev["plain"] and ev1["short"] != ev["short"]
