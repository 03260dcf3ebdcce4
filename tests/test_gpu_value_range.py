"""The kernels OFF the unit sphere.  Every other numerical test runs on moc_amd/synth.py data -- unit-norm rows, unit-norm
bank columns, cosine logits in [-1, 1] -- while the reference multiplies whatever its feature files hold
(main_moc.py:336).  Needs an MI355X: run with -m gpu.  The inputs, float64 references and rules are in
helpers_value_range.py; test_value_range_cpu.py checks them without a GPU.

Exact checks (bits, no tolerance): a row times 2^s is exact in its storage type, so products and fp32 accumulations scale
exactly and every statistic of degree one -- logits, gap, background sum and maximum, the hidden layer with b1 = 0 --
scales exactly, whatever the summation order; a repeated row gives repeated statistics wherever it sits in its tile; zero
rows give +0 logits.  Bounded checks carry the unit-sphere tolerance (TIGHT and its multiples) to the row's scale by that
exactness, or add the reference's own fp32 noise, measured inside the test (helpers_value_range.measured_allowed).

Reference noise of the gradient task, max|g32 - g64| / max|g64| per scale (fp32 rows; slides 0, 1), measured on the CPU:
2^-6: 1.4e-5, 1.7e-6;  1/8: 4.6e-7, 1.3e-6;  5: 2.2e-7, 4.9e-7;  32: 1.5e-6, 6.7e-7;  200: 6.2e-2, 6.1e-2 (the reference's
own cancellation in 1 - p at a loss of 1e-7: the rule is loose there by construction)."""
import ctypes

import numpy as np
import pytest
import torch

import helpers as H
import helpers_value_range as V
from moc_amd import synth

pytestmark = pytest.mark.gpu

TIGHT = V.TIGHT
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NAME = {F32: "fp32", BF16: "bf16", F16: "fp16"}
SIZES = [1, 15, 17, 33, 300]                 # short first tiles: bases 1, 16, 33, 66
# (storage, ring kernel, C, D): the register streaming kernel in every storage, the ring kernel (fp32, one n-tile), and
# a thirty-class bank -- three n-tiles
FORMS = [(F32, False, 2, 256), (F32, False, 3, 512), (F32, True, 2, 512), (F32, True, 3, 256), (BF16, False, 2, 512),
         (BF16, False, 3, 256), (F16, False, 2, 256), (F16, False, 3, 512), (BF16, False, 30, 512)]
FORM_IDS = [f"{NAME[d]}-{'ring' if r else 'reg'}-C{c}-D{D}" for d, r, c, D in FORMS]


@pytest.fixture(scope="module")
def dev(gpu_device):
    return gpu_device


def _engine():
    from moc_amd import engine
    return engine


def _pow2_scales(dtype):
    return V.POW2_F16 if dtype == F16 else V.POW2_WIDE


def _bits(t):
    return t.contiguous().view(torch.int32)


def _valid(sizes, mask):
    return torch.cat([torch.arange(off, off + nk) for off, nk, _ in V.slot_ranges(sizes, mask)])


def _kept_rows(sizes, mask):
    """Row of the packed array behind every valid slot, in slot order."""
    return torch.cat([off + kept for off, _, kept in V.slot_ranges(sizes, mask)])


def _scores(dev, xs, sizes, Cn, bank, mask=None, ring=False):
    """SlideBatch.scores over the host rows xs (already in their storage type) -> the [2C+3, T] statistics on the host."""
    E = _engine()
    L = E._lib
    b = E.SlideBatch(xs.to(dev).contiguous(), sizes, Cn, Cn + 4, 10, 10, (), mask=mask)
    if ring:
        assert b.use_score_ring(), "the plan gives this shape the ring kernel"
    else:
        assert E.lib().moc_scores_form(ctypes.byref(b.c)) != L.SCORE_FORM_RING
    b.stats.fill_(float("nan"))
    b.scores(bank)
    torch.cuda.synchronize()
    assert bool(b.c.flags & L.MOC_SCORES_RING) == ring
    if mask is not None:
        assert b.n_kept.cpu().tolist() == [nk for _, nk, _ in V.slot_ranges(sizes, mask)]
    return b.stats.cpu()


def _bank(dev, W, We, dtype):
    return _engine().Bank.get(W, We, dtype, dev)


def _rows(seed, sizes, D, We, Cn, dtype):
    bags, _ = synth.make_slide_set(seed, sizes, D, We, Cn)
    return torch.cat(bags).to(dtype)


def _check_softmax(st, Cn, what):
    """Degree zero: against a float64 softmax of the kernel's OWN fp32 logits, at TIGHT absolute.  The value lies in
    [0, 1] at any scale and the exp2 argument's error contributes at most t e^-t 2^-23: the unit-sphere bound as it is."""
    err = float((st[Cn:2 * Cn].to(torch.float64) - V.softmax64(st[:Cn])).abs().max())
    assert err <= TIGHT, f"{what}: softmax off by {err:.3e}"


def _check_against_float64(st, xs_valid, W, We, Cn, what, mult=1.0):
    """Logits, gap, background sum and maximum per row against float64 of the rounded rows, at the existing multiples of
    TIGHT times the power of two at or above the row's norm (the unit-sphere bound carried over by the exact 2^s
    scaling; `mult`: a further exact power of two, for a scaled bank); the softmax as above."""
    ref = V.stats64(xs_valid, W, We, Cn)
    norm = xs_valid.to(torch.float64).norm(dim=1).numpy()
    assert float(norm.min()) > 0
    unit = torch.from_numpy(V.next_pow2(norm)) * TIGHT * mult
    err = (st.to(torch.float64) - ref).abs()
    worst = {}
    for name, rows in (("logits", list(range(Cn))), ("gap", [2 * Cn]), ("bg_sum", [2 * Cn + 1]), ("bg_max", [2 * Cn + 2])):
        ratio = float((err[rows] / (unit * V.TIGHT_MULT[name]).unsqueeze(0)).max())
        worst[name] = ratio
    print(f"{what}: error / allowed {', '.join(f'{k} {v:.3f}' for k, v in worst.items())}")
    for name, ratio in worst.items():
        assert ratio <= 1.0, f"{what}: {name} at {ratio:.2f} of its bound"
    _check_softmax(st, Cn, what)


# ------------------------------------------------------------------ 1. score pass: homogeneity under 2^s
@pytest.mark.parametrize("dtype,ring,Cn,D", FORMS, ids=FORM_IDS)
def test_scores_scale_exactly_with_power_of_two_rows(dev, dtype, ring, Cn, D):
    """stats(2^s X) == 2^s stats(X), as bits, for logits, gap, background sum and maximum; masked and unmasked; slides
    with short first tiles.  fp32 / bf16: s in {-20, -7, -1, 1, 6, 20}; fp16: s in {1, 4, 8} (2^s applied to the rounded
    fp16 values: upscaling is exact, subnormals included; downscaling is not)."""
    W, We = synth.make_bank(900 + Cn, D, Cn)
    xs = _rows(910 + D + Cn, SIZES, D, We, Cn, dtype)
    bank = _bank(dev, W, We, dtype)
    rows = V.degree_one_rows(Cn)
    for mask in (None, V.half_mask(sum(SIZES), 11)):
        valid = _valid(SIZES, mask)
        base = _scores(dev, xs, SIZES, Cn, bank, mask, ring)[:, valid]
        assert torch.isfinite(base).all()
        _check_softmax(base, Cn, "scale 1")
        for s in _pow2_scales(dtype):
            got = _scores(dev, V.scaled_pow2(xs, s), SIZES, Cn, bank, mask, ring)[:, valid]
            exp = base[rows] * float(2.0 ** s)
            assert torch.isfinite(exp).all() and torch.equal(exp.to(torch.float64), base[rows].to(torch.float64) * 2.0 ** s)
            bad = _bits(got[rows]) != _bits(exp)
            assert not bad.any(), (f"2^{s}{' masked' if mask is not None else ''}: {int(bad.sum())} statistics do not scale exactly; "
                                   f"first at (row, slot) {torch.nonzero(bad)[0].tolist()}")
            _check_softmax(got, Cn, f"2^{s}")


@pytest.mark.parametrize("dtype,ring,Cn,D", [(F32, False, 2, 512), (F32, True, 3, 256), (BF16, False, 3, 512), (BF16, False, 30, 256)],
                         ids=["fp32-reg", "fp32-ring", "bf16", "bf16-C30"])
def test_scores_scale_exactly_with_a_power_of_two_bank(dev, dtype, ring, Cn, D):
    """W and W_ext times 2^s, s in {-6, -1}: fp32 images hold the weights themselves and the bf16 image their
    round-to-nearest three-term split, which is scale-invariant -- the same exactness."""
    W, We = synth.make_bank(920 + Cn, D, Cn)
    xs = _rows(930 + D, SIZES, D, We, Cn, dtype)
    rows = V.degree_one_rows(Cn)
    base = _scores(dev, xs, SIZES, Cn, _bank(dev, W, We, dtype), None, ring)
    for s in V.POW2_BANK:
        Ws, Wes = W * float(2.0 ** s), We * float(2.0 ** s)
        got = _scores(dev, xs, SIZES, Cn, _bank(dev, Ws, Wes, dtype), None, ring)
        assert torch.equal(_bits(got[rows]), _bits(base[rows] * float(2.0 ** s))), f"bank x 2^{s}"
        _check_softmax(got, Cn, f"bank x 2^{s}")


@pytest.mark.parametrize("Cn,D", [(2, 256), (3, 512)])
def test_fp16_scores_with_a_power_of_two_bank_against_float64(dev, Cn, D):
    """The fp16 image holds the three fp16 terms of w 2^14: scaling the bank down sends the low term into fp16's
    subnormals, so the scaling is not exact there -- the logits against float64 at TIGHT 2^s instead."""
    W, We = synth.make_bank(940 + Cn, D, Cn)
    xs = _rows(950 + D, SIZES, D, We, Cn, F16)
    for s in V.POW2_BANK:
        Ws, Wes = W * float(2.0 ** s), We * float(2.0 ** s)
        got = _scores(dev, xs, SIZES, Cn, _bank(dev, Ws, Wes, F16))
        err = float((got[:Cn].to(torch.float64) - V.stats64(xs, Ws, Wes, Cn)[:Cn]).abs().max())
        print(f"fp16 bank x 2^{s}: logits off by {err:.3e}, allowed {TIGHT * 2.0 ** s:.3e}")
        assert err <= TIGHT * 2.0 ** s


@pytest.mark.parametrize("dtype,ring,Cn,D", [(F32, False, 2, 256), (F32, True, 3, 512), (BF16, False, 3, 256), (BF16, False, 2, 512),
                                             (F16, False, 2, 512), (F16, False, 3, 256)],
                         ids=["fp32-reg", "fp32-ring", "bf16-C3", "bf16-C2", "fp16-C2", "fp16-C3"])
def test_scores_at_scales_that_are_no_power_of_two(dev, dtype, ring, Cn, D):
    """Rows times 0.3, 5, 23, and times a different factor per row between 0.01 and 30 within one slide.  The rounded
    scaled rows are just another input: per row against float64 of that input."""
    W, We = synth.make_bank(960 + Cn, D, Cn)
    x = _rows(970 + D, SIZES, D, We, Cn, F32)
    bank = _bank(dev, W, We, dtype)
    inputs = [(f"x {f:g}", (x * np.float32(f)).to(dtype)) for f in V.ODD_SCALES]
    inputs.append(("x a factor per row", (x * V.row_factors(x.size(0), 12)).to(dtype)))
    for what, xs in inputs:
        assert torch.isfinite(xs.to(F32)).all()
        for mask in (None, V.half_mask(sum(SIZES), 13)):
            got = _scores(dev, xs, SIZES, Cn, bank, mask, ring)[:, _valid(SIZES, mask)]
            _check_against_float64(got, xs[_kept_rows(SIZES, mask)], W, We, Cn, f"{NAME[dtype]} {what}{' masked' if mask is not None else ''}")


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("Cn,D", [(2, 512), (3, 256)])
def test_scores_with_unequal_bank_column_norms(dev, dtype, Cn, D):
    """Column norms from 0.25 to 1.5 (every |w| < 2, so the fp16 image takes the bank), on the same per-row rule."""
    W, We = V.unequal_bank(980 + Cn, D, Cn)
    xs = _rows(990 + D, SIZES, D, We, Cn, dtype)
    got = _scores(dev, xs, SIZES, Cn, _bank(dev, W, We, dtype))
    _check_against_float64(got, xs, W, We, Cn, f"{NAME[dtype]} unequal columns")


# ------------------------------------------------------------------ 2. repeated rows, zero rows, ties
REP_SIZES = [33, 50, 17]                     # 100 rows; bases 33 and 83 are off multiples of 16
ZERO_SIZES = [21, V.ZERO_HEAD + 100 + V.ZERO_TAIL]
TIE_FORMS = [(F32, False), (F32, True), (BF16, False), (F16, False)]
TIE_IDS = ["fp32-reg", "fp32-ring", "bf16", "fp16"]


@pytest.mark.parametrize("dtype,ring", TIE_FORMS, ids=TIE_IDS)
@pytest.mark.parametrize("Cn,D", [(2, 256), (3, 512)])
def test_a_repeated_row_gives_repeated_statistics(dev, dtype, ring, Cn, D):
    """One row, 100 times over three slides: every column of `stats` holds the same bits -- the MFMA layout and the row
    epilogue's cross-lane top-2 and background merges do not depend on where a row sits in its tile.  At scale 1 and 2^6."""
    W, We = synth.make_bank(1000 + Cn, D, Cn)
    bank = _bank(dev, W, We, dtype)
    x = V.repeated_rows(1001, D, We, Cn).to(dtype)
    for s in (0, 6):
        xs = V.scaled_pow2(x, s)
        for mask in (None, V.half_mask(100, 14)):
            st = _scores(dev, xs, REP_SIZES, Cn, bank, mask, ring)[:, _valid(REP_SIZES, mask)]
            assert torch.isfinite(st).all() and float(st[:Cn].abs().max()) > 0
            assert torch.equal(_bits(st), _bits(st[:, :1].expand_as(st))), f"2^{s}: the statistics depend on the row's place"


@pytest.mark.parametrize("dtype,ring", TIE_FORMS, ids=TIE_IDS)
@pytest.mark.parametrize("Cn,D", [(2, 256), (3, 512)])
def test_zero_rows_give_zero_logits_and_a_uniform_softmax(dev, dtype, ring, Cn, D):
    """A slide whose first 40 and last 7 rows are zeros: logits exactly +0, gap exactly +0, background sum and maximum
    zero; softmax exactly 1/2 for C = 2.  For C = 3 the kernel gives exp2(0) * rcp(3) = 0.3333333432674408 (0x3EAAAAAB, the
    fp32 nearest 1/3) in every storage and in both kernel forms on an MI355X: held to TIGHT of 1/3 and to one value for
    all zero rows and classes; the value is printed."""
    W, We = synth.make_bank(1010 + Cn, D, Cn)
    bank = _bank(dev, W, We, dtype)
    xs = torch.cat([synth.make_bag(1011, ZERO_SIZES[0], D, We, Cn, label=0), V.zero_block_slide(1012, 100, D, We, Cn)]).to(dtype)
    st = _scores(dev, xs, ZERO_SIZES, Cn, bank, None, ring)
    o = ZERO_SIZES[0]
    zero = torch.cat([torch.arange(o, o + V.ZERO_HEAD), torch.arange(o + V.ZERO_HEAD + 100, o + ZERO_SIZES[1])])
    z = st[:, zero]
    assert (_bits(z[:Cn]) == 0).all(), "logits of zero rows are not +0"
    assert (_bits(z[2 * Cn]) == 0).all(), "gap of zero rows is not +0"
    assert (z[2 * Cn + 1:] == 0).all()
    soft = z[Cn:2 * Cn]
    if Cn == 2:
        assert (soft == 0.5).all()
    else:
        print(f"softmax of a zero row, C = 3: {sorted(set(soft.flatten().tolist()))}")
        assert float((soft.to(torch.float64) - 1.0 / 3.0).abs().max()) <= TIGHT
        assert torch.equal(_bits(soft), _bits(soft[:1, :1].expand_as(soft)))
    ordinary = st[:, o + V.ZERO_HEAD:o + V.ZERO_HEAD + 100]
    assert float(ordinary[:Cn].abs().min()) > 0
    _check_against_float64(torch.cat([st[:, :o], ordinary], 1), torch.cat([xs[:o], xs[o + V.ZERO_HEAD:o + V.ZERO_HEAD + 100]]),
                           W, We, Cn, "rows around the zero blocks")


def _phase_a(dev, xs, sizes, Cn, bank, j, discard, mask, compact=None):
    """phase_a with topj = j -> (n_sel, sel_idx, sel_row) on the host; compact: the statistics layout of a wide bank."""
    E = _engine()
    b = E.SlideBatch(xs.to(dev).contiguous(), sizes, Cn, Cn + 4, j, 10, discard, mask=mask)
    keep = E.COMPACT_STATS
    if compact is not None:
        E.COMPACT_STATS = compact
    try:
        b.phase_a(bank)
    finally:
        E.COMPACT_STATS = keep
    torch.cuda.synchronize()
    if compact is not None:
        assert bool(b.c.flags & E._lib.MOC_STATS_COMPACT) == compact
    return b.n_sel.cpu().tolist(), b.sel_idx.cpu(), b.sel_row.cpu()


def _check_selection_rule(dev, xs, sizes, Cn, bank, j, discard, mask, compact, what):
    """sel_idx against the restated rule applied to the kernel's own (full-layout) statistics; -> boundary ties met."""
    st = _scores(dev, xs, sizes, Cn, bank, mask)
    n_sel, sel_idx, sel_row = _phase_a(dev, xs, sizes, Cn, bank, j, discard, mask, compact)
    ties = 0
    for s_i, (off, nk, kept) in enumerate(V.slot_ranges(sizes, mask)):
        exp = V.select_rule(st[:, off:off + nk], Cn, j, discard)
        got = sel_idx[off:off + n_sel[s_i]].tolist()
        assert got == exp, f"{what}: slide {s_i} ({nk} kept rows, topj {j}): got {got[:12]} ..., rule {exp[:12]} ..."
        assert sel_row[off:off + n_sel[s_i]].tolist() == (off + kept[exp]).tolist()
        ties += V.boundary_ties(st[:, off:off + nk], Cn, j)
    return ties


SELECT_CASES = [(F32, 2, 256, None), (BF16, 3, 512, None), (F16, 2, 512, None), (BF16, 30, 512, True), (BF16, 30, 512, False)]
SELECT_IDS = ["fp32-C2", "bf16-C3", "fp16-C2", "bf16-C30-compact", "bf16-C30-full"]


@pytest.mark.parametrize("dtype,Cn,D,compact", SELECT_CASES, ids=SELECT_IDS)
def test_selection_among_repeated_rows_takes_the_lowest_rows(dev, dtype, Cn, D, compact):
    """phase_a over the repeated row with topj = 10, fewer than the tied rows of any slide: every key ties, the row order
    decides.  Default and compact statistics layouts (the thirty-class bank), with and without a mask."""
    W, We = synth.make_bank(1020 + Cn, D, Cn)
    bank = _bank(dev, W, We, dtype)
    xs = V.repeated_rows(1021, D, We, Cn).to(dtype)
    for discard in ((), ("topk", "bottomk")):
        for mask in (None, V.half_mask(100, 15)):
            ties = _check_selection_rule(dev, xs, REP_SIZES, Cn, bank, 10, discard, mask, compact, f"discard {discard}")
            assert ties > 0
            n_sel, sel_idx, _ = _phase_a(dev, xs, REP_SIZES, Cn, bank, 10, discard, mask, compact)
            for s_i, (off, nk, _) in enumerate(V.slot_ranges(REP_SIZES, mask)):
                assert sel_idx[off:off + n_sel[s_i]].tolist() == list(range(min(10, nk)))


@pytest.mark.parametrize("dtype,Cn,D,compact", SELECT_CASES, ids=SELECT_IDS)
def test_selection_with_a_boundary_inside_the_zero_rows(dev, dtype, Cn, D, compact):
    """phase_a over the slide with zero blocks, topj chosen (from the float64 statistics of the input) so that the
    smallest-background selector's boundary falls among the tied zero rows."""
    W, We = synth.make_bank(1030 + Cn, D, Cn)
    bank = _bank(dev, W, We, dtype)
    xs = torch.cat([synth.make_bag(1031, ZERO_SIZES[0], D, We, Cn, label=0), V.zero_block_slide(1032, 100, D, We, Cn)]).to(dtype)
    for mask in (None, V.half_mask(sum(ZERO_SIZES), 16)):
        off, nk, kept = V.slot_ranges(ZERO_SIZES, mask)[1]
        bg = V.stats64(xs[off + kept], W, We, Cn)[2 * Cn + 1]
        n_neg, n_zero = int((bg < 0).sum()), int((bg == 0).sum())
        assert n_zero >= 12
        j = n_neg + n_zero // 2
        for discard in ((), ("delta_softmax",)):
            ties = _check_selection_rule(dev, xs, ZERO_SIZES, Cn, bank, j, discard, mask, compact, f"discard {discard}")
            assert ties > 0, "no key column ties across the boundary"


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("Cn", [2, 3])
def test_selection_is_unchanged_by_power_of_two_scaling(dev, dtype, Cn):
    """With delta_softmax discarded every key is of degree one: sel_idx and n_sel on 2^s X equal those on X exactly.
    With it enabled (C = 2, where a softmax column is monotone in the logit difference at any scale; for C = 3 the
    ranking of a softmax column across rows is not scale-invariant in exact arithmetic either) the selections agree
    outside helpers.ambiguous_rows of the scaled keys."""
    D, sizes, j = 256, [17, 300, 120], 20
    W, We = synth.make_bank(1040 + Cn, D, Cn)
    bank = _bank(dev, W, We, dtype)
    xs = _rows(1041, sizes, D, We, Cn, dtype)
    scales = (1, 4) if dtype == F16 else (-7, -1, 1, 6)
    for mask in (None, V.half_mask(sum(sizes), 17)):
        for discard in (("delta_softmax",), ()) if Cn == 2 else (("delta_softmax",),):
            n0, idx0, row0 = _phase_a(dev, xs, sizes, Cn, bank, j, discard, mask)
            for s in scales:
                xs_s = V.scaled_pow2(xs, s)
                n1, idx1, row1 = _phase_a(dev, xs_s, sizes, Cn, bank, j, discard, mask)
                if discard:
                    assert n1 == n0
                    for s_i, (off, _, _) in enumerate(V.slot_ranges(sizes, mask)):
                        assert torch.equal(idx1[off:off + n1[s_i]], idx0[off:off + n0[s_i]]), f"2^{s}: slide {s_i}"
                        assert torch.equal(row1[off:off + n1[s_i]], row0[off:off + n0[s_i]])
                    continue
                st = _scores(dev, xs_s, sizes, Cn, bank, mask)
                for s_i, (off, nk, _) in enumerate(V.slot_ranges(sizes, mask)):
                    a, b = set(idx0[off:off + n0[s_i]].tolist()), set(idx1[off:off + n1[s_i]].tolist())
                    amb = H.ambiguous_rows(V.keys_of(st[:, off:off + nk], Cn), j)
                    assert (a ^ b) <= amb, f"2^{s}: slide {s_i}: rows {sorted((a ^ b) - amb)} differ outside the tie band"


# ------------------------------------------------------------------ 3. meta forward off the sphere
def _h1(dev, model, x, n_slides, rows):
    """H1 of moc_meta_forward over x [n_slides * rows, D] (device, its storage type), keep_hidden=True."""
    E = _engine()
    D = x.size(1)
    b = E.CompactBatch(n_slides, n_slides * rows, rows, D, x.dtype, 2, 3, rows, 1, dev, X=x)
    b.n_sel.fill_(rows)
    b.set_layout([i * rows for i in range(n_slides + 1)])
    meta = E.MetaState(model)
    E.meta_forward(b, meta, 0, n_slides, 0, keep_hidden=True)
    torch.cuda.synchronize()
    return b.meta_ws()[0]["H1"][:n_slides * rows].cpu()


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("D", [256, 512])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval128"])
def test_hidden_layer_scales_exactly_with_power_of_two_rows(dev, dtype, D, train):
    """b1 zeroed before the MetaState is built: H1 = relu(x W1^T) is homogeneous of degree one, H1(2^s X) == 2^s H1(X)
    as bits.  fp32 rows (the truncating three-term split is a bit mask: scale-invariant), bf16 rows, fp16 rows
    (upscaling only); the training kernel (one slide of 300 rows) and the 128-row evaluation kernel (four slides of 1,024)."""
    from moc_amd import main_moc as M
    n_slides, rows = (1, 300) if train else (4, 1024)
    torch.manual_seed(21 + D)
    model = M.senet(D, 4).to(dev)
    with torch.no_grad():
        model.model[0].bias.zero_()
    g = torch.Generator().manual_seed(22 + D)
    x = torch.randn(n_slides * rows, D, generator=g).to(dtype)
    base = _h1(dev, model, x.to(dev), n_slides, rows)
    assert torch.isfinite(base).all() and float((base > 0).float().mean()) > 0.25 and float((base == 0).float().mean()) > 0.25
    for s in _pow2_scales(dtype):
        got = _h1(dev, model, V.scaled_pow2(x, s).to(dev), n_slides, rows)
        bad = _bits(got) != _bits(base * float(2.0 ** s))
        assert not bad.any(), f"2^{s}: {int(bad.sum())} of {bad.numel()} hidden units do not scale exactly; first {torch.nonzero(bad)[0].tolist()}"


def _gpu_case(dev, case):
    """The case's two slides through phase A (topj above every slide: all rows), the meta forward and moc_train_grad per
    slide -> [(gates, mixed, pooled, loss, pred, [grads])] per slide, numpy."""
    from moc_amd import engine as E, main_moc as M
    Cn, D, n = V.GRAD_C, V.GRAD_D, len(V.GRAD_SIZES)
    model = M.senet(D, 4)
    model.load_state_dict(case.state)
    model = model.to(dev)
    X = torch.cat(case.xs).to(dev).contiguous()
    batch = E.SlideBatch(X, list(V.GRAD_SIZES), Cn, Cn + 4, V.GRAD_TOPJ, V.GRAD_K, [])
    batch.phase_a(E.Bank.get(case.W, case.We, case.dtype, dev))
    lab = torch.tensor(case.labels, dtype=torch.int64, device=dev)
    meta = E.MetaState(model, None, need_grads=True)
    E.meta_forward(batch, meta, 0, n, 15, keep_hidden=True)
    torch.cuda.synchronize()
    t, _ = batch.meta_ws()
    assert batch.n_sel.cpu().tolist() == list(V.GRAD_SIZES)
    gates, mixed = t["gates"].cpu().numpy().astype(np.float64), t["mixed"].cpu().numpy().astype(np.float64)
    out = []
    for s_i, (off, rows, _) in enumerate(V.slot_ranges(V.GRAD_SIZES)):
        E.train_grad(batch, meta, lab, s_i, 15)
        torch.cuda.synchronize()
        out.append((gates[off:off + rows], mixed[:, off:off + rows].T, t["pooled"][s_i].cpu().numpy().astype(np.float64),
                    float(t["loss"][s_i].cpu()), int(t["pred"][s_i].cpu()), [g.cpu().numpy().astype(np.float64) for g in meta.grads]))
    return out


def _assert_measured(got, r32, r64, base_abs, base_rel, what):
    allowed = V.measured_allowed(base_abs, base_rel, r32, r64)
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(r64, dtype=np.float64))
    print(f"{what}: error {float(err.max()):.3e}, allowed {float(np.min(allowed)):.3e} "
          f"(reference noise {float(np.abs(np.asarray(r32, dtype=np.float64) - np.asarray(r64, dtype=np.float64)).max()):.3e})")
    assert np.isfinite(np.asarray(got, dtype=np.float64)).all(), f"{what}: not finite"
    assert (err <= allowed).all(), f"{what}: off by {float(err.max()):.3e}, allowed {float(np.min(allowed)):.3e}"


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("scale", V.FWD_SCALES, ids=lambda s: f"x{s:g}")
def test_gates_and_mixed_scores_at_scale_against_the_float64_oracle(dev, dtype, scale):
    """Rows times 2^-6, 0.3, 5, 32: the gates and the mixed scores of every row against oracle.moc_oracle in float64, under
    the measured rule on helpers.ATOL."""
    case = V.grad_case(dtype, scale)
    for s_i, (gates, mixed, *_rest) in enumerate(_gpu_case(dev, case)):
        r32, r64 = case.ref32[s_i], case.ref[s_i]
        _assert_measured(gates, r32.gates, r64.gates, H.ATOL, 0.0, f"x{scale:g} slide {s_i} gates")
        _assert_measured(mixed, r32.mixed, r64.mixed, H.ATOL, 0.0, f"x{scale:g} slide {s_i} mixed")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("scale", V.GRAD_SCALES, ids=lambda s: f"x{s:g}")
def test_pooling_cross_entropy_and_gradients_at_scale(dev, dtype, scale):
    """moc_train_grad at row scales 2^-6, 1/8, 5, 32, 200 against autograd on the oracle in float64 (double model, double
    inputs), topj above every slide so that selection cannot differ.  The measured rule: pooled and loss at helpers.ATOL,
    each gradient tensor at 2e-6 + 1e-4 |g64|, plus four times the reference's own fp32-against-float64 distance on that
    tensor.  At 200 the cross entropy saturates (loss64 5.1e-7 and 1.3e-7): what is held there is finite outputs, the loss
    and the pooled logits under the rule, and pred.  The gradients at 200 are printed, not held: on an MI355X g_W1 of slide 0
    is off by 1.1e-5 on max|g64| = 1.2e-5 where the rule would allow 4.9e-6 (fp32 rows; bf16: 1.1e-5 / 4.4e-6), and the loss
    reads exactly 0.  Located in ce_wave0 (moc_step_shared.h; the same lines in moc_step_tiles.hip and moc_step_pool.hip):
    lse = mx + logf(se) rounds log(se) = 5e-7 away against mx = 8 (half an ulp of mx is 4.8e-7), so loss = lse - x_y and
    d loss / d pooled = expf(x - lse) - onehot carry an ABSOLUTE error of up to ulp(mx) / 2 -- fp32 noise on a
    probability, but the whole of a saturated slide's gradient.  torch's log-softmax keeps log(se) apart from mx and is
    off by a twentieth there.  Not changed here: it would move the bits of every training step.
    Reference noise max|g32 - g64| / max|g64| (slides 0, 1): fp32 rows 2^-6: 1.4e-5, 1.7e-6; 1/8: 4.6e-7, 1.3e-6; 5: 2.2e-7,
    4.9e-7; 32: 1.5e-6, 6.7e-7; 200: 6.2e-2, 6.1e-2.  bf16 rows 2^-6: 2.1e-6, 4.4e-6; 1/8: 3.6e-7, 2.8e-6; 5: 1.3e-7, 7.0e-7;
    32: 3.4e-6, 6.0e-7; 200: 5.3e-2, 4.4e-2."""
    case = V.grad_case(dtype, scale)
    for s_i, (_, _, pooled, loss, pred, grads) in enumerate(_gpu_case(dev, case)):
        r32, r64 = case.ref32[s_i], case.ref[s_i]
        what = f"x{scale:g} slide {s_i}"
        assert np.isfinite(pooled).all() and np.isfinite(loss) and all(np.isfinite(g).all() for g in grads)
        _assert_measured(loss, r32.loss, r64.loss, H.ATOL, 0.0, f"{what} loss")
        assert pred == r64.pred
        _assert_measured(pooled, r32.pooled, r64.pooled, H.ATOL, 0.0, f"{what} pooled")
        for name, g, g32, g64 in zip(("g_W1", "g_b1", "g_W2", "g_b2"), grads, r32.grads, r64.grads):
            if scale >= 200.0:
                print(f"{what} {name}: error {float(np.abs(g - g64).max()):.3e} on max|g64| {float(np.abs(g64).max()):.3e}, the rule "
                      f"would allow {float(np.min(V.measured_allowed(2e-6, 1e-4, g32, g64))):.3e}")
                continue
            _assert_measured(g, g32, g64, 2e-6, 1e-4, f"{what} {name}")


# ------------------------------------------------------------------ 5. the fp16 bank's range
def test_fp16_bank_refuses_a_weight_of_two_or_more(dev):
    """moc_prepare_bank: the fp16 image holds w 2^14, so a bank with an element |w| >= 2 is refused for fp16 storage, with
    a message that names the way out; fp32 and bf16 storage take the same bank and match float64."""
    E = _engine()
    Cn, D = 2, 256
    W, We = synth.make_bank(1050, D, Cn)
    W, We = W.clone(), We.clone()
    xs = _rows(1051, SIZES, D, We, Cn, F32)
    refusal = (r"fp16 bags need classifier weights with \|w\| < 2 \(unit-norm columns\); "
               r"use bf16 or fp32 storage for this bank")
    Wa, Wea = W.clone(), We.clone()
    Wa[7, 1] = Wea[7, 1] = 2.0                                        # a foreground weight AT the bound
    with pytest.raises(AssertionError, match=refusal):
        E.Bank(Wa, Wea, F16, dev)
    Web = We.clone()
    Web[100, Cn + 2] = -2.5                                           # a background weight beyond it
    with pytest.raises(AssertionError, match=refusal):
        E.Bank(W, Web, F16, dev)
    Wc, Wec = W.clone(), We.clone()
    Wc[7, 1] = Wec[7, 1] = Wec[100, Cn + 2] = 1.999                   # (just inside: accepted)
    E.Bank(Wc, Wec, F16, dev)
    W, We = Wa, Wea.clone()
    We[100, Cn + 2] = -2.5
    for dtype in (F32, BF16):
        got = _scores(dev, xs.to(dtype), SIZES, Cn, _bank(dev, W, We, dtype))
        _check_against_float64(got, xs.to(dtype), W, We, Cn, f"{NAME[dtype]} bank with |w| >= 2")
