"""moc_meta_forward_by_slide: the evaluation forward in which every slide names the meta-learner that scores it (the
evaluation of several runs in one pass).  For a slide of model r the mixed scores at its union slots are BIT-identical to
moc_meta_forward with model r alone, for all three storages, the full and the compact statistics layout, candidates from
the statistics, and any assignment of slides to models."""
import ctypes as C

import numpy as np
import pytest
import torch

from moc_amd import _lib, engine, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(gpu_device):
    return gpu_device


def _models(R, D, dev):
    from moc_amd import main_moc as M
    out = []
    for r in range(R):
        torch.manual_seed(300 + r)
        out.append(M.senet(D, 4).to(dev))
    return out


def _batch(dev, n, Cc, D, dtype, j, discard=(), seed=0, lo=700, hi=2600):
    W, We = synth.make_bank(41 + Cc, D, Cc)
    g = np.random.default_rng(900 + seed)
    sizes = [int(v) for v in g.integers(lo, hi, size=n)]
    bags, _ = synth.make_slide_set(7000 + seed, sizes, D, We, Cc)
    X = torch.cat([b.to(dtype) for b in bags]).to(dev)
    bank = engine.Bank(W, We, dtype, dev)
    batch = engine.SlideBatch(X, sizes, Cc, We.size(1), j, 10, discard)
    return batch, bank


def _alone(batch, models, use):
    """mixed [R, C, T] of moc_meta_forward with every model alone (sentinel where nothing was written)."""
    t, _ = batch.meta_ws()
    out = []
    for m in models:
        t["mixed"].fill_(float("nan"))
        engine.meta_forward(batch, engine.MetaState(m), 0, batch.n_slides, use, keep_hidden=False)
        out.append(t["mixed"].clone())
    return out


def _check(batch, models, assign, use):
    R, n = len(models), batch.n_slides
    ref = _alone(batch, models, use)
    arena = engine.ModelArena.of_models(models)
    t, _ = batch.meta_ws()
    t["mixed"].fill_(float("nan"))
    mos = torch.tensor(assign, dtype=torch.int32, device=batch.device)
    engine.meta_forward_by_slide(batch, arena, 0, R, mos, 0, n, use)
    torch.cuda.synchronize()
    got = t["mixed"].view(torch.int32).cpu()
    n_sel = batch.n_sel.cpu().tolist()
    checked = 0
    for b in range(n):
        o, S = batch.row_off_host[b], n_sel[b]
        assert S > 0
        want = ref[assign[b]][:, o:o + S].view(torch.int32).cpu()
        assert torch.equal(got[:, o:o + S], want), f"slide {b} (model {assign[b]}): mixed differs from the model alone"
        assert not torch.isnan(t["mixed"][:, o:o + S]).any()
        checked += S
    assert checked > 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Cc,D,R,j", [(2, 512, 3, 400), (3, 1024, 16, 150), (30, 512, 3, 40), (2, 1024, 1, 300), (30, 1024, 16, 30)])
def test_every_slide_gets_its_models_bits(dev, dtype, Cc, D, R, j):
    n = 19 if R == 16 else 9
    batch, bank = _batch(dev, n, Cc, D, dtype, j, seed=Cc + R)
    batch.phase_a(bank, for_eval=True)               # C > 4: candidates from the (compact, for a wide bank) statistics
    models = _models(R, D, dev)
    use = engine.eval_use_bits(())
    interleaved = [b % R for b in range(n)]
    _check(batch, models, interleaved, use)
    per = (n + R - 1) // R
    blocked = [min(b // per, R - 1) for b in range(n)]
    _check(batch, models, blocked, use)
    if R >= 3:                                       # one model that owns no slide
        _check(batch, models, [0 if b % 2 else R - 1 for b in range(n)], use)


def test_full_statistics_layout_from_stats_and_a_discard_set(dev, monkeypatch):
    models = _models(3, 512, dev)
    # wide bank with the FULL statistics layout (cand_mode 1)
    monkeypatch.setattr(engine, "COMPACT_STATS", False)
    batch, bank = _batch(dev, 7, 30, 512, torch.bfloat16, 40, seed=5)
    batch.phase_a(bank, for_eval=True)
    assert batch.c.flags & _lib.MOC_CAND_FROM_STATS and not (batch.c.flags & _lib.MOC_STATS_COMPACT)
    _check(batch, models, [b % 3 for b in range(7)], engine.eval_use_bits(()))
    monkeypatch.undo()
    # a discard set: fewer selectors in the union, fewer terms in the mix; materialised candidates (as in training)
    discard = ("delta_diff", "bottomk")
    batch, bank = _batch(dev, 8, 2, 512, torch.float32, 300, discard=discard, seed=6)
    batch.phase_a(bank, for_eval=False)
    _check(batch, models, [2, 2, 0, 1, 1, 0, 2, 1], engine.eval_use_bits(discard))


def test_one_model_is_meta_forward_and_a_slide_range_leaves_the_rest_alone(dev):
    batch, bank = _batch(dev, 6, 2, 512, torch.float32, 400, seed=9)
    batch.phase_a(bank, for_eval=True)
    models = _models(2, 512, dev)
    use = engine.eval_use_bits(())
    _check(batch, models[:1], [0] * 6, use)
    # slides [2, 5) only: the other slides' slots keep what they held; an out-of-range index is clamped, not followed
    ref = _alone(batch, models, use)
    t, _ = batch.meta_ws()
    t["mixed"].fill_(7.0)
    mos = torch.tensor([0, 0, 1, 99, -5, 1], dtype=torch.int32, device=dev)
    engine.meta_forward_by_slide(batch, engine.ModelArena.of_models(models), 0, 2, mos, 2, 3, use)
    torch.cuda.synchronize()
    n_sel, off = batch.n_sel.cpu().tolist(), batch.row_off_host
    for b, r in ((2, 1), (3, 1), (4, 0)):            # 99 -> the last model, -5 -> model 0
        assert torch.equal(t["mixed"][:, off[b]:off[b] + n_sel[b]], ref[r][:, off[b]:off[b] + n_sel[b]])
    for b in (0, 1, 5):
        assert bool((t["mixed"][:, off[b]:off[b + 1]] == 7.0).all())


def test_refused_arguments_are_errors_not_faults(dev):
    batch, bank = _batch(dev, 5, 2, 512, torch.float32, 200, seed=11)
    models = _models(2, 512, dev)
    arena = engine.ModelArena.of_models(models)
    mos = torch.zeros(5, dtype=torch.int32, device=dev)
    _, ws = batch.meta_ws()
    lib = _lib.lib()

    def call(b=None, mc=None, runs=None, mp=mos.data_ptr(), w=ws, s0=0, n=5):
        m0, r0 = arena.group(0, 2)
        rc = lib.moc_meta_forward_by_slide(C.byref(b or batch.c), C.byref(mc or m0), C.byref(runs or r0), mp, C.byref(w), s0, n,
                                           15, engine._stream())
        return rc, lib.moc_last_error().decode()

    batch.phase_a(bank, for_eval=True)
    assert call()[0] == 0
    bad = []
    masked = _lib.MocBatch.from_buffer_copy(batch.c)
    masked.mask = batch.sel_flag.data_ptr()
    masked.kept, masked.n_kept = batch.sel_idx.data_ptr(), batch.n_sel.data_ptr()
    bad.append(("masked", call(b=masked)))
    bare = _lib.MocBatch.from_buffer_copy(batch.c)
    bare.sel_row = None
    bad.append(("phase-A", call(b=bare)))
    bad.append(("model_of_slide", call(mp=None)))
    for k in (0, 17):
        r = _lib.MocRuns.from_buffer_copy(arena.group(0, 2)[1])
        r.n_runs = k
        bad.append(("n_runs", call(runs=r)))
    r = _lib.MocRuns.from_buffer_copy(arena.group(0, 2)[1])
    r.slide_stride = 3
    bad.append(("slide_stride", call(runs=r)))
    r = _lib.MocRuns.from_buffer_copy(arena.group(0, 2)[1])
    r.par_stride = 64 * 512
    bad.append(("par_stride", call(runs=r)))
    r = _lib.MocRuns.from_buffer_copy(arena.group(0, 2)[1])
    r.image_stride = 1024
    bad.append(("image_stride", call(runs=r)))
    m = _lib.MocMeta.from_buffer_copy(arena.group(0, 2)[0])
    m.D = 1024
    bad.append(("meta D", call(mc=m)))
    bad.append(("slide range", call(s0=3, n=3)))
    bad.append(("slide range", call(s0=-1, n=2)))
    bad.append(("slide range", call(n=0)))
    w = type(ws).from_buffer_copy(ws)
    w.mixed = None
    bad.append(("mixed", call(w=w)))
    for what, (rc, msg) in bad:
        assert rc == 1, (what, rc, msg)                  # MOC_EINVAL, before anything was launched
        assert "moc_meta_forward_by_slide" in msg and what.split()[0].lower() in msg.lower(), (what, msg)
    torch.cuda.synchronize()
