"""The training forward's tail (meta_forward_ksplit_kernel: gate chain on 16-byte LDS operands, tile ranks on the score
words): the same bits as the forwards whose tail is the older code.  Needs an MI355X: run with -m gpu.

One slide of S selected fp32 rows goes through the sixteen-wave kernel (one-slide launch), through the four-wave kernel
(MOC_FORWARD_FOUR_WAVES: the older gate chain) and through the 128-row evaluation kernel (the launch of all four slides of
the batch, cap >= 1,024: the older gate chain, no records): hidden layer, gates and mixed scores must be equal,
torch.equal.  With tile records (a training step of the slide) the sixteen-wave and the four-wave kernel must leave the
same record arrays -- key, rid, lam, sc -- and rho, and the step the same parameters, moments and loss.  Both rank with
the same device function, so the records are also checked against a ranking of the mixed scores done on the host.

C = 1 is not a shape the library takes (every entry requires 2 <= C < Ce): that case asserts the refusal on both routes.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TILE_R = 4
N_SLIDES, CAP, TOPJ, TOPK = 4, 1024, 400, 10
OTHERS = [3, 16, 1]                                   # selected rows of the three slides beside the one under test


@pytest.fixture(scope="module")
def dev(gpu_device):
    return gpu_device


def _batch(dev, S, Cc, D, seed, ties=False):
    """Four slides in a CompactBatch (the selected rows themselves, their candidate scores): slide 0 has S rows."""
    from moc_amd import engine as E
    n_sel = [S] + OTHERS
    off = [0]
    for n in n_sel:
        off.append(off[-1] + n + 3)                   # (three unselected slots behind every slide)
    T = max(off[-1], CAP)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, D, generator=g)
    cand = torch.randn(2 * Cc + 2, T, generator=g)
    if ties:                                          # tile 1 (rows 16..31): sixteen equal rows; tile 0: rows 3 and 9 equal
        x[16:32] = x[16]
        cand[:, 16:32] = cand[:, 16:17]
        x[9] = x[3]
        cand[:, 9] = cand[:, 3]
    b = E.CompactBatch(N_SLIDES, T, CAP, D, torch.float32, Cc, Cc + 4, TOPJ, TOPK, dev, X=x.to(dev))
    b.cand.copy_(cand)
    b.n_sel.copy_(torch.tensor(n_sel, dtype=torch.int32))
    b.set_layout(off)
    torch.cuda.synchronize()
    return b, n_sel, off


def _model(dev, D, seed):
    from moc_amd import main_moc as M
    torch.manual_seed(seed)
    return M.senet(D, 4).to(dev)


def _set_four(b, four):
    from moc_amd import _lib
    b.c.flags = (b.c.flags & ~_lib.MOC_FORWARD_FOUR_WAVES) | (_lib.MOC_FORWARD_FOUR_WAVES if four else 0)


def _forward_outputs(b, meta, launches):
    from moc_amd import engine as E
    t = b.meta_ws()[0]
    for k in ("mixed", "H1", "gates"):
        t[k].zero_()
    for s0, n in launches:
        E.meta_forward(b, meta, s0, n, 15)
    torch.cuda.synchronize()
    return {k: t[k].clone() for k in ("mixed", "H1", "gates")}


def _assert_rows_equal(a, c, n_sel, off, what):
    for i, n in enumerate(n_sel):
        o = off[i]
        assert torch.equal(a["mixed"][:, o:o + n], c["mixed"][:, o:o + n]), (what, "mixed", i)
        assert torch.equal(a["H1"][o:o + n], c["H1"][o:o + n]), (what, "H1", i)
        assert torch.equal(a["gates"][o:o + n], c["gates"][o:o + n]), (what, "gates", i)


@pytest.mark.parametrize("D", [256, 512])
@pytest.mark.parametrize("Cc", [1, 2, 3])
@pytest.mark.parametrize("S", [1, 15, 16, 17, 33, 257])
def test_tail_outputs_equal_the_four_wave_and_the_128_row_forward(dev, S, Cc, D):
    from moc_amd import engine as E
    b, n_sel, off = _batch(dev, S, Cc, D, 100 * S + 10 * Cc + D)
    meta = E.MetaState(_model(dev, D, 3))
    singles = [(i, 1) for i in range(N_SLIDES)]
    if Cc < 2:
        for four in (False, True):
            _set_four(b, four)
            with pytest.raises((AssertionError, RuntimeError), match="2 <= C"):
                E.meta_forward(b, meta, 0, 1, 15)
        return
    _set_four(b, False)
    new = _forward_outputs(b, meta, singles)                    # the sixteen-wave kernel, a slide per launch
    assert float(new["H1"][:S].abs().sum()) > 0 and float(new["gates"][:S].min()) > 0
    _set_four(b, True)
    four = _forward_outputs(b, meta, singles)                   # the four-wave kernel
    _set_four(b, False)
    ev = _forward_outputs(b, meta, [(0, N_SLIDES)])             # four slides per launch, bound 1,024: the 128-row kernel
    _assert_rows_equal(new, four, n_sel, off, "four waves")
    _assert_rows_equal(new, ev, n_sel, off, "128 rows")


def _records(buf, total, Cc):
    """The arrays of a tile-record buffer (moc_meta_internal.h tile_carve)."""
    ns = ((total >> 4) + N_SLIDES + 2) * Cc * TILE_R
    lam = buf[:ns * 16].view(torch.float32).view(ns, 4)
    sc = buf[ns * 16:ns * 32].view(torch.float32).view(ns, 4)
    key = buf[ns * 32:ns * 40].view(torch.int64)
    rid = buf[ns * 40:ns * 48].view(torch.int64)
    rho = buf[ns * 48:ns * 48 + (ns // TILE_R) * 4].view(torch.int32)
    return dict(lam=lam, sc=sc, key=key, rid=rid, rho=rho)


def _train_step_records(dev, S, Cc, D, ties):
    """One training step of slide 0 (forward with tile records, then the step over them), through the sixteen-wave
    forward and through the four-wave one, each on its own copy of the model, optimizer and (zeroed) record buffer."""
    from moc_amd import _lib, engine as E
    b, n_sel, off = _batch(dev, S, Cc, D, 7 + 100 * S + 10 * Cc + D, ties=ties)
    t, ws = b.meta_ws()
    lab = torch.tensor([i % Cc for i in range(N_SLIDES)], dtype=torch.int64, device=dev)
    nb = _lib.lib().moc_tile_ws_bytes(b.total, N_SLIDES, Cc)
    model0 = _model(dev, D, 5)
    out = {}
    for four in (False, True):
        _set_four(b, four)
        model = copy.deepcopy(model0)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
        meta = E.MetaState(model, opt)
        rec = torch.zeros(nb, dtype=torch.uint8, device=dev)
        ws_rec = _lib.MocMetaWs.from_buffer_copy(ws)
        ws_rec.tile_ws, ws_rec.tile_ws_bytes = rec.data_ptr(), nb
        assert _lib.lib().moc_train_runs_mode(C.byref(b.c), C.byref(ws_rec)) == 1, "the shape must be one the tile-record step serves"
        for k in ("mixed", "H1", "gates", "loss"):
            t[k].zero_()
        _lib.check(_lib.lib().moc_train_steps(C.byref(b.c), C.byref(meta.c), C.byref(ws_rec), lab.data_ptr(), 0, 1,
                                              E.train_use_bits([]), E._stream()), "moc_train_steps")
        torch.cuda.synchronize()
        out[four] = dict(rec=rec, fwd={k: t[k].clone() for k in ("mixed", "H1", "gates")}, loss=t["loss"][:1].clone(),
                         params=[p.detach().clone() for p in model.parameters()],
                         moments=[opt.state[p][k].clone() for p in model.parameters() for k in ("exp_avg", "exp_avg_sq")])
    _set_four(b, False)
    return b, n_sel, off, out


def _key_desc(f32):
    """moc_key_desc: the score as an unsigned word that orders like the float (zeros canonical)."""
    u = f32.view(np.uint32).copy()
    u[(u << np.uint32(1)) == 0] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _assert_records_as_ranked_on_the_host(b, Cc, S, off, fwd, rec):
    """Slide 0's records against a ranking done here: per (class, tile) the sixteen keys (score word of the mixed score,
    0 for an absent row) << 32 | ~row, sorted descending; records = the first four with the row's id, gates and candidate
    scores, rho = the fifth's score word."""
    cap = (off[1] - off[0] + 15) // 16
    mixed, gates, cand = fwd["mixed"].cpu().numpy(), fwd["gates"].cpu().numpy(), b.cand.cpu().numpy()
    key = rec["key"][:Cc * cap * TILE_R].view(Cc, cap, TILE_R).cpu().numpy().view(np.uint64)
    rid = rec["rid"][:Cc * cap * TILE_R].view(Cc, cap, TILE_R).cpu().numpy()
    lam = rec["lam"][:Cc * cap * TILE_R].view(Cc, cap, TILE_R, 4).cpu().numpy()
    sc = rec["sc"][:Cc * cap * TILE_R].view(Cc, cap, TILE_R, 4).cpu().numpy()
    rho = rec["rho"][:Cc * cap].view(Cc, cap).cpu().numpy().view(np.uint32)
    for c in range(Cc):
        for x in range((S + 15) // 16):
            rows = np.arange(16 * x, 16 * x + 16)
            hi = np.where(rows < S, _key_desc(np.ascontiguousarray(mixed[c, np.minimum(rows, S - 1)])), 0).astype(np.uint64)
            keys = (hi << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - rows.astype(np.uint64))
            order = np.argsort(keys)[::-1]
            assert key[c, x].tolist() == keys[order[:TILE_R]].tolist(), (c, x)
            assert int(rho[c, x]) == int(keys[order[TILE_R]] >> np.uint64(32)), (c, x)
            for r in range(TILE_R):
                row = int(rows[order[r]])
                if row >= S:
                    continue
                assert rid[c, x, r] == off[0] + row                          # (CompactBatch: sel_row is the identity)
                assert np.array_equal(lam[c, x, r], gates[row])
                assert np.array_equal(sc[c, x, r], cand[[c, Cc + c, 2 * Cc, 2 * Cc + 1], row])


def _assert_records_equal(b, Cc, out, S, off):
    new, old = _records(out[False]["rec"], b.total, Cc), _records(out[True]["rec"], b.total, Cc)
    # key and rho everywhere; the payload (rid, lam, sc) of every record of a present row -- an absent row's record is
    # (0, ~row), which the step never pools, and its payload is whatever the kernel's clamped or skipped loads left (the
    # sixteen-wave kernel loads the last row's candidate scores there, the four-wave kernel none: so before this change too)
    assert torch.equal(new["key"], old["key"]) and torch.equal(new["rho"], old["rho"])
    present = (new["key"].cpu().numpy().view(np.uint64) >> np.uint64(32)) > 0
    assert present.any()
    sel = torch.from_numpy(present).to(new["key"].device)
    for k in ("rid", "lam", "sc"):
        assert torch.equal(new[k][sel], old[k][sel]), k
    _assert_records_as_ranked_on_the_host(b, Cc, S, off, out[False]["fwd"], new)
    assert torch.equal(out[False]["loss"], out[True]["loss"]) and float(out[False]["loss"]) > 0
    for p, q in zip(out[False]["params"] + out[False]["moments"], out[True]["params"] + out[True]["moments"]):
        assert torch.equal(p, q)
    return new


@pytest.mark.parametrize("D", [256, 512])
@pytest.mark.parametrize("Cc", [2, 3])
@pytest.mark.parametrize("S", [1, 15, 16, 17, 33, 257])
def test_tile_records_equal_the_four_wave_forward(dev, S, Cc, D):
    b, n_sel, off, out = _train_step_records(dev, S, Cc, D, ties=False)
    _assert_rows_equal(out[False]["fwd"], out[True]["fwd"], n_sel[:1], off, "four waves, tile records")
    rec = _assert_records_equal(b, Cc, out, S, off)
    # the records of slide 0: per (class, tile) the four largest keys, descending; a short tile has 0 where a row is absent
    cap = (off[1] - off[0] + 15) // 16
    key = rec["key"][:Cc * cap * TILE_R].view(Cc, cap, TILE_R).cpu().numpy().view(np.uint64)
    tiles = (S + 15) // 16
    assert (key[:, :tiles, 0] >> np.uint64(32) > 0).all()                       # every tile with rows has a first record
    assert (key[:, :tiles, :-1] > key[:, :tiles, 1:]).all()                     # keys are unique and descend
    rows_last = S - 16 * (tiles - 1)                                            # rows of the last tile
    present = (key[:, tiles - 1] >> np.uint64(32)) > 0
    assert (present.sum(axis=1) == min(rows_last, TILE_R)).all()


def test_absent_rows_carry_zero_and_the_complement_of_their_row(dev):
    """S = 18: the second tile has two rows; its records of ranks 2 and 3 are the absent rows 18 and 19, (0, ~row), and
    rho is the fifth key's score word, 0."""
    S, Cc, D = 18, 2, 512
    b, n_sel, off, out = _train_step_records(dev, S, Cc, D, ties=False)
    rec = _assert_records_equal(b, Cc, out, S, off)
    cap = (off[1] - off[0] + 15) // 16
    key = rec["key"][:Cc * cap * TILE_R].view(Cc, cap, TILE_R).cpu().numpy().view(np.uint64)
    rho = rec["rho"][:Cc * cap].view(Cc, cap).cpu().numpy().view(np.uint32)
    for c in range(Cc):
        assert (key[c, 1, :2] >> np.uint64(32) > 0).all()
        assert [int(k) for k in key[c, 1, 2:]] == [0xFFFFFFFF - 18, 0xFFFFFFFF - 19]
        assert rho[c, 1] == 0 and rho[c, 0] > 0


def test_sixteen_equal_scores_in_a_tile_rank_by_row(dev):
    """Rows 16..31 are one row sixteen times (equal rows, equal candidate scores): sixteen equal mixed scores, so the
    score words alone do not rank the tile and the kernel ranks on the whole key -- records = rows 16, 17, 18, 19 in that
    order, rho = their common score word; rows 3 and 9 of tile 0 are equal too."""
    S, Cc, D = 33, 2, 512
    b, n_sel, off, out = _train_step_records(dev, S, Cc, D, ties=True)
    mixed = out[False]["fwd"]["mixed"]
    for c in range(Cc):
        assert len(torch.unique(mixed[c, 16:32])) == 1, "the case must have sixteen equal mixed scores in tile 1"
        assert float(mixed[c, 3]) == float(mixed[c, 9])
    _assert_rows_equal(out[False]["fwd"], out[True]["fwd"], n_sel[:1], off, "four waves, ties")
    rec = _assert_records_equal(b, Cc, out, S, off)
    cap = (off[1] - off[0] + 15) // 16
    key = rec["key"][:Cc * cap * TILE_R].view(Cc, cap, TILE_R).cpu().numpy().view(np.uint64)
    rid = rec["rid"][:Cc * cap * TILE_R].view(Cc, cap, TILE_R).cpu().numpy()
    rho = rec["rho"][:Cc * cap].view(Cc, cap).cpu().numpy().view(np.uint32)
    for c in range(Cc):
        assert [int(k & np.uint64(0xFFFFFFFF)) for k in key[c, 1]] == [0xFFFFFFFF - r for r in (16, 17, 18, 19)]
        assert rid[c, 1].tolist() == [16, 17, 18, 19]                           # (CompactBatch: sel_row is the identity)
        assert len({int(k >> np.uint64(32)) for k in key[c, 1]}) == 1 and int(key[c, 1, 0] >> np.uint64(32)) == int(rho[c, 1])


def test_three_training_passes_equal_with_and_without_tile_records(dev, monkeypatch):
    """main_moc.train, three passes: with the tile-record step (the forward leaves records, ranked by the new code) and
    without (engine.TILE_RECORDS off, what MOC_TILE_RECORDS=0 sets: no record arrays, the step ranks every mixed score)
    -- parameters, moments and per-step losses equal."""
    import helpers as H
    from moc_amd import engine as E, main_moc as M, synth
    Cc, D, j, K = 2, 512, 400, 10
    sizes = [2100, 1500, 1800, 2500, 1700, 2300]
    W, We = synth.make_bank(4242, D, Cc)
    bags, labels = synth.make_slide_set(4243, sizes, D, We, Cc)
    M.set_classifier_bank(W.to(dev), We.to(dev))
    args = H.make_args(Cc, j, K)
    out = {}
    for tiles in (True, False):
        monkeypatch.setattr(E, "TILE_RECORDS", tiles)
        res = M.ResidentBags(bags, labels, dev)
        torch.manual_seed(4)
        model = M.senet(D, 4).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
        losses = []
        for epoch in range(3):
            torch.manual_seed(300 + epoch)
            M.train(model, res, opt, dev, args)
            batch = M.train.last[0]
            assert (batch.meta_ws()[0]["tile_ws"] is not None) == tiles
            losses.append(batch.meta_ws()[0]["loss"].clone())
        torch.cuda.synchronize()
        out[tiles] = (losses, [p.detach().clone() for p in model.parameters()],
                      [opt.state[p][k].clone() for p in model.parameters() for k in ("exp_avg", "exp_avg_sq")])
    for a, c in zip(out[True][0], out[False][0]):
        assert torch.equal(a, c) and bool((a > 0).all())
    for a, c in zip(out[True][1] + out[True][2], out[False][1] + out[False][2]):
        assert torch.equal(a, c)
