"""The selected-row counts by pinned mailbox (moc_batch_t.n_sel_mail / n_sel_ticket): compact_kernel stores slide b's
(ticket << 32) | S into a pinned word, moc_train_steps reads that word in front of step b's two launches and hands the
count to both by value.  Whatever share of a pass's steps knows its S -- all, none, some -- the losses, pooled logits,
pooled rows, parameters and both Adam moments are BIT-identical to the same passes with engine.N_SEL_HOST off, and
moc_n_sel_stats says how many steps knew."""
import ctypes

import numpy as np
import pytest
import torch

import helpers as H
from moc_amd import synth

pytestmark = pytest.mark.gpu

SHAPES = {
    "tiny": (2, 512, torch.float32, [40, 18, 9, 300], 400, 10),        # slides of a tile or two, S < K, S = 0 possible
    "vq": (2, 512, torch.float32, [3000, 2500, 4100], 400, 10),        # eight against twelve record keys per lane
    "bf16": (3, 256, torch.bfloat16, [900, 700, 1100], 100, 5),
}
PASSES = 4
_reference = {}


def _stats(reset=True):
    from moc_amd import _lib
    known, steps = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert _lib.lib().moc_n_sel_stats(ctypes.byref(known), ctypes.byref(steps), int(reset)) == 0
    return known.value, steps.value


def _passes(dev, shape, passes=PASSES, n_sel_host=True, graph=False):
    """`passes` passes of main_moc.train over a resident split -> (everything a step leaves behind as host arrays,
    (known steps, issued steps) of moc_train_steps over them)."""
    from moc_amd import engine as E, main_moc as M
    C, D, dtype, sizes, j, K = SHAPES[shape]
    keep = (E.N_SEL_HOST, E.STEP_GRAPH)
    E.N_SEL_HOST, E.STEP_GRAPH = n_sel_host, graph
    try:
        W, We = synth.make_bank(77 + C, D, C)
        bags, labels = synth.make_slide_set(177 + C, sizes, D, We, C)
        M.set_classifier_bank(W.to(dev), We.to(dev))
        torch.manual_seed(7 + C)
        model = M.senet(D, 4).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
        res = M.ResidentBags([b.to(dtype) for b in bags], labels, dev)
        args = H.make_args(C, j, K)
        torch.manual_seed(17 + C)
        out = {"loss": [], "pooled": [], "topk": []}
        _stats()
        for _ in range(passes):
            M.train(model, res, opt, dev, args)
            torch.cuda.synchronize()
            t = M.train.last[0].meta_ws()[0]
            out["loss"].append(t["loss"].cpu().numpy().copy())
            out["pooled"].append(t["pooled"].cpu().numpy().copy())
            out["topk"].append(t["topk_idx"].cpu().numpy().copy())
        out["params"] = H.flat_params(model)
        out["m"], out["v"] = H.flat_state(opt, "exp_avg"), H.flat_state(opt, "exp_avg_sq")
        return out, _stats()
    finally:
        E.N_SEL_HOST, E.STEP_GRAPH = keep


def _same_as_reference(dev, shape, got, passes=PASSES):
    """Against the same passes with no mailbox and no host copy at all (computed once per shape, left unchanged)."""
    if shape not in _reference:
        _reference[shape], (known, _) = _passes(dev, shape, n_sel_host=False)
        assert known == 0
    ref = _reference[shape]
    for e in range(passes):
        np.testing.assert_array_equal(got["loss"][e], ref["loss"][e])
        np.testing.assert_array_equal(got["pooled"][e], ref["pooled"][e])
        np.testing.assert_array_equal(got["topk"][e], ref["topk"][e])
    if passes == PASSES:
        for k in ("params", "m", "v"):
            np.testing.assert_array_equal(got[k], ref[k])


def _wrap_publish(monkeypatch, before):
    """SlideBatch.publish_n_sel -- what engine.train_steps calls in front of a pass's steps -- with `before(batch)` run
    first, behind a device synchronisation: phase A has run, every word it stores has arrived."""
    from moc_amd import engine as E
    orig = E.SlideBatch.publish_n_sel
    handed = []

    def publish(self, allow=True):
        torch.cuda.synchronize()
        allow = before(self, allow)
        handed.append(orig(self, allow))
        return handed[-1]

    monkeypatch.setattr(E.SlideBatch, "publish_n_sel", publish)
    return handed


@pytest.mark.parametrize("shape", list(SHAPES))
def test_arrived_words_serve_every_step(gpu_device, monkeypatch, shape):
    n = len(SHAPES[shape][3])
    handed = _wrap_publish(monkeypatch, lambda batch, allow: allow)
    got, (known, steps) = _passes(gpu_device, shape)
    assert all(handed) and len(handed) == PASSES
    assert (known, steps) == (PASSES * n, PASSES * n)
    _same_as_reference(gpu_device, shape, got)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_words_of_an_earlier_ticket_serve_no_step(gpu_device, monkeypatch, shape):
    n = len(SHAPES[shape][3])

    def fresh_ticket(batch, allow):
        batch._n_sel_stale()          # a fresh ticket and no phase A under it: every word carries the previous one
        return allow

    handed = _wrap_publish(monkeypatch, fresh_ticket)
    got, (known, steps) = _passes(gpu_device, shape)
    assert all(handed)
    assert (known, steps) == (0, PASSES * n)
    _same_as_reference(gpu_device, shape, got)


@pytest.mark.parametrize("shape,some", [("tiny", (0, 3)), ("tiny", (1, 2)), ("vq", (1,)), ("vq", (0, 2)), ("bf16", (2,))])
def test_a_pass_of_known_and_unknown_slides(gpu_device, monkeypatch, shape, some):
    """The C ABI on its own: under a fresh ticket the test itself writes the words of the slides `some`, with the counts
    phase A left in n_sel.  Exactly those steps know their S -- forward and step kernel of a slide alike -- beside steps
    that load it."""
    n = len(SHAPES[shape][3])

    def only_some(batch, allow):
        batch._n_sel_stale()
        counts = batch.n_sel.cpu().tolist()
        for b in some:
            word = (batch._n_sel_ticket << 32) | counts[b]
            batch._n_sel_mail[b] = word - (1 << 64) if word >> 63 else word     # (the pinned tensor is int64)
        return allow

    _wrap_publish(monkeypatch, only_some)
    got, (known, steps) = _passes(gpu_device, shape)
    assert (known, steps) == (PASSES * len(some), PASSES * n)
    _same_as_reference(gpu_device, shape, got)


def test_ticket_wraps_past_zero(gpu_device, monkeypatch):
    """The ticket counter set just below 2^32: every batch's next phase A's take 0xFFFFFFFF and then 1 -- never 0, which
    says "no ticket" -- and the words keep serving every step."""
    from moc_amd import engine as E
    shape, tickets = "vq", []
    n = len(SHAPES[shape][3])
    init = E.SlideBatch.__init__

    def init_high(self, *a, **kw):
        init(self, *a, **kw)
        if self._n_sel_mail is not None:
            self._n_sel_ticket = 0xFFFFFFFE

    monkeypatch.setattr(E.SlideBatch, "__init__", init_high)
    _wrap_publish(monkeypatch, lambda batch, allow: tickets.append(batch._n_sel_ticket) or allow)
    got, (known, steps) = _passes(gpu_device, shape)          # two sets of arrays alternate: two phase A's each
    assert len(tickets) == PASSES and 0 not in tickets, tickets
    assert max(tickets) == 0xFFFFFFFF and min(tickets) < 16, tickets      # before the wrap and behind it
    assert (known, steps) == (PASSES * n, PASSES * n)
    _same_as_reference(gpu_device, shape, got)


def test_captured_pass_ignores_the_mailbox(gpu_device, monkeypatch):
    """MOC_STEP_GRAPH=1: a pass that IS handed the mailbox (engine.train_steps never does) runs no step on a host count --
    a captured pass serves other passes, with other counts."""
    shape = "vq"
    handed = _wrap_publish(monkeypatch, lambda batch, allow: True)
    got, (known, _) = _passes(gpu_device, shape, graph=True)
    assert all(handed) and len(handed) == PASSES
    assert known == 0
    _same_as_reference(gpu_device, shape, got)
