"""The evaluation family held to a record (test-side only): the splits, the calls and the way a call's outcome is written
down, shared by tests/golden/make_eval_family.py (which writes tests/golden/eval_family.json) and
tests/test_gpu_eval_family.py (which compares with it).

Per call the outcome is: the result (Python floats as float.hex(), arrays as SHA-256 of their bytes; an exception as its
type and text), the split's `repeat_num` afterwards, and the library entries called, in order, run-length compressed."""
from __future__ import annotations

import dataclasses
import hashlib
import json
import os
import types

import numpy as np
import torch

import helpers as H
from moc_amd import engine, synth
from moc_amd import main_moc as M
from moc_amd import patch_selection_classifier as P

RECORD = os.path.join(H.GOLDEN_DIR, "eval_family.json")
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
D = 512
# name -> (classes, storage, slides, five banks).  Thirty classes take thirty slides: the multi-class AUC needs every class
# among the slides (sklearn refuses otherwise, as in the reference), so six slides would record refusals only.
SPLITS = {"C2-fp32-D512": (2, "fp32", 6, True), "C3-bf16-D512": (3, "bf16", 6, True), "C30-bf16-D512": (30, "bf16", 30, False)}
TOPJS, TOPKS = (5, 40), (1, 10, 64)
DISCARDS = ((), ("delta_softmax",), ("topk", "bottomk"))
TOPJ, TOPK, DISCARD = 40, 10, ("delta_softmax",)
SITUATIONS = ("none", "more", "four", "list", "chunks")

# entries that size or build cached objects (a bank's image, a model arena): whether a call makes them depends on what
# ran before it in the process, not on the call
SETUP_ENTRIES = ("moc_prepare_bank", "moc_scores_banks_max", "moc_last_error", "moc_version")


class EntryLog:
    """Stands in for engine.lib: `log()()` is the library behind a proxy whose moc_* entries append their name to
    `log.names` before forwarding."""

    def __init__(self, real_lib):
        self._real, self.names = real_lib, []

    def __call__(self):
        return self

    def __getattr__(self, name):
        fn = getattr(self._real(), name)
        if not name.startswith("moc_") or name.endswith("_bytes") or name in SETUP_ENTRIES:
            return fn

        def forward(*a):
            self.names.append(name)
            return fn(*a)
        return forward

    def take(self):
        """The names since the last take, run-length compressed: [[name, count], ...]."""
        out = []
        for n in self.names:
            if out and out[-1][0] == n:
                out[-1][1] += 1
            else:
                out.append([n, 1])
        self.names = []
        return out


def _unit_columns(n, g):
    w = torch.randn((D, n), generator=g)
    return (w / w.norm(dim=0, keepdim=True)).contiguous()


def _five_banks(C):
    """Widths C+4, C+1, 16, C+2, C+4; bank 3's extended foreground is not its W (tests/test_gpu_banks.py::_split)."""
    W0, We0 = synth.make_bank(60 + C, D, C)
    g = torch.Generator().manual_seed(600 + C)
    banks = [(W0, We0)]
    for b, ce in enumerate([C + 1, 16, C + 2, C + 4], start=1):
        fg = We0[:, :C] + 0.05 * b * _unit_columns(C, g)
        fg = fg / fg.norm(dim=0, keepdim=True)
        bg = _unit_columns(ce - C, g)
        n_old = min(4, ce - C)
        bg[:, :n_old] = We0[:, C:C + n_old]
        We = torch.cat([fg, bg], 1).contiguous()
        W = fg.clone().contiguous()
        if b == 3:
            e = fg + 0.1 * _unit_columns(C, g)
            We[:, :C] = e / e.norm(dim=0, keepdim=True)
        banks.append((W, We))
    return banks


_built = {}


def split(name, dev):
    """The split's banks, bags, models and resident splits: built once per process."""
    if name not in _built:
        C, st, n, five = SPLITS[name]
        banks = _five_banks(C) if five else [synth.make_bank(40 + C, D, C)]
        sizes = [int(v) for v in np.random.default_rng(C * 77).integers(200, 701, size=n)]
        sizes[0], sizes[1] = 200, 700
        bags, labels = synth.make_slide_set(7000 + C, sizes, D, banks[0][1], C, confusion=0.3)
        models = []
        for m in range(len(banks) if five else 2):
            torch.manual_seed(23 + C + m)
            model = M.senet(D, 4).to(dev)
            with torch.no_grad():                        # gates away from 0 / 1: every term of the mix matters
                model.model[2].weight.mul_(3.0)
            models.append(model)
        mk = lambda b, l: M.ResidentBags(b, l, dev, dtype=DT[st])
        _built[name] = types.SimpleNamespace(
            name=name, C=C, dev=dev, dtype=DT[st], banks=[(W.to(dev), We.to(dev)) for W, We in banks], bags=bags, labels=labels,
            models=models, res=mk(bags, labels),
            # evaluation_runs packs its splits side by side: it gets two of its own (the second in reverse slide order)
            runs=(mk(bags, labels), mk(bags[::-1], labels[::-1])),
            bytes=sum(sizes) * D * (4 if st == "fp32" else 2))
    return _built[name]


def _custom(logits_ext, topj, **kw):
    """A plain callable: zs_evaluation's path for anything that is not one of the four fused functions."""
    return P.bottomk_irrel_classifier_pooling(logits_ext, topj, **kw)


def forms(S):
    """[(name, takes a plain loader, datasets whose repeat_num is set and read, call(loader))] in a fixed order."""
    dev, C = S.dev, S.C
    args = lambda **kw: types.SimpleNamespace(**{**vars(H.make_args(C, TOPJ, TOPK, DISCARD)), **kw})
    sds = [m.state_dict() for m in S.models[:2]]
    out = [("evaluation", True, lambda ld: M.evaluation(S.models[0], ld, dev, args()))]
    for f in M.ZS_POOLING_FUNCS:
        out.append((f"zs_evaluation/{f.__name__}", True, lambda ld, f=f: M.zs_evaluation(ld, dev, args(), pooling_func=f)))
    out.append(("zs_evaluation/custom", True, lambda ld: M.zs_evaluation(ld, dev, args(), pooling_func=_custom)))
    for mode in ("avg", "sum", "max"):
        out.append((f"ablation_evaluation/{mode}", True, lambda ld, mode=mode: M.ablation_evaluation(ld, dev, args(ablation_study=mode))))
    out.append(("evaluation_sweep", False, lambda ld: M.evaluation_sweep(S.models[0], ld, dev, args(), TOPJS, TOPKS, DISCARDS)))
    out.append(("zs_evaluation_sweep", False, lambda ld: M.zs_evaluation_sweep(ld, dev, args(), TOPKS)))
    if len(S.banks) > 1:
        def own_ext(ld):                 # bottomk's image is not the others': one pass per distinct image
            M.set_classifier_bank(*S.banks[3])
            try:
                return M.zs_evaluation_sweep(ld, dev, args(), TOPKS)
            finally:
                M.set_classifier_bank(*S.banks[0])
        out.append(("zs_evaluation_sweep/own_ext", False, own_ext))
        for f in (P.topj_pooling, P.bottomk_irrel_classifier_pooling):
            out.append((f"zs_evaluation_banks/{f.__name__}", False,
                        lambda ld, f=f: M.zs_evaluation_banks(ld, dev, args(), S.banks, pooling_func=f)))
        out.append(("zs_evaluation_sweep_banks", False, lambda ld: M.zs_evaluation_sweep_banks(ld, dev, args(), S.banks, TOPKS)))
        for tag, ms in (("one_model", S.models[0]), ("model_per_bank", S.models)):
            out.append((f"evaluation_banks/{tag}", False, lambda ld, ms=ms: M.evaluation_banks(ms, ld, dev, args(), S.banks)))
            out.append((f"evaluation_sweep_banks/{tag}", False,
                        lambda ld, ms=ms: M.evaluation_sweep_banks(ms, ld, dev, args(), S.banks, TOPJS, TOPKS, DISCARDS)))
    out.append(("predict/maps", True, lambda ld: _predict(sds, ld, dev, args(), True)))
    out.append(("predict/no_maps", True, lambda ld: _predict(sds, ld, dev, args(), False)))
    out.append(("patch_maps/model", True, lambda ld: _patch_maps(S.models[0], ld, dev, args())))
    out.append(("patch_maps/zero_shot", True, lambda ld: _patch_maps(None, ld, dev, args())))
    return out


def _predict(sds, ld, dev, args, maps):
    from moc_amd import predict
    return predict.predict(sds, ld, dev, args, maps=maps)


def _patch_maps(model, ld, dev, args):
    from moc_amd import patch_maps
    return patch_maps.patch_maps(model, ld, dev, args)


def _runs(S):
    """Two models over three loaders, the first model and the first split named twice."""
    a, b = S.runs
    res = M.evaluation_runs([S.models[0], S.models[1], S.models[0]], [a, b, a], S.dev, H.make_args(S.C, TOPJ, TOPK, DISCARD))
    return {"result": res, "last_pooled": list(M.evaluation_runs.last_pooled)}


def cells(S):
    """[(id, situation, datasets, thunk)]: every form in every situation it admits."""
    out = []
    for name, plain, call in forms(S):
        for sit in SITUATIONS:
            if sit == "list":
                if plain:
                    ld = H.ListLoader(S.bags, S.labels)
                    out.append((f"{name}@list", sit, [ld.dataset], lambda call=call, ld=ld: call(ld)))
            else:
                out.append((f"{name}@{sit}", sit, [S.res], lambda call=call: call(S.res)))
    for sit in SITUATIONS:
        if sit != "list":
            out.append((f"evaluation_runs@{sit}", sit, list(S.runs), lambda: _runs(S)))
    return out


def run_cell(S, log, sit, datasets, thunk, monkeypatch_setattr):
    """One call in its situation -> the outcome (module docstring).  `monkeypatch_setattr(obj, name, value)` returns a
    function that undoes it."""
    for ds in datasets:
        ds.repeat_num = {"more": ds.real_len() + 3, "four": 4}.get(sit)
    undo = None
    if sit == "chunks":
        undo = monkeypatch_setattr(M, "MAX_BATCH_BYTES", S.bytes // 4)
        item = 4 if S.dtype == torch.float32 else 2
        assert len(M._chunks(S.res.sizes, D, item)) >= 3
        assert len(S.banks) == 1 or len(M._chunks_banks(S.res.sizes, D, item, len(S.banks), S.C)) >= 3
    log.take()
    try:
        try:
            result = pack(thunk())
        except Exception as e:                       # (sklearn refusing a split without every class, as in the reference)
            result = {"raises": type(e).__name__, "text": str(e)}
    finally:
        if undo is not None:
            undo()
    return {"result": result, "repeat_num": [ds.repeat_num for ds in datasets], "entries": log.take()}


def setattr_undo(obj, name, value):
    old = getattr(obj, name)
    setattr(obj, name, value)
    return lambda: setattr(obj, name, old)


# ---- a result as JSON ----------------------------------------------------------------------------------------------------
def _sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is None:
            h.update(b"none")
            continue
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype}{a.shape}".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def _maps(maps):
    """A list of PatchMap / EnsembleMap -> field by field: plain values as a list, arrays as one digest over the slides."""
    out = {"n": len(maps)}
    for f in dataclasses.fields(maps[0]) if maps else ():
        vals = [getattr(m, f.name) for m in maps]
        if all(v is None or isinstance(v, np.ndarray) for v in vals):
            out[f.name] = _sha(vals)
        else:
            out[f.name] = pack(vals)
    return out


def pack(x):
    if isinstance(x, float):
        return x.hex()
    if x is None or isinstance(x, (bool, int, str)):
        return x
    if isinstance(x, (np.floating, np.integer)):
        return pack(x.item())
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    if isinstance(x, np.ndarray):
        return {"sha256": _sha([x])}
    if isinstance(x, dict):
        if list(x) == ["loss", "acc", "auc"]:            # (the order is part of the value)
            return ["metrics"] + [pack(v) for v in x.values()]
        return {"keys": [pack(k) for k in x], "vals": [pack(v) for v in x.values()]}
    if isinstance(x, (list, tuple)):
        if x and dataclasses.is_dataclass(x[0]):
            return _maps(list(x))
        return [pack(v) for v in x]
    if dataclasses.is_dataclass(x):                      # predict.Predictions
        return {f.name: pack(getattr(x, f.name)) for f in dataclasses.fields(x)}
    raise TypeError(f"eval family record: no rule for {type(x)}")


# ---- the record file: every repeated string, list or dict once -----------------------------------------------------------
def shrink(record):
    """The record with every string, list and dict of 8 characters or more (as JSON) kept once in "nodes" and named "~i"
    where it occurs: the calls share most of their floats, digests and entry sequences.  Nothing is lost: expand()."""
    nodes = {}

    def ref(x):
        if isinstance(x, str):
            assert not x.startswith("~")
        elif isinstance(x, list):
            x = [ref(v) for v in x]
        elif isinstance(x, dict):
            x = {k: ref(v) for k, v in x.items()}
        else:
            return x
        s = json.dumps(x, separators=(",", ":"))
        return x if len(s) < 8 else "~%d" % nodes.setdefault(s, len(nodes))
    cells = {name: {cid: ref(v) for cid, v in c.items()} for name, c in record.items()}
    return {"nodes": [json.loads(s) for s in nodes], "cells": cells}


def expand(doc):
    def val(x):
        if isinstance(x, str) and x.startswith("~"):
            return val(doc["nodes"][int(x[1:])])
        if isinstance(x, list):
            return [val(v) for v in x]
        if isinstance(x, dict):
            return {k: val(v) for k, v in x.items()}
        return x
    return val(doc["cells"])


def save_record(record, path=RECORD):
    doc = shrink(record)
    assert expand(doc) == record
    lines, cur = [], ""
    for s in (json.dumps(n, separators=(",", ":")) for n in doc["nodes"]):      # (a few hundred characters a line)
        if cur and len(cur) + len(s) > 400:
            lines.append(cur)
            cur = ""
        cur += ("," if cur else "") + s
    lines.append(cur)
    with open(path, "w") as f:
        f.write('{"nodes":[\n' + ",\n".join(lines) + '\n],\n"cells":' + json.dumps(doc["cells"], separators=(",", ":")) + "}\n")


def load_record(path=RECORD):
    with open(path) as f:
        return expand(json.load(f))
