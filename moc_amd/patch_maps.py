"""Patch maps: for every patch of every slide of a split, the meta-learner's gates and meta score, the zero-shot logits,
union membership and the patches behind the prediction -- what a pathology user looks at after training a slide
classifier (which patches drive the prediction), and what the reference's authors collect by hand for the zero-shot
path (utils/conch_zs_topk_visual.py: topj_pooling_return_idx, run_mizero_simple_4visual).

One pass per split, in the evaluation's visit order (repeat_num restored, as evaluation() does):
  * the evaluation path unchanged -- phase A (unmasked), moc_meta_forward over the union rows, moc_pool_loss -- so
    `pooled` is evaluation()'s logits bit for bit and `evidence` the rows that pooling averaged;
  * then moc_meta_forward_dense: the same forward over EVERY row (contiguous, no gather) into buffers of its own;
  * the zero-shot top-K rows per class by logit over all rows (moc_topk_mean);
  * one copy of each array to the host per chunk.

write_patch_maps stores one `<slide_id>.npz` per slide plus `index.json`; load_patch_map reads one back.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, fields

import numpy as np
import torch
import torch.nn.functional as F

from . import engine
from . import main_moc as M


@dataclass
class PatchMap:
    """One slide's map; host numpy arrays, N = patches of the slide, k = min(topk, N) (evidence: min(topk, S))."""
    path: str
    label: int
    pred: int
    pooled: np.ndarray                   # [C] float32: the slide's pooled logits (evaluation(); zero-shot top-K mean if no model)
    coords: np.ndarray                   # [N, 2] int64, from the bag
    logits: np.ndarray                   # [N, C] float32 zero-shot scores feat @ W
    selected: np.ndarray                 # [N] bool: member of the four selectors' union
    zs_evidence: np.ndarray              # [C, k] int64: top-K rows by zero-shot logit (ranked, ties: lower row first)
    gates: np.ndarray | None = None      # [N, 4] float32: lambda of every patch
    mixed: np.ndarray | None = None      # [N, C] float32: the meta score (evaluation mix, main_moc.py:482-492)
    evidence: np.ndarray | None = None   # [C, k] int64: the bag rows the pooled logit averages (ranked by value)


def patch_maps(model, loader, device, args) -> list[PatchMap]:
    """The patch maps of one unmasked pass over `loader` (a ResidentBags split or a loader of
    (features, label, coords, path) items).  model=None: zero-shot maps only (logits, zs_evidence; `pooled` is then the
    zero-shot top-K mean of the logits and `pred` its argmax)."""
    if model is not None and model.training:
        model.eval()
    K = int(args.topk)
    out = []
    with M._every_slide_once(loader):
        M._loader_seed_draw(loader)
        extras = []
        bank, batches = M._eval_batches(loader, device, args, "eval", extras=extras)
        C_ = bank.C
        meta = engine.MetaState(model) if model is not None else None
        use_bits = engine.eval_use_bits(args.discard_classifiers)
        v = 0
        for batch, lab, lab_list in batches:
            n, T = batch.n_slides, batch.total
            tensors, _ = batch.meta_ws()
            batch.phase_a(bank, for_eval=True)
            logits_d = batch.stats[:C_]
            zs_pooled, zs_idx, zs_cnt = engine.topk_mean(logits_d, logits_d, K, want_idx=True, seg_off=batch.row_off)
            host = {"logits": logits_d, "sel_flag": batch.sel_flag, "zs_idx": zs_idx, "zs_cnt": zs_cnt}
            if meta is not None:
                engine.meta_forward(batch, meta, 0, n, use_bits, keep_hidden=False)
                engine.pool_loss(batch, lab, 0, n)
                gates = torch.empty((T, 4), dtype=torch.float32, device=batch.device)
                mixed = torch.empty((C_, T), dtype=torch.float32, device=batch.device)
                engine.meta_forward_dense(batch, meta, 0, n, use_bits, gates, mixed)
                host.update(gates=gates, mixed=mixed, pooled=tensors["pooled"], pred=tensors["pred"],
                            sel_idx=batch.sel_idx, topk_idx=tensors["topk_idx"], topk_cnt=tensors["topk_cnt"])
            else:
                host.update(pooled=zs_pooled, pred=zs_pooled.argmax(dim=1))
            h = {k: t.cpu().numpy() for k, t in host.items()}     # one copy of each array per chunk
            for b in range(n):
                o, N = batch.row_off_host[b], batch.sizes[b]
                coords, path = extras[v]
                v += 1
                kz = int(h["zs_cnt"][b, 0])
                pm = PatchMap(
                    path=path, label=int(lab_list[b]), pred=int(h["pred"][b]), pooled=h["pooled"][b].copy(),
                    coords=np.asarray(coords, dtype=np.int64).reshape(N, 2).copy(),
                    logits=np.ascontiguousarray(h["logits"][:, o:o + N].T),
                    selected=h["sel_flag"][o:o + N].astype(bool),
                    zs_evidence=h["zs_idx"][b, :, :kz].astype(np.int64))
                if meta is not None:
                    kk = int(h["topk_cnt"][b, 0])
                    pm.gates = h["gates"][o:o + N].copy()
                    pm.mixed = np.ascontiguousarray(h["mixed"][:, o:o + N].T)
                    pm.evidence = h["sel_idx"][o + h["topk_idx"][b, :, :kk]].astype(np.int64)
                out.append(pm)
    return out


def probabilities(pooled: np.ndarray) -> np.ndarray:
    """softmax(56.3477 * pooled): the evaluation's class probabilities (main_moc.py:505)."""
    t = torch.from_numpy(np.asarray(pooled, dtype=np.float32)).reshape(1, -1)
    return F.softmax(t * M.CONCH_TEMPERATURE, dim=1)[0].numpy()


def slide_id_of(path: str) -> str:
    return os.path.splitext(os.path.basename(str(path)))[0]


def write_patch_maps(maps, out_dir, slide_ids=None):
    """One `<slide_id>.npz` per map (its fields, plus evidence_coords [C, k, 2] = coords of the evidence rows) and
    `index.json`: slide id -> label, pred, probabilities, file.  slide_ids default to the bag file names."""
    return _write_maps(maps, PatchMap, out_dir, slide_ids, lambda m: probabilities(m.pooled))


def load_patch_map(path) -> PatchMap:
    """A PatchMap back from a `<slide_id>.npz` of write_patch_maps (fields absent from the file: None)."""
    return _load_map(path, PatchMap)


@dataclass
class EnsembleMap:
    """One slide's map of an ensemble of R meta-learners (moc_amd.predict --patch_maps); host numpy arrays, N = patches of
    the slide, k = min(topk, N) (evidence: min(topk, S))."""
    path: str
    label: int                           # -1: unlabeled
    pred: int                            # argmax of `probabilities`
    probabilities: np.ndarray            # [C] float32: the ensemble's slide probabilities (predictions.csv's row)
    pooled: np.ndarray                   # [R, C] float32: each model's pooled logits
    coords: np.ndarray                   # [N, 2] int64
    logits: np.ndarray                   # [N, C] float32 zero-shot scores
    selected: np.ndarray                 # [N] bool: union membership
    zs_evidence: np.ndarray              # [C, k] int64: top-K rows by zero-shot logit
    prob_mean: np.ndarray                # [N, C] float32: mean over models of softmax(56.3477 * meta score)
    prob_std: np.ndarray                 # [N, C] float32: their population std -- where the models disagree
    gates_mean: np.ndarray               # [N, 4] float32: mean gates
    evidence: np.ndarray                 # [R, C, k] int64: bag rows of each model's pooled top-K (ranked as in PatchMap)


def write_ensemble_maps(maps, out_dir, slide_ids=None):
    """write_patch_maps for EnsembleMaps: `<slide_id>.npz` (fields, evidence_coords [R, C, k, 2], zs_evidence_coords) and
    index.json with the ensemble's probabilities."""
    return _write_maps(maps, EnsembleMap, out_dir, slide_ids, lambda m: m.probabilities)


def load_ensemble_map(path) -> EnsembleMap:
    return _load_map(path, EnsembleMap)


def _write_maps(maps, cls, out_dir, slide_ids, probs_of):
    os.makedirs(out_dir, exist_ok=True)
    slide_ids = [slide_id_of(m.path) for m in maps] if slide_ids is None else list(slide_ids)
    assert len(slide_ids) == len(maps) and len(set(slide_ids)) == len(slide_ids), "one distinct slide id per map"
    index = {}
    for sid, m in zip(slide_ids, maps):
        arrays = {}
        for f in fields(cls):
            val = getattr(m, f.name)
            if val is None:
                continue
            arrays[f.name] = np.asarray(val)
        if m.evidence is not None:
            arrays["evidence_coords"] = m.coords[m.evidence]
        arrays["zs_evidence_coords"] = m.coords[m.zs_evidence]
        fname = f"{sid}.npz"
        np.savez(os.path.join(out_dir, fname), **arrays)
        index[sid] = {"label": int(m.label), "pred": int(m.pred),
                      "probabilities": [float(p) for p in probs_of(m)], "file": fname}
    with open(os.path.join(out_dir, "index.json"), "w") as f:
        json.dump(index, f, indent=2)
    return index


def _load_map(path, cls):
    with np.load(path, allow_pickle=False) as z:
        kw = {}
        for f in fields(cls):
            if f.name not in z.files:
                continue
            a = z[f.name]
            if f.name == "path":
                a = str(a)
            elif f.name in ("label", "pred"):
                a = int(a)
            kw[f.name] = a
    return cls(**kw)
