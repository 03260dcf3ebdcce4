"""Per-slide class probabilities from one or several trained meta-learners -- what a user expects after training the five
folds of a shot: apply them to new slides and average the folds' probabilities (the usual k-fold few-shot ensemble).

One unmasked pass in the evaluation's visit order (repeat_num restored, as evaluation() does):
  * phase A once (score pass, the four selectors, union, candidate scores): it does not depend on the parameters;
  * moc_meta_forward_models: the evaluation forward of all R meta-learners in one launch, each model's mixed scores bit for
    bit those of moc_meta_forward with that model alone;
  * moc_pool_loss once per model over its own slab -> per-model pooled logits, so that with R = 1 this is evaluation().

The ensemble probability of a slide is the mean over models of softmax(CONCH_TEMPERATURE * pooled) -- the evaluation's
probabilities (main_moc.py:505, patch_maps.probabilities).

    python -m moc_amd.predict --ckpt f0.pt f1.pt f2.pt f3.pt f4.pt --slides list.csv --data_dir bags/ --out preds/
    python -m moc_amd.predict --ckpt best.pt --dataset nsclc --shot 16 --fold 0 --split test --root /data/MOC --out preds/
    python -m moc_amd.predict --ckpt best.pt --synthetic 24 --shot 4 --fold 0 --split test --out preds/

--slides: a CSV with a `slide_id` column and an optional `label` column; bags are read with datasets.read_bag from
--data_dir (h5_files/, pt_files/ or npy_files/).  The zero-shot bank is the --dataset's, from --root as run_moc loads it.
Writes DIR/predictions.csv (one row per slide) and DIR/predictions.json (arguments, checkpoints, and with labels the
per-model and ensemble loss / acc / AUC).

--patch_maps adds DIR/patch_maps/<slide_id>.npz and index.json (patch_maps.EnsembleMap) from the same pass: after the pooling,
moc_meta_forward_dense_models gives every patch the mean and population std over the models of softmax(56.3477 * meta
score) and the mean gates, the per-model slabs never leaving the device; the zero-shot half is patch_maps' (moc_topk_mean).
"""
from __future__ import annotations

import argparse
import json
import os
from dataclasses import dataclass

import numpy as np
import pandas as pd
import torch

MAX_MODELS = 16
SPLITS = ("train", "val", "test")


@dataclass
class Predictions:
    """R models, N slides, C classes; host arrays."""
    slide_ids: list
    paths: list
    classes: list                        # C class names
    pooled: np.ndarray                   # [R, N, C] float32: per-model pooled logits (evaluation()'s)
    probs: np.ndarray                    # [R, N, C] float32: softmax(CONCH_TEMPERATURE * pooled)
    ensemble: np.ndarray                 # [N, C] float32: mean of probs over the models
    pred: np.ndarray                     # [N] int64: argmax of the ensemble
    labels: np.ndarray | None = None     # [N] int64 when known
    loss: np.ndarray | None = None       # [R, N] float32: per-model cross entropy (moc_pool_loss) when labels are known
    maps: list | None = None             # N patch_maps.EnsembleMap (predict(..., maps=True))


def _probs(pooled: np.ndarray) -> np.ndarray:
    from .main_moc import CONCH_TEMPERATURE
    t = torch.from_numpy(np.ascontiguousarray(pooled, dtype=np.float32))
    return torch.softmax(t * CONCH_TEMPERATURE, dim=-1).numpy()


def predict(state_dicts, loader, device, args, labeled: bool = True, slide_ids=None, maps: bool = False) -> Predictions:
    """Predictions of the R = len(state_dicts) meta-learners (senet(D, 4) state_dicts) over `loader` (a ResidentBags
    split or a loader of (features, label, coords, path) items), in one pass.  labeled=False: the loader's labels are
    placeholders (zeros) and are neither reported nor used.  maps=True: also the ensemble patch map of every slide
    (Predictions.maps), from the same pass."""
    from . import engine
    from . import main_moc as M
    from .patch_maps import EnsembleMap, slide_id_of
    R = len(state_dicts)
    assert 1 <= R <= MAX_MODELS, f"predict: 1 .. {MAX_MODELS} checkpoints"
    pooled, losses, labels = [], [], []
    parts = []                                             # maps: per slide, everything but the ensemble's probabilities
    with M._every_slide_once(loader):
        M._loader_seed_draw(loader)
        extras = []
        bank, batches = M._eval_batches(loader, device, args, "eval", extras=extras)
        arena = engine.ModelArena(state_dicts, device)
        use_bits = engine.eval_use_bits(args.discard_classifiers)
        if maps and bank.C > 64:
            raise SystemExit(f"--patch_maps: {bank.C} classes; the ensemble maps take at most 64")
        K = int(args.topk)
        v = 0
        for batch, lab, lab_list in batches:
            n = batch.n_slides
            batch.phase_a(bank, for_eval=True)
            mixed = torch.empty((R, batch.C, batch.total), dtype=torch.float32, device=batch.device)
            engine.meta_forward_models(batch, arena, R, mixed, 0, n, use_bits)
            lab_d = lab if labeled else torch.zeros_like(lab)
            out = engine.pool_models(batch, mixed, lab_d, 0, n)
            if maps:
                T = batch.total
                pm = torch.empty((batch.C, T), dtype=torch.float32, device=batch.device)
                ps = torch.empty((batch.C, T), dtype=torch.float32, device=batch.device)
                gm = torch.empty((T, 4), dtype=torch.float32, device=batch.device)
                engine.meta_forward_dense_models(batch, arena, R, M.CONCH_TEMPERATURE, pm, ps, gm, 0, n, use_bits)
                logits_d = batch.stats[:batch.C]
                _, zs_idx, zs_cnt = engine.topk_mean(logits_d, logits_d, K, want_idx=True, seg_off=batch.row_off)
                dev_arrays = {"logits": logits_d, "sel_flag": batch.sel_flag, "zs_idx": zs_idx, "zs_cnt": zs_cnt,
                              "prob_mean": pm, "prob_std": ps, "gates_mean": gm, "sel_idx": batch.sel_idx,
                              "topk_idx": out["topk_idx"], "topk_cnt": out["topk_cnt"], "pooled": out["pooled"]}
                h = {k: t.cpu().numpy() for k, t in dev_arrays.items()}     # one copy of each array per chunk
                for b in range(n):
                    o, N = batch.row_off_host[b], batch.sizes[b]
                    coords, path = extras[v]
                    v += 1
                    kz, kk = int(h["zs_cnt"][b, 0]), int(h["topk_cnt"][0, b, 0])
                    parts.append(dict(
                        path=path, label=int(lab_list[b]) if labeled else -1, pooled=h["pooled"][:, b].copy(),
                        coords=np.asarray(coords, dtype=np.int64).reshape(N, 2).copy(),
                        logits=np.ascontiguousarray(h["logits"][:, o:o + N].T),
                        selected=h["sel_flag"][o:o + N].astype(bool),
                        zs_evidence=h["zs_idx"][b, :, :kz].astype(np.int64),
                        prob_mean=np.ascontiguousarray(h["prob_mean"][:, o:o + N].T),
                        prob_std=np.ascontiguousarray(h["prob_std"][:, o:o + N].T),
                        gates_mean=h["gates_mean"][o:o + N].copy(),
                        evidence=h["sel_idx"][o + h["topk_idx"][:, b, :, :kk]].astype(np.int64)))
                pooled.append(h["pooled"])
                losses.append(out["loss"].cpu().numpy())
            else:
                pooled.append(out["pooled"].cpu().numpy())
                losses.append(out["loss"].cpu().numpy())
            labels.extend(lab_list)
    paths = [str(p) for _, p in extras]
    pooled = np.concatenate(pooled, axis=1)
    probs = _probs(pooled)
    ens = probs.mean(axis=0, dtype=np.float64).astype(np.float32)
    C = pooled.shape[2]
    names = list(getattr(args, "class_names", None) or [str(c) for c in range(C)])
    pred = ens.argmax(axis=1).astype(np.int64)
    emaps = [EnsembleMap(pred=int(pred[i]), probabilities=ens[i].copy(), **d) for i, d in enumerate(parts)] if maps else None
    return Predictions(slide_ids=list(slide_ids) if slide_ids is not None else [slide_id_of(p) for p in paths],
                       paths=paths, classes=names, pooled=pooled, probs=probs, ensemble=ens,
                       pred=pred, labels=np.asarray(labels, dtype=np.int64) if labeled else None,
                       loss=np.concatenate(losses, axis=1) if labeled else None, maps=emaps)


def metrics(p: Predictions, args, n_div=None) -> dict:
    """Per-model loss / acc / AUC exactly as evaluation() computes them (main_moc._metrics) and the ensemble's: acc of
    its argmax, AUC of its probabilities (main_moc._auc), loss = mean negative log of the true class's probability."""
    from . import main_moc as M
    assert p.labels is not None, "metrics need labels"
    N = len(p.labels)
    lbl = p.labels
    models = []
    for r in range(p.pooled.shape[0]):
        pr = torch.from_numpy(p.pooled[r])
        if p.loss is not None:
            loss = p.loss[r].tolist()
        else:
            loss = torch.nn.functional.cross_entropy(pr, torch.from_numpy(lbl), reduction="none").tolist()
        models.append(M._metrics(pr, lbl.tolist(), loss, n_div or N, N, args))
    ens = p.ensemble.astype(np.float64)
    score = ens[:, 1] if ens.shape[1] == 2 else ens
    ensemble = {"loss": float(np.mean(-np.log(np.maximum(ens[np.arange(N), lbl], 1e-300)))),
                "acc": float((p.pred == lbl).sum()) / N, "auc": float(M._auc(lbl, score))}
    return {"models": models, "ensemble": ensemble}


def write_predictions(p: Predictions, out_dir, info: dict | None = None, metrics_: dict | None = None):
    """DIR/predictions.csv: slide_id, path, pred, prob_<class> (ensemble), m<r>_prob_<class>, m<r>_logit_<class>, label
    (when known); DIR/predictions.json: `info` (arguments, checkpoints), classes, slide count, metrics (when given)."""
    os.makedirs(out_dir, exist_ok=True)
    R = p.pooled.shape[0]
    cols = {"slide_id": list(p.slide_ids), "path": list(p.paths), "pred": p.pred.astype(np.int64)}
    for c, name in enumerate(p.classes):
        cols[f"prob_{name}"] = p.ensemble[:, c]
    for r in range(R):
        for c, name in enumerate(p.classes):
            cols[f"m{r}_prob_{name}"] = p.probs[r, :, c]
        for c, name in enumerate(p.classes):
            cols[f"m{r}_logit_{name}"] = p.pooled[r, :, c]
    if p.labels is not None:
        cols["label"] = p.labels.astype(np.int64)
    pd.DataFrame(cols).to_csv(os.path.join(out_dir, "predictions.csv"), index=False, float_format="%.9g")
    doc = dict(info or {})
    doc.update(classes=list(p.classes), n_models=R, n_slides=len(p.slide_ids))
    if metrics_ is not None:
        doc["metrics"] = metrics_
    with open(os.path.join(out_dir, "predictions.json"), "w") as f:
        json.dump(doc, f, indent=2)
    return doc


def load_predictions(out_dir) -> Predictions:
    """A Predictions back from write_predictions' files (float32 values exactly: nine significant digits)."""
    with open(os.path.join(out_dir, "predictions.json")) as f:
        doc = json.load(f)
    df = pd.read_csv(os.path.join(out_dir, "predictions.csv"), dtype={"slide_id": str, "path": str})
    names, R = doc["classes"], doc["n_models"]
    f32 = lambda k: df[k].to_numpy(dtype=np.float32)
    return Predictions(slide_ids=df["slide_id"].tolist(), paths=df["path"].tolist(), classes=list(names),
                       pooled=np.stack([np.stack([f32(f"m{r}_logit_{n}") for n in names], 1) for r in range(R)]),
                       probs=np.stack([np.stack([f32(f"m{r}_prob_{n}") for n in names], 1) for r in range(R)]),
                       ensemble=np.stack([f32(f"prob_{n}") for n in names], 1),
                       pred=df["pred"].to_numpy(dtype=np.int64),
                       labels=df["label"].to_numpy(dtype=np.int64) if "label" in df.columns else None)


# ------------------------------------------------------------------ command line
def get_args(argv=None):
    p = argparse.ArgumentParser(description="Per-slide predictions of one or several MOC checkpoints (fold ensemble)")
    p.add_argument("--ckpt", nargs="+", required=True, help="saved senet state_dicts (best_model_*.pt), 1 .. 16")
    p.add_argument("--out", required=True, help="output directory (predictions.csv, predictions.json)")
    p.add_argument("--slides", default=None, help="CSV with a slide_id column and an optional label column")
    p.add_argument("--data_dir", default=None, help="--slides: directory holding h5_files/, pt_files/ or npy_files/")
    p.add_argument("--synthetic", type=int, default=0, help="the generated slides of run_moc --synthetic N")
    p.add_argument("--split", default=None, choices=SPLITS, help="dataset / synthetic modes: which split")
    p.add_argument("--dataset", default="nsclc", help="task: label map and zero-shot bank (run_moc --dataset)")
    p.add_argument("--shot", type=int, default=1)
    p.add_argument("--fold", type=int, default=0)
    p.add_argument("--root", default=".", help="directory holding dataset_csv/, splits/, data/, models/ (run_moc --root)")
    p.add_argument("--topj", type=int, default=10)
    p.add_argument("--topk", type=int, default=10)
    p.add_argument("--discard_classifiers", nargs="+", default=[])
    p.add_argument("--bag_dtype", default="fp32", choices=["fp32", "bf16", "fp16"])
    p.add_argument("--disable_tqdm", action="store_true")
    p.add_argument("--patch_maps", action="store_true",
                   help="also write OUT/patch_maps/<slide_id>.npz + index.json: the ensemble's per-patch probabilities "
                        "(mean, std over the models), mean gates and each model's evidence, from the same pass")
    a = p.parse_args(argv)
    a.pretrain = "conch"
    return a


def load_checkpoints(paths):
    """The state_dicts of `paths` on the CPU, refused unless every one is a senet(D, 4) with one D."""
    from .engine import HIDDEN
    if not 1 <= len(paths) <= MAX_MODELS:
        raise SystemExit(f"--ckpt: {len(paths)} checkpoints; one prediction pass takes 1 .. {MAX_MODELS}")
    sds, dims = [], set()
    for pth in paths:
        sd = torch.load(pth, map_location="cpu")
        ok = isinstance(sd, dict) and set(sd) == {"model.0.weight", "model.0.bias", "model.2.weight", "model.2.bias"}
        if ok:
            D = int(sd["model.0.weight"].shape[-1])
            ok = (tuple(sd["model.0.weight"].shape) == (HIDDEN, D) and tuple(sd["model.0.bias"].shape) == (HIDDEN,) and
                  tuple(sd["model.2.weight"].shape) == (4, HIDDEN) and tuple(sd["model.2.bias"].shape) == (4,))
        if not ok:
            raise SystemExit(f"--ckpt {pth}: not a senet(D, 4) state_dict (model.0.* [64, D], model.2.* [4, 64])")
        dims.add(D)
        sds.append(sd)
    if len(dims) != 1:
        raise SystemExit(f"--ckpt: the checkpoints disagree on the input width D: {sorted(dims)}")
    return sds


def check_args(a):
    """Refusals from the command line and the files alone, before any GPU work."""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("predict is a one-GPU tool: run it without a launcher")
    modes = [bool(a.slides), a.synthetic > 0]
    if sum(modes) > 1:
        raise SystemExit("give exactly one input: --slides CSV, --synthetic N, or --dataset/--shot/--fold/--split")
    if a.slides:
        if not a.data_dir:
            raise SystemExit("--slides needs --data_dir")
        if a.split:
            raise SystemExit("--split belongs to the dataset / synthetic modes, not to --slides")
        df = pd.read_csv(a.slides, dtype={"slide_id": str})
        if "slide_id" not in df.columns:
            raise SystemExit(f"{a.slides}: no slide_id column")
        dup = sorted(df["slide_id"][df["slide_id"].duplicated()].unique().tolist())
        if dup:
            raise SystemExit(f"{a.slides}: slide ids named more than once: {dup[:8]}")
    elif not a.split:
        raise SystemExit("the dataset / synthetic modes need --split {train,val,test}")
    return load_checkpoints(a.ckpt)


def _class_names(a, C):
    from .run_moc import TASKS
    if a.synthetic or a.dataset not in TASKS:
        return [str(c) for c in range(C)]
    lab = TASKS[a.dataset]["labels"]
    if lab is None:
        csv_path = os.path.join(a.root, TASKS[a.dataset]["csv"])
        if not os.path.exists(csv_path):
            return [str(c) for c in range(C)]
        lab = {name: i for i, name in enumerate(dict.fromkeys(pd.read_csv(csv_path, dtype=str)["label"]))}
    names = [None] * C
    for k, v in lab.items():
        if 0 <= v < C:
            names[v] = str(k)
    return [n if n is not None else str(c) for c, n in enumerate(names)]


def _slides_loader(a, device):
    """--slides mode: a resident split of the CSV's slides (labels zero when the CSV has none) and the bank of --dataset."""
    from . import main_moc as M
    from .datasets import read_bag
    from .run_moc import TASKS, _load_weights
    df = pd.read_csv(a.slides, dtype={"slide_id": str})
    labeled = "label" in df.columns
    W, We = _load_weights(a, TASKS[a.dataset], device)
    M.set_classifier_bank(W, We)
    a.n_classes = int(W.size(1))
    label_map = TASKS[a.dataset]["labels"] or {}
    labels = []
    if labeled:
        for v in df["label"].tolist():
            labels.append(int(label_map[v]) if v in label_map else int(v))
    bags, coords, paths = [], [], []
    for sid in df["slide_id"].tolist():
        f, c, pth = read_bag(a.data_dir, sid)
        bags.append(f.to(torch.float32))
        coords.append(c)
        paths.append(pth)
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16}.get(a.bag_dtype)
    res = M.ResidentBags(bags, labels if labeled else [0] * len(bags), device, dtype=dt, paths=paths, coords=coords)
    return res, labeled, df["slide_id"].tolist()


def cli(argv=None):
    a = get_args(argv)
    sds = check_args(a)
    if not torch.cuda.is_available():
        raise RuntimeError("moc_amd needs a GPU: there is no CPU fallback")
    device = torch.device("cuda")
    if a.slides:
        loader, labeled, ids = _slides_loader(a, device)
    else:
        from . import run_moc
        ra = run_moc.get_args([])
        for k in ("root", "dataset", "shot", "fold", "topj", "topk", "discard_classifiers", "bag_dtype", "synthetic",
                  "disable_tqdm"):
            setattr(ra, k, getattr(a, k))
        loader = run_moc.prepare(ra, device)[SPLITS.index(a.split)]
        a.n_classes, labeled, ids = ra.n_classes, True, None
    a.class_names = _class_names(a, a.n_classes)
    p = predict(sds, loader, device, a, labeled=labeled, slide_ids=ids, maps=a.patch_maps)
    info = {"args": {k: getattr(a, k) for k in ("slides", "data_dir", "synthetic", "dataset", "shot", "fold", "split", "root",
                                                "topj", "topk", "discard_classifiers", "bag_dtype")},
            "checkpoints": [os.path.abspath(c) for c in a.ckpt]}
    m = metrics(p, a, n_div=len(loader.dataset)) if labeled else None
    write_predictions(p, a.out, info, m)
    if a.patch_maps:
        from .patch_maps import write_ensemble_maps
        write_ensemble_maps(p.maps, os.path.join(a.out, "patch_maps"), p.slide_ids)
    print(f"predict: {len(p.slide_ids)} slides x {len(sds)} model(s) -> {a.out}" + (f"; ensemble {m['ensemble']}" if m else ""))
    return p, m


if __name__ == "__main__":
    cli()
