"""Sensitivity tables of a trained checkpoint (and of the zero-shot bank alone): how loss / accuracy / AUC move with
--topj, --topk and the discard set (the component ablation), over one split, from ONE score pass.

    python -m moc_amd.sweep --ckpt best.pt --topjs 100,200,400,800 --topks 1,5,10,20,50 \\
        [--discard_sets none topk delta_softmax delta_diff bottomk] [--zs] --split test --out DIR

The inputs are predict's three: `--synthetic N --shot S`, a split of the dataset's tables, or `--slides CSV --data_dir
DIR` (the CSV needs a label column here).  A discard set is the classifier names joined with `+` (`topk+bottomk`);
`none` is the empty set.  `--zs` adds the zero-shot table (the four pooling functions x topks) and needs no checkpoint
when given alone.  Writes DIR/sensitivity.json (both tables, tuple keys flattened to strings, and the arguments) and
DIR/sensitivity.csv (one row per cell: kind, topj, topk, discard, loss, acc, auc).

The work is main_moc.evaluation_sweep / zs_evaluation_sweep: every cell is exactly what evaluation() / zs_evaluation()
returns with those arguments.
"""
from __future__ import annotations

import argparse
import json
import os

import pandas as pd
import torch

from ._lib import SEL_BITS
from .predict import SPLITS

MAX_TOPK = 64          # main_moc.SWEEP_MAX_TOPK (kept literal here: parsing needs no GPU library)


def _int_list(text):
    try:
        out = [int(v) for v in str(text).split(",") if v.strip() != ""]
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a comma-separated list of integers: {text!r}")
    if not out or min(out) < 1:
        raise argparse.ArgumentTypeError(f"a non-empty list of integers >= 1 is needed, got {text!r}")
    return out


def parse_discard_set(text):
    """`none` -> (), `topk+bottomk` -> ("topk", "bottomk")."""
    text = str(text).strip()
    if text in ("none", ""):
        return ()
    names = tuple(text.split("+"))
    bad = [n for n in names if n not in SEL_BITS]
    if bad or len(set(names)) != len(names):
        raise argparse.ArgumentTypeError(f"discard set {text!r}: classifier names are {sorted(SEL_BITS)}, joined with +, or none")
    return names


def discard_name(d):
    return "+".join(d) if d else "none"


def get_args(argv=None):
    p = argparse.ArgumentParser(description="topj x topk x discard sensitivity tables of a MOC checkpoint from one score pass")
    p.add_argument("--ckpt", default=None, help="a saved senet state_dict (best_model_*.pt); not needed for --zs alone")
    p.add_argument("--out", required=True, help="output directory (sensitivity.json, sensitivity.csv)")
    p.add_argument("--topjs", type=_int_list, default=None, help="comma-separated topj values, e.g. 100,200,400,800")
    p.add_argument("--topks", type=_int_list, required=True, help=f"comma-separated topk values, each <= {MAX_TOPK}")
    p.add_argument("--discard_sets", nargs="+", type=parse_discard_set, default=None,
                   help="discard sets: classifier names joined with + (topk+bottomk), or none")
    p.add_argument("--zs", action="store_true", help="also the zero-shot table: the four pooling functions x topks")
    p.add_argument("--slides", default=None, help="CSV with a slide_id and a label column")
    p.add_argument("--data_dir", default=None, help="--slides: directory holding h5_files/, pt_files/ or npy_files/")
    p.add_argument("--synthetic", type=int, default=0, help="the generated slides of run_moc --synthetic N")
    p.add_argument("--split", default=None, choices=SPLITS, help="dataset / synthetic modes: which split")
    p.add_argument("--dataset", default="nsclc", help="task: label map and zero-shot bank (run_moc --dataset)")
    p.add_argument("--shot", type=int, default=1)
    p.add_argument("--fold", type=int, default=0)
    p.add_argument("--root", default=".", help="directory holding dataset_csv/, splits/, data/, models/ (run_moc --root)")
    p.add_argument("--bag_dtype", default="fp32", choices=["fp32", "bf16", "fp16"])
    p.add_argument("--disable_tqdm", action="store_true")
    a = p.parse_args(argv)
    if a.ckpt is None and not a.zs:
        p.error("--ckpt is needed (only --zs alone runs without a checkpoint)")
    if a.ckpt is not None and a.topjs is None:
        p.error("--topjs is needed with --ckpt")
    if max(a.topks) > MAX_TOPK:
        p.error(f"--topks: every topk must be <= {MAX_TOPK} (one ranking serves K <= {MAX_TOPK})")
    if a.discard_sets is None:
        a.discard_sets = [()]
    a.pretrain = "conch"
    # the fields evaluation()'s args carry; every cell overrides the three that are swept
    a.topj, a.topk, a.discard_classifiers = (a.topjs or [10])[0], a.topks[0], list(a.discard_sets[0])
    return a


def check_args(a):
    """Refusals from the command line and the files alone, before any GPU work -> the checkpoint's state_dict or None."""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("sweep is a one-GPU tool: run it without a launcher")
    if sum([bool(a.slides), a.synthetic > 0]) > 1:
        raise SystemExit("give exactly one input: --slides CSV, --synthetic N, or --dataset/--shot/--fold/--split")
    if a.slides:
        if not a.data_dir:
            raise SystemExit("--slides needs --data_dir")
        if a.split:
            raise SystemExit("--split belongs to the dataset / synthetic modes, not to --slides")
        df = pd.read_csv(a.slides, dtype={"slide_id": str})
        if "slide_id" not in df.columns or "label" not in df.columns:
            raise SystemExit(f"{a.slides}: a sensitivity table needs slide_id and label columns")
    elif not a.split:
        raise SystemExit("the dataset / synthetic modes need --split {train,val,test}")
    if a.ckpt is None:
        return None
    from .predict import load_checkpoints
    return load_checkpoints([a.ckpt])[0]


def flatten(eval_table=None, zs_table=None):
    """The two dicts of evaluation_sweep / zs_evaluation_sweep as rows (kind, topj, topk, discard, loss, acc, auc): `eval`
    rows carry topj and the discard set's spelling; zero-shot rows name their pooling function in `kind`
    (`zs:<function>`) and leave topj and discard empty."""
    rows = []
    for (j, k, d), m in (eval_table or {}).items():
        rows.append({"kind": "eval", "topj": int(j), "topk": int(k), "discard": discard_name(tuple(d)),
                     "loss": float(m["loss"]), "acc": float(m["acc"]), "auc": float(m["auc"])})
    for (name, k), m in (zs_table or {}).items():
        rows.append({"kind": f"zs:{name}", "topj": None, "topk": int(k), "discard": None,
                     "loss": float(m["loss"]), "acc": float(m["acc"]), "auc": float(m["auc"])})
    return rows


def write_sensitivity(out_dir, eval_table=None, zs_table=None, info=None):
    """DIR/sensitivity.json: {"args": info, "evaluation": {"topj=J,topk=K,discard=D": {loss, acc, auc}},
    "zero_shot": {"<function>,topk=K": {...}}} and DIR/sensitivity.csv, one row per cell.  A pure function of its
    arguments (no GPU).  -> the JSON document."""
    os.makedirs(out_dir, exist_ok=True)
    doc = {"args": dict(info or {})}
    if eval_table is not None:
        doc["evaluation"] = {f"topj={int(j)},topk={int(k)},discard={discard_name(tuple(d))}": dict(m)
                             for (j, k, d), m in eval_table.items()}
    if zs_table is not None:
        doc["zero_shot"] = {f"{name},topk={int(k)}": dict(m) for (name, k), m in zs_table.items()}
    with open(os.path.join(out_dir, "sensitivity.json"), "w") as f:
        json.dump(doc, f, indent=2)
    rows = flatten(eval_table, zs_table)
    df = pd.DataFrame(rows, columns=["kind", "topj", "topk", "discard", "loss", "acc", "auc"])
    df["topj"] = df["topj"].astype("Int64")                 # (empty in zero-shot rows; whole numbers elsewhere)
    df.to_csv(os.path.join(out_dir, "sensitivity.csv"), index=False, float_format="%.17g")
    return doc


def cli(argv=None):
    a = get_args(argv)
    sd = check_args(a)
    if not torch.cuda.is_available():
        raise RuntimeError("moc_amd needs a GPU: there is no CPU fallback")
    from . import main_moc as M
    device = torch.device("cuda")
    if a.slides:
        from .predict import _slides_loader
        loader, _, _ = _slides_loader(a, device)
    else:
        from . import run_moc
        ra = run_moc.get_args([])
        for k in ("root", "dataset", "shot", "fold", "topj", "topk", "discard_classifiers", "bag_dtype", "synthetic",
                  "disable_tqdm"):
            setattr(ra, k, getattr(a, k))
        loader = run_moc.prepare(ra, device)[SPLITS.index(a.split)]
        a.n_classes = ra.n_classes
    eval_table = zs_table = None
    if sd is not None:
        D = int(sd["model.0.weight"].shape[-1])
        model = M.senet(D, 4).to(device)
        model.load_state_dict(sd)
        eval_table = M.evaluation_sweep(model, loader, device, a, a.topjs, a.topks, a.discard_sets)
    if a.zs:
        zs_table = M.zs_evaluation_sweep(loader, device, a, a.topks)
    info = {k: getattr(a, k) for k in ("ckpt", "slides", "data_dir", "synthetic", "dataset", "shot", "fold", "split", "root",
                                       "topjs", "topks", "zs", "bag_dtype")}
    info["discard_sets"] = [discard_name(d) for d in a.discard_sets]
    write_sensitivity(a.out, eval_table, zs_table, info)
    n = len(eval_table or {}) + len(zs_table or {})
    print(f"sweep: {n} cells over {len(loader.dataset)} slides -> {a.out}")
    return eval_table, zs_table


if __name__ == "__main__":
    cli()
