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

`--banks NAME=W.pt,W_ext.pt [NAME=...]` adds the prompt-bank axis: every bank (saved tensors [D, C] and [D, Ce], one class
count, at most 16 columns each) gets the tables above from ONE read of the bags per group of banks
(main_moc.evaluation_sweep_banks / zs_evaluation_sweep_banks).  `--ckpt` then takes one checkpoint for all banks or exactly
one per bank, in the banks' order.  DIR/<NAME>/ holds what the sweep writes for that bank alone, DIR/bank_summary.csv one
row per (bank, cell): the columns of sensitivity.csv behind a `bank` column.
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


def parse_bank(text):
    """`NAME=W.pt,W_ext.pt` -> (NAME, W.pt, W_ext.pt)."""
    name, eq, files = str(text).partition("=")
    parts = files.split(",")
    if not eq or not name or len(parts) != 2 or not all(parts) or os.sep in name or name in (".", ".."):
        raise argparse.ArgumentTypeError(f"a bank is NAME=W.pt,W_ext.pt (NAME becomes a directory name), got {text!r}")
    return name, parts[0], parts[1]


def get_args(argv=None):
    p = argparse.ArgumentParser(description="topj x topk x discard sensitivity tables of a MOC checkpoint from one score pass")
    p.add_argument("--ckpt", default=None, nargs="+",
                   help="a saved senet state_dict (best_model_*.pt); not needed for --zs alone.  With --banks: one for all "
                        "banks, or one per bank")
    p.add_argument("--banks", default=None, nargs="+", type=parse_bank, metavar="NAME=W.pt,W_ext.pt",
                   help="prompt banks to compare: saved [D, C] and [D, Ce] tensors, one class count, Ce <= 16")
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
    if a.banks is None and a.ckpt is not None:
        if len(a.ckpt) != 1:
            p.error("--ckpt takes one checkpoint (several only with --banks: one per bank)")
        a.ckpt = a.ckpt[0]
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
    if a.banks is not None:
        return None                      # (check_bank_args loads the banks' checkpoints)
    if a.ckpt is None:
        return None
    from .predict import load_checkpoints
    return load_checkpoints([a.ckpt])[0]


MAX_BANK_CE = 16       # engine.BANK_SET_MAX_CE (kept literal here, as MAX_TOPK is)


def check_bank_names(specs, flag="--banks"):
    """[(name, W file, W_ext file)]: duplicate names and missing files are refused (SystemExit).  Shared with run_moc --banks."""
    names = [n for n, _, _ in specs]
    dup = sorted({n for n in names if names.count(n) > 1})
    if dup:
        raise SystemExit(f"{flag}: duplicate bank name {dup[0]!r} (a name is its bank's output directory)")
    for _, fw, fe in specs:
        for f in (fw, fe):
            if not os.path.isfile(f):
                raise SystemExit(f"{flag}: {f}: no such file")


def load_bank_files(specs, flag="--banks", wide="the bank axis takes banks of at most {ce} (wide banks: one plain sweep per bank)",
                    mixed="run one sweep per class count"):
    """The banks' tensors from their files -> [(name, W, W_ext)] host fp32; a file that does not hold W [D, C] / W_ext [D, Ce]
    with Ce > C, a bank wider than MAX_BANK_CE columns and banks of different C are refused (SystemExit)."""
    banks = []
    for name, fw, fe in specs:
        W, We = (torch.load(f, map_location="cpu") for f in (fw, fe))
        if not (torch.is_tensor(W) and torch.is_tensor(We) and W.dim() == 2 and We.dim() == 2 and W.size(0) == We.size(0)
                and We.size(1) > W.size(1)):
            raise SystemExit(f"{flag}: {name}: need saved tensors W [D, C] and W_ext [D, Ce] with Ce > C")
        if We.size(1) > MAX_BANK_CE:
            raise SystemExit(f"{flag}: {name}: Ce={We.size(1)} columns; " + wide.format(ce=MAX_BANK_CE))
        banks.append((name, W.float(), We.float()))
    Cs = sorted({int(W.size(1)) for _, W, _ in banks})
    if len(Cs) != 1:
        raise SystemExit(f"{flag}: banks of different C ({Cs}) do not share a score pass; {mixed}")
    return banks


def check_bank_args(a):
    """--banks: refusals from the command line and the files alone, before any GPU work -> ([(name, W, W_ext)] host
    tensors, the checkpoints' state_dicts: none, one, or one per bank)."""
    check_bank_names(a.banks)
    n_ckpt = len(a.ckpt or ())
    if n_ckpt not in (0, 1, len(a.banks)):
        raise SystemExit(f"--ckpt: one checkpoint for all banks or one per bank ({len(a.banks)}); got {n_ckpt}")
    banks = load_bank_files(a.banks)
    sds = []
    if n_ckpt:
        from .predict import load_checkpoints
        sds = load_checkpoints(list(a.ckpt))
    return banks, sds


def write_bank_summary(out_dir, names, eval_tables=None, zs_tables=None):
    """DIR/bank_summary.csv: one row per (bank, cell) -- sensitivity.csv's columns behind `bank`, banks in the given order.
    A pure function of its arguments (no GPU).  -> the rows."""
    os.makedirs(out_dir, exist_ok=True)
    rows = []
    for g, name in enumerate(names):
        for r in flatten(eval_tables[g] if eval_tables else None, zs_tables[g] if zs_tables else None):
            rows.append({"bank": name, **r})
    df = pd.DataFrame(rows, columns=["bank", "kind", "topj", "topk", "discard", "loss", "acc", "auc"])
    df["topj"] = df["topj"].astype("Int64")
    df.to_csv(os.path.join(out_dir, "bank_summary.csv"), index=False, float_format="%.17g")
    return rows


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
    bank_files = check_bank_args(a) if a.banks is not None else None
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
    if bank_files is not None:
        return _cli_banks(a, M, loader, device, *bank_files)
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


def _cli_banks(a, M, loader, device, banks, sds):
    """The --banks run: -> ({name: evaluation table} or None, {name: zero-shot table} or None)."""
    names = [n for n, _, _ in banks]
    tensors = [(W.to(device), We.to(device)) for _, W, We in banks]
    eval_tables = zs_tables = None
    if sds:
        models = []
        for sd in sds:
            m = M.senet(int(sd["model.0.weight"].shape[-1]), 4).to(device)
            m.load_state_dict(sd)
            models.append(m)
        eval_tables = M.evaluation_sweep_banks(models, loader, device, a, tensors, a.topjs, a.topks, a.discard_sets)
    if a.zs:
        zs_tables = M.zs_evaluation_sweep_banks(loader, device, a, tensors, a.topks)
    info = {k: getattr(a, k) for k in ("slides", "data_dir", "synthetic", "dataset", "shot", "fold", "split", "root",
                                       "topjs", "topks", "zs", "bag_dtype")}
    info["discard_sets"] = [discard_name(d) for d in a.discard_sets]
    for g, (name, fw, fe) in enumerate(a.banks):
        ck = None if not a.ckpt else a.ckpt[g if len(a.ckpt) > 1 else 0]
        write_sensitivity(os.path.join(a.out, name), eval_tables[g] if eval_tables else None, zs_tables[g] if zs_tables else None,
                          dict(info, ckpt=ck, bank=name, bank_files=[fw, fe]))
    rows = write_bank_summary(a.out, names, eval_tables, zs_tables)
    print(f"sweep: {len(rows)} cells over {len(names)} banks x {len(loader.dataset)} slides -> {a.out}")
    return (dict(zip(names, eval_tables)) if eval_tables else None, dict(zip(names, zs_tables)) if zs_tables else None)


if __name__ == "__main__":
    cli()
