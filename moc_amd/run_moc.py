"""Driver for the MOC path: the command line, data/weight
preparation, `main()` and `--summary` of the reference's main_moc.py (:29-127, :161-293, :586-644)
around the GPU callables of moc_amd.main_moc.

    python -m moc_amd.run_moc --fold 0 --shot 16 --topj 400 --topk 10 --dataset nsclc
    python -m moc_amd.run_moc --summary --summary_dir results/moc_train/nsclc
    python -m moc_amd.run_moc --synthetic 24 --shot 4 --disable_tqdm        # no data needed
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 -m moc_amd.run_moc ...   # 8 GPUs
    python -m moc_amd.run_moc --folds 0,1,2,3,4 --shot 16 --seed 1 ...      # five folds in ONE process, stepped in lockstep
    python -m moc_amd.run_moc --shots 1,2,4,8,16 --folds 0,1,2,3,4 --seed 1 ...   # the launcher's whole grid in one process
    python -m moc_amd.run_moc --topjs 100,400 --topks 5,10 --discard_sets none topk+bottomk --folds 0,1,2,3,4 --seed 1 ...   # a hyper-parameter grid
    python -m moc_amd.run_moc --seeds 1,2,3 --lrs 3e-4,1e-3,3e-3 --wds 0,1e-4 --folds 0,1,2,3,4 --shot 16 ...   # an optimizer grid

Same flags and defaults as the reference, same result files (`zs_results_*`, `best_results_*`,
`ablation_results_*`, `best_model_*.pt`, `summary_*.csv`) with the same keys.  Differences, all
additive: the dataset branch is table driven (ebrains12 / ebrains30 work like nsclc / rcc); the
CONCH text tower is not part of this path, so the zero-shot weights must already be cached under
`models/classifier_weights/` (the reference caches them there on first run, main_moc.py:149-197);
`--bag_dtype bf16|fp16` stores bags as bfloat16 / float16; `--resident 0` falls back to per-epoch re-reads;
`--synthetic N` runs the whole loop on N generated slides per split; `--patch_maps SPLIT` writes per-patch maps with the
best checkpoint after training, `--patch_maps_from best_model_*.pt` only those (moc_amd.patch_maps).

Under a launcher (WORLD_SIZE > 1) every split is spread over the GPUs (each rank reads only its block of slides):
training is the exact-sequential mode -- phase A where the bags are, the compact results all-gathered, the reference's
one-Adam-step-per-slide recurrence on every rank (moc_amd.dist.train_seq: the numbers of a one-GPU run, bit for bit) --
and the evaluations shard by slide with one gather of the pooled logits (moc_amd.dist.evaluation).  Rank 0 prints and
writes the result files.
"""
from __future__ import annotations

import argparse
import copy
import json
import os
from glob import glob

import numpy as np
import pandas as pd
import torch

from . import dist as mdist
from . import main_moc as M
from .datasets import Generic_MIL_Dataset, to_resident, to_sharded

# dataset -> (csv, split dir, label map, weight file stems)   main_moc.py:161-293
TASKS = {
    "nsclc": dict(csv="dataset_csv/nsclc.csv", splits="splits/nsclc_fewshot", data="data/nsclc",
                  labels={"LUAD": 0, "LUSC": 1}, weights="weights_nsclc_conch.pt", weights_ext="weights_nsclc_ext_conch.pt"),
    "rcc": dict(csv="dataset_csv/rcc.csv", splits="splits/rcc_fewshot", data="data/rcc",
                labels={"KICH": 0, "KIRC": 1, "KIRP": 2}, weights="weights_rcc_conch.pt", weights_ext="weights_rcc_ext_conch.pt"),
    "ebrains12": dict(csv="dataset_csv/ebrains12.csv", splits="splits/ebrains12_fewshot", data="data/ebrains12",
                      labels=None, weights="weights_ebrains12_conch.pt", weights_ext="weights_ebrains12_ext_conch.pt"),
    "ebrains30": dict(csv="dataset_csv/ebrains30.csv", splits="splits/ebrains30_fewshot", data="data/ebrains30",
                      labels=None, weights="weights_ebrains30_conch.pt", weights_ext="weights_ebrains30_ext_conch.pt"),
}


def get_args(argv=None):
    p = argparse.ArgumentParser(description="Configurations for WSI Training")
    p.add_argument("--fold", type=int, default=0, help="fold number")
    p.add_argument("--shot", type=int, default=1, help="split number")
    p.add_argument("--topj", type=int, default=10, help="topj for classifier selection")
    p.add_argument("--topk", type=int, default=10, help="topk for final pooling")
    p.add_argument("--result_dir", type=str, default="results/moc_train", help="result directory")
    p.add_argument("--dataset", type=str, default="nsclc", choices=sorted(TASKS), help="dataset name")
    p.add_argument("--pretrain", type=str, default="conch", choices=["conch"], help="pretrain model")
    p.add_argument("--disable_tqdm", action="store_true", help="disable tqdm for better log")
    p.add_argument("--discard_classifiers", nargs="+", default=[], help="topk, delta_softmax, delta_diff, bottomk")
    p.add_argument("--load_weight", type=bool, default=True, help="load stored classifier weight")
    p.add_argument("--check_zeroshot", type=bool, default=True, help="get zero-shot results")
    p.add_argument("--ablation_study", type=str, default="none", choices=["none", "avg", "sum", "max"], help="ablation study")
    p.add_argument("--summary", action="store_true", help="summary results, no training")
    p.add_argument("--summary_dir", type=str, default="")
    # additive
    p.add_argument("--root", type=str, default=".", help="directory holding dataset_csv/, splits/, data/, models/")
    p.add_argument("--bag_dtype", type=str, default="fp32", choices=["fp32", "bf16", "fp16"], help="bag storage in HBM")
    p.add_argument("--resident", type=int, default=1, help="keep each split packed in HBM across epochs")
    p.add_argument("--loader_seed_draw", type=int, default=0,
                   help="resident splits make the base-seed draw a DataLoader makes per pass (the reference's exact mask stream)")
    p.add_argument("--epochs", type=int, default=25, help="main_moc.py:611 hard-codes 25")
    p.add_argument("--synthetic", type=int, default=0, help="run on N generated slides per split instead of files")
    p.add_argument("--seed", type=int, default=None, help="torch.manual_seed before building the meta-learner")
    p.add_argument("--cache_scores", type=int, default=0,
                   help="1: keep the per-row statistics of the resident train split from one score pass and re-use them every "
                        "epoch (the bank is frozen: the same bits as recomputing them, main_moc.py:336-337, without reading the bags)")
    p.add_argument("--folds", type=str, default="",
                   help="comma-separated folds: train them ALL in this process, stepped in lockstep (moc_amd.main_moc.train_runs) -- "
                        "what scripts/moc_train.sh starts as one process per fold.  Every fold's numbers and files are those of "
                        "`--fold F` alone (with --seed: bit for bit).  Under a launcher the folds are dealt to the ranks, no "
                        "communication")
    p.add_argument("--shots", type=str, default="",
                   help="comma-separated shot counts: train every (shot, fold) pair of --shots x --folds (without --folds: the one "
                        "--fold) in this process -- scripts/moc_train.sh's whole grid.  Run (S, F) writes into "
                        "{result_dir}/{S}_shot/ what `--fold F --shot S --result_dir {result_dir}/{S}_shot` writes alone, so that "
                        "`--summary --summary_dir {result_dir}` reads the tree.  Under a launcher the pairs are dealt to the ranks")
    p.add_argument("--topjs", type=str, default=None,
                   help="comma-separated topj values: train every configuration of --topjs x --topks x --discard_sets (a list that "
                        "is not given: the one --topj / --topk / --discard_classifiers) for every fold of --folds (or the one --fold) "
                        "in this process.  Run (J, K, set, F) writes into {result_dir}/topj{J}_topk{K}_{set}/ what `--topj J --topk K "
                        "--discard_classifiers ... --fold F --result_dir {that dir}` writes alone.  With --seed the configurations "
                        "of a fold draw the same masks and share one score pass per epoch (moc_amd.runs)")
    p.add_argument("--topks", type=str, default=None, help="comma-separated topk values (see --topjs)")
    p.add_argument("--discard_sets", nargs="*", default=None,
                   help="discard sets, classifier names joined with + (topk+bottomk), `none` for the empty set (see --topjs)")
    p.add_argument("--lr", type=float, default=1e-3, help="Adam's learning rate (main_moc.py:316 hard-codes 1e-3)")
    p.add_argument("--weight_decay", type=float, default=1e-4, help="Adam's coupled weight decay (main_moc.py:316 hard-codes 1e-4)")
    p.add_argument("--seeds", type=str, default=None,
                   help="comma-separated seeds: train every cell of --seeds x --lrs x --wds (a list that is not given: the one "
                        "--seed / --lr / --weight_decay) for every fold of --folds (or the one --fold) in this process.  Cell "
                        "(S, LR, WD) of fold F writes into {result_dir}/seed{S}_lr{LR}_wd{WD}/ what `--fold F --seed S --lr LR "
                        "--weight_decay WD --result_dir {that dir}` writes alone, and {result_dir}/opt_grid_summary.csv holds one "
                        "line per (lr, wd).  The cells of a (seed, fold) start from one meta-learner and one mask stream: they "
                        "share a score pass per epoch and step in one lockstep chain, each with its own Adam (moc_amd.runs)")
    p.add_argument("--lrs", type=str, default=None, help="comma-separated learning rates (see --seeds)")
    p.add_argument("--wds", type=str, default=None, help="comma-separated weight decays (see --seeds)")
    p.add_argument("--banks", default=None, nargs="+", type=_parse_bank, metavar="NAME=W.pt,W_ext.pt",
                   help="prompt banks to compare in the few-shot setting: saved [D, C] and [D, Ce] tensors, one class count, "
                        "Ce <= 16 (moc_amd.sweep --banks takes the same).  Trains a meta-learner under EVERY bank for every fold of "
                        "--folds (or the one --fold) in this process; needs --seed: the banks' runs of a fold then draw the same "
                        "masks and share one multi-bank score pass per epoch (moc_amd.runs).  Run (NAME, F) writes into "
                        "{result_dir}/bank_{NAME}/ what `--fold F` alone writes with that bank installed, and "
                        "{result_dir}/bank_grid_summary.csv holds one line per bank")
    p.add_argument("--patch_maps", type=str, default=None, choices=list(PATCH_MAP_CHOICES),
                   help="after main(), write per-patch maps (moc_amd.patch_maps) of these splits with the best checkpoint to "
                        "{result_dir}/patch_maps_shot_S_fold_F/{split}/ (default: none; test with --patch_maps_from)")
    p.add_argument("--patch_maps_from", type=str, default=None,
                   help="inference only: load this saved state dict, skip zero-shot and training, write the patch maps of "
                        "the --patch_maps splits and patch_maps_results_shot_S_fold_F.json (each split's evaluation())")
    return p.parse_args(argv)


PATCH_MAP_CHOICES = ("none", "train", "val", "test", "all")


def _parse_bank(text):
    from .sweep import parse_bank
    return parse_bank(text)


def patch_map_splits(args):
    """The splits `--patch_maps` / `--patch_maps_from` ask for, in train, val, test order."""
    want = args.patch_maps or ("test" if args.patch_maps_from else "none")
    return {"none": [], "all": ["train", "val", "test"]}.get(want, [want])


def check_patch_map_args(args):
    """Refusals of the patch-map flags, from the command line alone (before any GPU work)."""
    if not patch_map_splits(args) and not args.patch_maps_from:
        return
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("--patch_maps / --patch_maps_from are one-GPU options: run them without a launcher")
    if args.folds or getattr(args, "shots", ""):
        raise SystemExit("--patch_maps / --patch_maps_from do not combine with --folds / --shots: run one --fold and --shot at a time")
    if args.ablation_study != "none":
        raise SystemExit("--patch_maps / --patch_maps_from need the meta-learner: the ablation study trains none")


# ------------------------------------------------------------------ --summary (main_moc.py:53-127)
def _fold_results(summary_dir, shot, pattern="best_results_shot_{shot}_fold_{fold}.json"):
    out = []
    for fold in range(5):
        with open(os.path.join(summary_dir, pattern.format(shot=shot, fold=fold))) as f:
            out.append(json.load(f))
    return out


def summary(args):
    print("start summary")
    for shot in [1, 2, 4, 8]:
        summary_dir = args.summary_dir + f"/{shot}_shot"
        if not os.path.isdir(summary_dir):          # a directory that holds the result files itself (a grid's configuration directory)
            summary_dir = args.summary_dir
        summary_file = os.path.join(args.summary_dir, f"summary_{shot}.csv")
        folds = [0, 1, 2, 3, 4, "mean"]

        def fresh():
            if os.path.exists(summary_file):
                os.remove(summary_file)

        def col(vals):
            return list(vals) + [np.mean(vals)]
        try:
            fresh()
            r = _fold_results(summary_dir, shot)
            pd.DataFrame({"fold": folds, "test_auc": col([x["test_at_best_val"] for x in r]),
                          "zs_test_auc": col([x["zero_shot_test"]["auc"] for x in r]),
                          "test_acc": col([x["test_acc_at_best_val"] for x in r]),
                          "zs_test_acc": col([x["zero_shot_test"]["acc"] for x in r])}).to_csv(summary_file, index=False)
        except Exception:
            try:      # probably no zero-shot results
                fresh()
                r = _fold_results(summary_dir, shot)
                pd.DataFrame({"fold": folds, "test_auc": col([x["test_at_best_val"] for x in r]),
                              "test_acc": col([x["test_acc_at_best_val"] for x in r])}).to_csv(summary_file, index=False)
            except Exception:
                try:  # probably an ablation study
                    fresh()
                    r = []
                    for fold in range(5):
                        with open(glob(os.path.join(summary_dir, f"*_shot_{shot}_fold_{fold}.json"))[0]) as f:
                            r.append(json.load(f))
                    pd.DataFrame({"fold": folds, "auc": col([x["auc"] for x in r]),
                                  "acc": col([x["acc"] for x in r])}).to_csv(summary_file, index=False)
                except Exception:
                    print(f"shot {shot} summary failed")
    print("end summary")


# ------------------------------------------------------------------ data / weights
def _load_weights(args, task, device):
    wdir = os.path.join(args.root, "models", "classifier_weights")
    paths = [os.path.join(wdir, task["weights"]), os.path.join(wdir, task["weights_ext"])]
    for pth in paths:
        if not os.path.exists(pth):
            raise FileNotFoundError(
                f"{pth} is missing.  The zero-shot classifier weights come from the CONCH text tower "
                "(utils/zeroshot_utils.py:20-51), which is outside this path; run the reference once "
                "(it caches them there, main_moc.py:149-197) or copy the two .pt files.")
    W, We = (torch.load(pth, map_location="cpu").to(torch.float32) for pth in paths)
    print("zershot weights shape: ", W.shape)
    print("zershot weights_ext shape: ", We.shape)
    return W.to(device), We.to(device)


def _synthetic_splits(args, C):
    """(seed base, slides, visits per pass or None) of the generated train / val / test split of (args.shot, args.fold)."""
    fo = 17 * int(getattr(args, "fold", 0))          # (every fold its own generated slides; fold 0: the fixtures' slides)
    return ((100 + fo, args.shot * C, args.shot * C), (5000 + fo, args.synthetic, None), (9000 + fo, args.synthetic, None))


def _synthetic_classes(args):
    return 2 if args.dataset == "nsclc" else 3 if args.dataset == "rcc" else 12 if args.dataset == "ebrains12" else 30


def _label_map(args):
    """The dataset's label map: the table's own, or (table driven) its classes in order of first appearance."""
    task = TASKS[args.dataset]
    labels = task["labels"]
    if labels is None:
        seen = list(dict.fromkeys(pd.read_csv(os.path.join(args.root, task["csv"]), dtype=str)["label"]))
        labels = {name: i for i, name in enumerate(seen)}
    return labels


def _real_splits(args):
    """The reference's dataset object and the three splits of (args.shot, args.fold), nothing loaded yet."""
    task = TASKS[args.dataset]
    labels = _label_map(args)
    csv_path = os.path.join(args.root, task["csv"])
    data_dir = os.path.join(args.root, task["data"], "merge_features_conch")
    dataset = Generic_MIL_Dataset(csv_path=csv_path, data_dir=data_dir, shuffle=False, seed=1, print_info=True,
                                  label_dict=labels, patient_strat=False, ignore=[])
    dataset.load_from_h5(True)
    dataset.load_full_path(True)
    splits = dataset.return_splits(from_id=False,
                                   csv_path=os.path.join(args.root, task["splits"], f"{args.shot}shots", f"splits_{args.fold}.csv"),
                                   repeat_num=int(args.shot) * len(labels))
    return labels, splits


def split_footprints(args):
    """[(share key, bag rows)] of the train / val / test split of (args.shot, args.fold) WITHOUT loading a bag: two runs whose
    keys for a split are equal visit the same slides in the same order and hold that split once (`prepare(share=)`)."""
    if args.synthetic:
        from . import synth
        C = _synthetic_classes(args)
        return [(("synthetic", s, base, n), int(sum(synth.bag_sizes(base, n, 3000, fixed=False, lo=500, hi=8000))))
                for s, (base, n, _) in enumerate(_synthetic_splits(args, C))]
    from .datasets import bag_rows
    _, splits = _real_splits(args)
    out = []
    for s_i, sp in enumerate(splits):
        ids = tuple(str(v) for v in sp.slide_data["slide_id"])
        out.append((("files", s_i, ids), sum(bag_rows(sp.data_dir, i, FEATURE_DIM) for i in ids)))
    return out


FEATURE_DIM = 512        # CONCH embeddings: the width of the bags and of the meta-learner this driver builds (main_moc.py:315)


def grid_bytes(footprints, D, itemsize, C):
    """Device bytes a grid of runs holds: `footprints[r]` = split_footprints of run r.  An estimate from the row counts: pure.
      * the bags of every DISTINCT split once (splits that two runs list alike are shared);
      * the work arrays of the evaluation passes per VISIT (main_moc.evaluation_runs puts a shared split into its batch
        once for every run that names it): statistics, selection, candidates and mixed scores per row -- no H1 / gates --
        for every run's train and validation split (the plan of every epoch) and twice for its test split (the plans of
        two different sets of improved runs are kept, main_moc.EVAL_RUN_PLANS);
      * every DISTINCT train split a second time (runs.TrainRuns packs its runs' bags; splits that are one object -- the
        configurations of a fold in a hyper-parameter grid -- once), and two sets of training work arrays per run;
      * the largest one-time packing copy (the splits of an evaluation pass are laid side by side)."""
    ws_eval = 4 * (2 * C + 3) + 4 * (2 * C + 2) + 13 + 4 * C
    ws_train = ws_eval + 4 * 64 + 16 + 8
    seen, total, pack = set(), 0, [0, 0]
    for fp in footprints:
        for s_i, (key, rows) in enumerate(fp):
            if key not in seen:
                seen.add(key)
                total += rows * D * itemsize
                pack[0 if s_i < 2 else 1] += rows * D * itemsize
        (tr_key, tr), (_, va), (_, te) = fp
        total += (tr + va + 2 * te) * ws_eval + tr * 2 * ws_train
        if ("train copy", tr_key) not in seen:
            seen.add(("train copy", tr_key))
            total += tr * D * itemsize
    return total + max(pack)


def largest_grid(footprints, D, itemsize, C, free_bytes):
    """How many of the leading runs of the grid fit into `free_bytes` (all of them: len(footprints))."""
    k = len(footprints)
    while k > 0 and grid_bytes(footprints[:k], D, itemsize, C) > free_bytes:
        k -= 1
    return k


def prepare(args, device, share=None, share_train=False):
    """-> (train_loader, val_loader, test_loader) and the classifier bank installed in moc_amd.main_moc.  Inside a
    process group of more than one rank the three are moc_amd.dist.ShardedSplit objects (each rank holds its block).
    `share` (a dict kept by a caller that prepares several runs): a resident split whose key (split_footprints) is in it is
    not loaded again -- the runs share the object and its array (the train split too with `share_train`: the configurations of
    one fold in a hyper-parameter grid)."""
    import torch.distributed as dist
    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    if args.synthetic:
        from . import synth
        C = _synthetic_classes(args)
        args.n_classes = C
        W, We = synth.make_bank(1234, 512, C)
        M.set_classifier_bank(W.to(device), We.to(device))
        dt = {"bf16": torch.bfloat16, "fp16": torch.float16}.get(args.bag_dtype, torch.float32)
        loaders = []
        for s, (base, n, rep) in enumerate(_synthetic_splits(args, C)):
            key = ("synthetic", s, base, n)
            if share is not None and (s > 0 or share_train) and key in share:
                loaders.append(share[key])
                continue
            sizes = synth.bag_sizes(base, n, 3000, fixed=False, lo=500, hi=8000)
            if world > 1:                    # every rank generates only the slides of its block (seeds are per slide)
                blocks = mdist.block_lists(n, world)
                labels = [i % C for i in range(n)]
                bags = [synth.make_bag(base + i, sizes[i], 512, We, C, labels[i]) for i in blocks[rank]]
                loaders.append(mdist.SeqShardedBags(bags, sizes, labels, device, rank, world, dtype=dt) if s == 0 else
                               mdist.ShardedSplit(bags, blocks[rank], labels, blocks, device, dtype=dt))
                continue
            bags, labels = synth.make_slide_set(base, sizes, 512, We, C)
            loaders.append(M.ResidentBags(bags, labels, device, dtype=dt, repeat_num=rep, cache_scores=bool(args.cache_scores) and s == 0))
            if share is not None and (s > 0 or share_train):
                share[key] = loaders[-1]
        return loaders
    task = TASKS[args.dataset]
    labels, splits = _real_splits(args)
    args.n_classes = len(labels)
    W, We = _load_weights(args, task, device)
    assert W.size(1) == args.n_classes and We.size(1) > W.size(1), "classifier bank does not match the label map"
    M.set_classifier_bank(W, We)
    loaders = []
    for s_i, sp in enumerate(splits):
        sp.load_full_path(True)
        sp.load_from_h5(True)
        key = ("files", s_i, tuple(str(v) for v in sp.slide_data["slide_id"]))
        if share is not None and (s_i > 0 or share_train) and world == 1 and args.resident and key in share:
            loaders.append(share[key])
            continue
        if world > 1:
            loaders.append(to_sharded(sp, device, rank, world, {"bf16": torch.bfloat16, "fp16": torch.float16}.get(args.bag_dtype),
                                      train=(s_i == 0)))
        elif args.resident:
            loaders.append(to_resident(sp, device, {"bf16": torch.bfloat16, "fp16": torch.float16}.get(args.bag_dtype),
                                       loader_seed_draw=bool(args.loader_seed_draw)))
            loaders[-1].cache_scores = bool(args.cache_scores) and s_i == 0
            if share is not None and (s_i > 0 or share_train):
                share[key] = loaders[-1]
        else:
            loaders.append(torch.utils.data.DataLoader(sp, batch_size=1, shuffle=False, num_workers=1))
    return loaders


# ------------------------------------------------------------------ main (main_moc.py:586-644)
def _train(model, loader, optimizer, device, args):
    if isinstance(loader, mdist.SeqShardedBags):
        return mdist.train_seq(model, loader, optimizer, device, args)
    return M.train(model, loader, optimizer, device, args)


def _evaluation(model, loader, device, args):
    if isinstance(loader, mdist.ShardedSplit):
        return mdist.evaluation(model, loader, device, args)
    return M.evaluation(model, loader, device, args)


def _zs_evaluation(loader, device, args):
    if isinstance(loader, mdist.ShardedSplit):
        return mdist.zs_evaluation(loader, device, args)
    return M.zs_evaluation(loader, device, args)


def _is_main():
    import torch.distributed as dist
    return not dist.is_initialized() or dist.get_rank() == 0


class ResultBook:
    """What main() (main_moc.py:586-644) keeps, prints and writes for ONE run: its zero-shot numbers, the best validation AUC so
    far with the test numbers at it, the checkpoint and the two result files.  `a` carries the run's shot / fold / result_dir;
    every line goes through `say` behind `prefix`, and the files are written only with `write`."""

    def __init__(self, a, prefix="", say=print, write=True):
        self.a, self.prefix, self.say, self.write = a, prefix, say, write
        self.zs = (-1, -1, -1)
        self.best_val = self.test_at_best_val = self.test_acc_at_best_val = self.best_epoch = 0
        self.model_path = os.path.join(a.result_dir, f"best_model_shot_{a.shot}_fold_{a.fold}.pt")
        if write:
            os.makedirs(a.result_dir, exist_ok=True)

    def _dump(self, stem, obj):
        if self.write:
            with open(os.path.join(self.a.result_dir, f"{stem}_shot_{self.a.shot}_fold_{self.a.fold}.json"), "w") as f:
                json.dump(obj, f, indent=4)

    def say_zero_shot(self):
        self.say(f"{self.prefix}Zero-shot Train: {self.zs[0]}, Val: {self.zs[1]}, Test: {self.zs[2]}")

    def zero_shot(self, zs_train, zs_val, zs_test):
        self.zs = (zs_train, zs_val, zs_test)
        self.say_zero_shot()
        self._dump("zs_results", {"zs_train": zs_train, "zs_val": zs_val, "zs_test": zs_test})

    def improves(self, val_eval):
        """Whether this epoch visits the test split: only on a strictly better validation AUC (:618-628)."""
        return val_eval["auc"] > self.best_val

    def epoch(self, epoch, model, train_eval, val_eval, test_eval=None):
        """The epoch's line; with `test_eval` (the caller evaluated the test split because `improves(val_eval)`) the new best
        and the checkpoint."""
        if test_eval is None:
            self.say(f"{self.prefix}Epoch: {epoch}, Train: {train_eval}, Val: {val_eval}")
            return
        self.say(f"{self.prefix}Epoch: {epoch}, Train: {train_eval}, Val: {val_eval}, Test: {test_eval}")
        self.best_val, self.test_at_best_val, self.test_acc_at_best_val = val_eval["auc"], test_eval["auc"], test_eval["acc"]
        self.best_epoch = epoch
        if self.write:
            torch.save(model.state_dict(), self.model_path)

    def close(self):
        """The `Best Val` line and best_results_shot_S_fold_F.json -> the result dict."""
        self.say(f"{self.prefix}Best Val: {self.best_val}, Test at Best Val: {self.test_at_best_val}, "
                 f"Test acc: {self.test_acc_at_best_val}, Best Epoch: {self.best_epoch}")
        results = {
            "zero_shot_train": self.zs[0], "zero_shot_val": self.zs[1], "zero_shot_test": self.zs[2],
            "best_val": self.best_val, "test_at_best_val": self.test_at_best_val, "test_acc_at_best_val": self.test_acc_at_best_val,
            "best_epoch": self.best_epoch, "best_model_path": self.model_path,
        }
        self._dump("best_results", results)
        return results


def main(args, model, optimizer, train_loader, val_loader, test_loader, device):
    """main_moc.py:586-644.  The loaders are anything main_moc's loops take, or moc_amd.dist.ShardedSplit objects
    (multi-GPU: every rank calls this; rank 0 prints and writes)."""
    chief = _is_main()
    say = print if chief else (lambda *a, **k: None)
    if args.ablation_study != "none":
        if chief:
            os.makedirs(args.result_dir, exist_ok=True)
        ablation_eval_dict = (mdist.ablation_evaluation(test_loader, device, args) if isinstance(test_loader, mdist.ShardedSplit)
                              else M.ablation_evaluation(test_loader, device, args))
        say(f"Ablation Study: {args.ablation_study}, Test: {ablation_eval_dict}")
        if chief:
            with open(os.path.join(args.result_dir, f"ablation_results_{args.ablation_study}_shot_{args.shot}_fold_{args.fold}.json"), "w") as f:
                json.dump(ablation_eval_dict, f, indent=4)
        return ablation_eval_dict

    book = ResultBook(args, say=say, write=chief)         # every rank keeps the book (the test split is a collective); the chief speaks
    if args.check_zeroshot:
        book.zero_shot(_zs_evaluation(train_loader, device, args), _zs_evaluation(val_loader, device, args),
                       _zs_evaluation(test_loader, device, args))
    for epoch in range(getattr(args, "epochs", 25)):
        say("Epoch: ", epoch)
        _train(model, train_loader, optimizer, device, args)
        train_eval = _evaluation(model, train_loader, device, args)
        val_eval = _evaluation(model, val_loader, device, args)
        test_eval = _evaluation(model, test_loader, device, args) if book.improves(val_eval) else None
        book.epoch(epoch, model, train_eval, val_eval, test_eval)
    book.say_zero_shot()        # main alone, as the reference (:629): once more before the last line, -1s without --check_zeroshot
    results = book.close()
    say("\nEnd training.")
    return results


def write_split_maps(args, model, loaders, device):
    """The patch maps of the `patch_map_splits(args)` splits under {result_dir}/patch_maps_shot_S_fold_F/{split}/.
    -> {split: evaluation() of that split}."""
    from . import patch_maps as PM
    root = os.path.join(args.result_dir, f"patch_maps_shot_{args.shot}_fold_{args.fold}")
    out = {}
    for split in patch_map_splits(args):
        loader = loaders[("train", "val", "test").index(split)]
        out[split] = M.evaluation(model, loader, device, args)
        maps = PM.patch_maps(model, loader, device, args)
        PM.write_patch_maps(maps, os.path.join(root, split))
        print(f"patch maps: {len(maps)} slides of {split} -> {os.path.join(root, split)}")
    return out


def patch_maps_from(args, model, loaders, device):
    """--patch_maps_from: inference with a saved meta-learner -- no zero-shot pass, no training."""
    state = torch.load(args.patch_maps_from, map_location="cpu")
    model.load_state_dict(state)
    os.makedirs(args.result_dir, exist_ok=True)
    res = write_split_maps(args, model, loaders, device)
    with open(os.path.join(args.result_dir, f"patch_maps_results_shot_{args.shot}_fold_{args.fold}.json"), "w") as f:
        json.dump(res, f, indent=4)
    return res


def main_runs(args_list, models, optimizers, loaders_list, device, generators=None, per_run_adam=False):
    """main() (main_moc.py:586-644) for several runs at once: the zero-shot evaluations run per run, the training passes of
    all runs in lockstep (moc_amd.main_moc.train_runs), and every epoch's evaluations in one pass for all runs' train and
    validation splits, then one more for the test splits of the runs whose validation AUC improved (the reference visits
    the test set only then) -- moc_amd.main_moc.evaluation_runs.  `args_list[r]` carries run r's fold / shot / result_dir;
    loaders_list[r] = (train, val, test) resident splits.  Every run prints, saves and returns what main() would for it
    alone.  `per_run_adam`: an optimizer grid -- every run steps with its own optimizer's hyper-parameters.
    -> list of result dicts."""
    R = len(models)
    a0 = args_list[0]
    # a hyper-parameter grid: the runs of every configuration (topj, topk, discard set), in order of first appearance
    by_cfg = {}
    for r, a in enumerate(args_list):
        by_cfg.setdefault((a.topj, a.topk, tuple(a.discard_classifiers or ())), []).append(r)
    shots = len({a.shot for a in args_list}) > 1

    def tag(a):
        """What tells the run's lines from its neighbours': only what differs between the runs of this call."""
        return ((f"[seed {a.seed} lr {a.lr:g} wd {a.weight_decay:g}] " if per_run_adam else "")
                + (f"[topj {a.topj} topk {a.topk} {hgrid_discard_name(a.discard_classifiers)}] " if len(by_cfg) > 1 else "")
                + (f"[shot {a.shot} fold {a.fold}]" if shots else f"[fold {a.fold}]"))

    def evaluate(ms, lds):
        """evaluation_runs over (model, loader) pairs named by run index: its plan belongs to one `args`, so a grid evaluates
        configuration by configuration (every call is the one the configuration alone makes)."""
        if len(by_cfg) == 1:
            return M.evaluation_runs([models[r] for r in ms], lds, device, a0)
        out = [None] * len(ms)
        for rs in by_cfg.values():
            pick = [i for i, r in enumerate(ms) if r in rs]
            if pick:
                for i, e in zip(pick, M.evaluation_runs([models[ms[i]] for i in pick], [lds[i] for i in pick], device, args_list[rs[0]])):
                    out[i] = e
        return out
    assert a0.ablation_study == "none", "main_runs: the ablation study trains nothing -- run it per fold"
    books = [ResultBook(a, prefix=tag(a) + " ") for a in args_list]
    for a, book, (tr, va, te) in zip(args_list, books, loaders_list):
        if a.check_zeroshot:
            book.zero_shot(M.zs_evaluation(tr, device, a), M.zs_evaluation(va, device, a), M.zs_evaluation(te, device, a))
    trains = [ls[0] for ls in loaders_list]
    M.pack_splits(trains + [ls[1] for ls in loaders_list])       # (one array per pass of evaluation_runs, packed once)
    M.pack_splits([ls[2] for ls in loaders_list])
    for epoch in range(getattr(a0, "epochs", 25)):
        print("Epoch: ", epoch)
        M.train_runs(models, trains, optimizers, device, a0 if len(by_cfg) == 1 else list(args_list), generators=generators,
                     per_run_adam=per_run_adam)
        # all runs' train and validation splits in one pass, then the test splits of the runs that improved in another
        ev = evaluate(list(range(R)) + list(range(R)), trains + [ls[1] for ls in loaders_list])
        better = [r for r in range(R) if books[r].improves(ev[R + r])]
        ev_test = dict(zip(better, evaluate(better, [loaders_list[r][2] for r in better]))) if better else {}
        for r in range(R):
            books[r].epoch(epoch, models[r], ev[r], ev[R + r], ev_test.get(r))
    out = [book.close() for book in books]
    print("\nEnd training.")
    return out


def folds_of_rank(spec: str, rank: int, world: int):
    """The folds of `--folds a,b,...` this rank trains: dealt round-robin, every fold exactly once over the job (runs x
    GPUs: whole runs shard over the ranks, nothing is exchanged -- SURVEY.md section 8e, the reference's own launcher)."""
    folds = [int(v) for v in spec.split(",") if v.strip() != ""]
    assert len(set(folds)) == len(folds), "--folds: a fold named twice"
    return folds[rank::world]


def pairs_of_rank(shots: str, folds: str, shot: int, fold: int, rank: int, world: int):
    """The (shot, fold) pairs of `--shots a,b,... --folds c,d,...` this rank trains, shot-major (runs of one pass length side
    by side: they step in one lockstep chain), dealt round-robin as folds_of_rank deals folds: every pair exactly once over
    the job, nothing exchanged.  An empty `shots` / `folds` means the one --shot / --fold."""
    sh = [int(v) for v in shots.split(",") if v.strip() != ""] or [int(shot)]
    fo = [int(v) for v in folds.split(",") if v.strip() != ""] or [int(fold)]
    assert len(set(sh)) == len(sh), "--shots: a shot count named twice"
    assert len(set(fo)) == len(fo), "--folds: a fold named twice"
    pairs = [(s_, f_) for s_ in sh for f_ in fo]
    return pairs[rank::world]


def run_result_dir(args, shot: int):
    """Where run (shot, fold) of this command writes: --result_dir itself for --folds alone, {result_dir}/{shot}_shot with
    --shots (what --summary reads)."""
    return os.path.join(args.result_dir, f"{shot}_shot") if getattr(args, "shots", "") else args.result_dir


# ------------------------------------------------------------------ what the grid drivers share (cli_folds, cli_hgrid, cli_optgrid, cli_bankgrid)
def grid_device():
    """The GPU of this process, made current: under a launcher the rank's own, else the current one."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")) if world > 1 else torch.cuda.current_device())
    torch.cuda.set_device(device)
    return device


def task_shape(args):
    """(classes, bytes per stored bag element) of the command's task, from the command line and the label table alone."""
    return _synthetic_classes(args) if args.synthetic else len(_label_map(args)), 2 if args.bag_dtype in ("bf16", "fp16") else 4


def fold_footprints(args, folds):
    """{fold: split_footprints of (--shot, fold)}: what a grid whose cells share the splits of a fold holds once per fold."""
    out = {}
    for fold in folds:
        a = copy.copy(args)
        a.fold = fold
        out[fold] = split_footprints(a)
    return out


def refuse_unless_fits(what, need, device, advice=lambda free: ": name fewer folds"):
    """The refusal before a bag is loaded: `need` (grid_bytes of the largest block) against the device's free memory."""
    free = torch.cuda.mem_get_info(device)[0]
    if need > free:
        raise SystemExit(f"{what} needs about {need / 2**30:.1f} GiB of device memory, {free / 2**30:.1f} GiB are free{advice(free)}")


def grid_blocks(n_items, runs_per_item, max_runs, too_many):
    """`n_items` things of `runs_per_item` runs each cut into blocks trained one after the other: whole items, as many as fit
    `max_runs` runs.  One item that does not fit is refused with `too_many`.  -> list of lists of item indices.  Pure."""
    if runs_per_item > max_runs:
        raise SystemExit(too_many)
    per = max(1, max_runs // runs_per_item)
    return [list(range(i, min(i + per, n_items))) for i in range(0, n_items, per)]


def grid_runs(args, cells, folds, of_cell):
    """The runs' namespaces: a copy of `args` per (cell, fold) with `of_cell(cell)`'s attributes (its result_dir among them),
    cells in the given order, fold-major inside one (the runs of a lockstep chain are consecutive)."""
    out = []
    for cell in cells:
        for fold in folds:
            a = copy.copy(args)
            a.fold = fold
            vars(a).update(of_cell(cell))
            out.append(a)
    return out


def build_run(seed, device, lr, weight_decay):
    """-> (meta-learner, its Adam, the run's mask generator): exactly what the run's own single command does with the default
    generator -- seed (with None the stream goes on from wherever it is, as it does without --seed), build the meta-learner,
    and the masks follow from wherever that leaves the stream -- here in a generator of the run's own.  The ORDER is the
    point: the generator takes the state the constructor left behind, so runs built from one seed start from equal
    parameters AND equal generator states; they draw the same masks, which is what lets the cells of a fold share a score
    pass per epoch (moc_amd.runs)."""
    if seed is not None:
        torch.manual_seed(seed)
    model = M.senet(FEATURE_DIM, 4).to(device)
    g = torch.Generator()
    g.set_state(torch.get_rng_state())
    return model, torch.optim.Adam(model.parameters(), lr=lr, weight_decay=weight_decay), g


def resident_splits(a, device, share, share_train, what):
    """prepare() for a run of a grid: lockstep training and the batched evaluations take resident splits only."""
    loaders = prepare(a, device, share=share, share_train=share_train)
    assert all(isinstance(ld, M.ResidentBags) for ld in loaders), f"{what} needs resident splits (--resident 1)"
    return loaders


def train_blocks(blocks, device, what, build, share_train=True, per_run_adam=False):
    """main_runs over every block (a list of run namespaces), one block after the other: per run its splits, THEN the run
    itself (`build(a)` -> build_run's triple; the single command prepares before it seeds, too).  One `share` dict serves
    all blocks: a split that any earlier run named is held once.  -> the result dicts in run order."""
    out, share = [], {}
    for args_list in blocks:
        models, optimizers, loaders_list, gens = [], [], [], []
        for a in args_list:
            loaders_list.append(resident_splits(a, device, share, share_train, what))
            model, optimizer, g = build(a)
            models.append(model)
            optimizers.append(optimizer)
            gens.append(g)
        out += main_runs(args_list, models, optimizers, loaders_list, device, generators=gens, per_run_adam=per_run_adam)
    return out


def cli_folds(args):
    """`--folds a,b,...` and / or `--shots a,b,...`: those runs in this process (under a launcher: this rank's share of
    them, nothing exchanged)."""
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    pairs = pairs_of_rank(getattr(args, "shots", ""), args.folds, args.shot, args.fold, rank, world)     # (shot, fold) pairs are what is dealt
    device = grid_device()
    if not pairs:
        print(f"rank {rank}: no fold to train")
        return []
    assert not args.loader_seed_draw, "--folds: the runs draw their masks from private generators (no DataLoader base-seed draw)"
    from . import runs as RUNS
    if len(pairs) > RUNS.MAX_RUNS:      # one block: runs of different shot counts share nothing that a cut could keep together
        raise SystemExit(f"--shots x --folds: {len(pairs)} runs in one process, at most {RUNS.MAX_RUNS}")
    args_list = []
    for shot, fold in pairs:
        a = copy.copy(args)
        a.fold, a.shot = fold, shot
        a.result_dir = run_result_dir(args, shot)
        args_list.append(a)
    if getattr(args, "shots", ""):
        # only with --shots: plain --folds is the reference launcher's handful of folds of one shot and has never been sized; a
        # grid grows with its shot counts, and since its runs stand alone the refusal can name the leading part that fits
        C_, itemsize = task_shape(args)
        fps = [split_footprints(a) for a in args_list]          # (splits that two runs share count once)

        def leading_part(free):
            k = largest_grid(fps, FEATURE_DIM, itemsize, C_, free)
            return f".  The largest leading part of it that fits is {k} run(s): {pairs[:k]}"
        refuse_unless_fits("--shots x --folds: this grid", grid_bytes(fps, FEATURE_DIM, itemsize, C_), device, leading_part)
    # share_train stays off: no two (shot, fold) pairs have the same train split, only validation and test splits recur
    return train_blocks([args_list], device, "--folds", share_train=False,
                        build=lambda a: build_run(args.seed, device, lr=args.lr, weight_decay=args.weight_decay))


# ------------------------------------------------------------------ hyper-parameter grids (--topjs / --topks / --discard_sets)
def hgrid_discard_name(d):
    return "+".join(d) if d else "none"


def hgrid_requested(args):
    return any(getattr(args, n, None) is not None for n in ("topjs", "topks", "discard_sets"))


def hgrid_configs(args):
    """[(topj, topk, discard tuple)] of --topjs x --topks x --discard_sets in the given order (topj-major, the discard set
    innermost); a list that is not given is the one --topj / --topk / --discard_classifiers.  The lists are parsed by
    moc_amd.sweep's parsers (the same spellings); an empty or malformed one is refused."""
    from .sweep import _int_list, parse_discard_set

    def parsed(flag, fn, text):
        try:
            return fn(text)
        except argparse.ArgumentTypeError as e:
            raise SystemExit(f"{flag}: {e}")
    js = [int(args.topj)] if args.topjs is None else parsed("--topjs", _int_list, args.topjs)
    ks = [int(args.topk)] if args.topks is None else parsed("--topks", _int_list, args.topks)
    if args.discard_sets is None:
        ds = [tuple(args.discard_classifiers or ())]
    else:
        if len(args.discard_sets) == 0:
            raise SystemExit("--discard_sets: an empty list -- name at least one set (`none` is the empty set)")
        ds = [parsed("--discard_sets", parse_discard_set, t) for t in args.discard_sets]
    for flag, vals in (("--topjs", js), ("--topks", ks), ("--discard_sets", ds)):
        if len(set(vals)) != len(vals):
            raise SystemExit(f"{flag}: a value named twice")
    return [(j, k, d) for j in js for k in ks for d in ds]


def hgrid_dir(result_dir, cfg):
    """Where the runs of configuration (topj, topk, discard) write: {result_dir}/topj{J}_topk{K}_{set}."""
    return os.path.join(result_dir, f"topj{cfg[0]}_topk{cfg[1]}_{hgrid_discard_name(cfg[2])}")


def check_hgrid_args(args):
    """Refusals of a hyper-parameter grid, from the command line alone (before any bag is loaded)."""
    if not hgrid_requested(args):
        return
    if getattr(args, "shots", ""):
        raise SystemExit("--topjs / --topks / --discard_sets do not combine with --shots: one --shot per grid")
    if patch_map_splits(args) or args.patch_maps_from:
        raise SystemExit("--topjs / --topks / --discard_sets do not combine with --patch_maps / --patch_maps_from: run one configuration at a time")
    if args.loader_seed_draw:
        raise SystemExit("--topjs / --topks / --discard_sets do not combine with --loader_seed_draw: the runs draw their masks from "
                         "private generators (no DataLoader base-seed draw)")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 and args.seed is None:
        raise SystemExit("--topjs / --topks / --discard_sets under a launcher need --seed: every rank must build the same meta-learners")
    if args.ablation_study != "none":
        raise SystemExit("--topjs / --topks / --discard_sets train the meta-learner: the ablation study trains none")
    hgrid_configs(args)


def hgrid_blocks(n_configs, n_folds, max_runs):
    """The configurations cut into blocks trained one after the other: whole configurations, as many as fit `max_runs` runs
    (a configuration is n_folds runs).  -> list of lists of configuration indices.  Pure."""
    return grid_blocks(n_configs, n_folds, max_runs, f"--folds: {n_folds} folds in one process, at most {max_runs}")


def hgrid_runs(args, configs, folds):
    """The runs' namespaces: configurations in the given order, fold-major inside one (grid_runs)."""
    return grid_runs(args, configs, folds, lambda cfg: dict(topj=cfg[0], topk=cfg[1], discard_classifiers=list(cfg[2]),
                                                            result_dir=hgrid_dir(args.result_dir, cfg)))


def cells_block_bytes(args, n_cells, folds):
    """grid_bytes of a block of `n_cells` cells x `folds` whose cells share the splits of a fold: those count once."""
    C_, itemsize = task_shape(args)
    fps = fold_footprints(args, folds)
    return grid_bytes([fps[f] for _ in range(n_cells) for f in folds], FEATURE_DIM, itemsize, C_)


def cli_hgrid(args):
    """`--topjs / --topks / --discard_sets` (with --folds or the one --fold): every (configuration, fold) run in this process.
    Under a launcher the configurations are dealt to the ranks, nothing exchanged."""
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    configs = hgrid_configs(args)[rank::world]      # whole configurations are what is dealt: a rank keeps every fold's shared score pass
    folds = folds_of_rank(args.folds, 0, 1) if args.folds else [int(args.fold)]
    device = grid_device()
    if not configs:
        print(f"rank {rank}: no configuration to train")
        return []
    from . import runs as RUNS
    blocks = hgrid_blocks(len(configs), len(folds), RUNS.MAX_RUNS)
    refuse_unless_fits(f"--topjs x --topks x --discard_sets: a block of {len(blocks[0])} configuration(s) x {len(folds)} fold(s)",
                       cells_block_bytes(args, len(blocks[0]), folds), device)
    # evaluation_runs' plan belongs to one (topj, topk, discard set), so main_runs evaluates configuration by configuration: a
    # plan per configuration of a block and kind of pass (train + val, and two sets of improved runs' test splits)
    M.EVAL_RUN_PLANS = max(M.EVAL_RUN_PLANS, 3 * len(blocks[0]))
    # (train_blocks' one `share` across the blocks: every block names the same folds, whose splits are loaded once)
    return train_blocks([hgrid_runs(args, [configs[i] for i in block], folds) for block in blocks], device, "a hyper-parameter grid",
                        build=lambda a: build_run(args.seed, device, lr=args.lr, weight_decay=args.weight_decay))


# ------------------------------------------------------------------ optimizer grids (--seeds / --lrs / --wds)
OPT_GRID_FLAGS = "--seeds / --lrs / --wds"


def optgrid_requested(args):
    return any(getattr(args, n, None) is not None for n in ("seeds", "lrs", "wds"))


def _number_list(flag, text, kind):
    try:
        out = [kind(v) for v in str(text).split(",") if v.strip() != ""]
    except ValueError:
        raise SystemExit(f"{flag}: not a comma-separated list of numbers: {text!r}")
    if not out:
        raise SystemExit(f"{flag}: a non-empty list is needed, got {text!r}")
    if len(set(out)) != len(out):
        raise SystemExit(f"{flag}: a value named twice")
    return out


def optgrid_cells(args):
    """[(seed, lr, weight_decay)] of --seeds x --lrs x --wds, seed-major, then lr, the weight decay innermost; a list that
    is not given is the one --seed / --lr / --weight_decay.  An empty or malformed list, a value named twice, a negative or
    non-finite rate and a grid without any seed are refused."""
    if args.seeds is None and args.seed is None:
        raise SystemExit("--lrs / --wds need --seed or --seeds: the cells of a fold start from one meta-learner and one mask stream")
    seeds = [int(args.seed)] if args.seeds is None else _number_list("--seeds", args.seeds, int)
    lrs = [float(args.lr)] if args.lrs is None else _number_list("--lrs", args.lrs, float)
    wds = [float(args.weight_decay)] if args.wds is None else _number_list("--wds", args.wds, float)
    for flag, vals in (("--lrs", lrs), ("--wds", wds)):
        if not all(np.isfinite(v) and v >= 0 for v in vals):
            raise SystemExit(f"{flag}: finite values >= 0 are needed, got {vals}")
    return [(s_, lr, wd) for s_ in seeds for lr in lrs for wd in wds]


def optgrid_dir(result_dir, cell):
    """Where the runs of cell (seed, lr, weight_decay) write: {result_dir}/seed{S}_lr{LR}_wd{WD}, the numbers as format(x, "g")."""
    return os.path.join(result_dir, f"seed{cell[0]}_lr{format(cell[1], 'g')}_wd{format(cell[2], 'g')}")


def check_optgrid_args(args):
    """Refusals of an optimizer grid, from the command line alone (before any bag is loaded)."""
    if not optgrid_requested(args):
        return
    if getattr(args, "shots", ""):
        raise SystemExit(f"{OPT_GRID_FLAGS} do not combine with --shots: one --shot per grid")
    if hgrid_requested(args):
        raise SystemExit(f"{OPT_GRID_FLAGS} do not combine with --topjs / --topks / --discard_sets: one grid per command")
    if patch_map_splits(args) or args.patch_maps_from:
        raise SystemExit(f"{OPT_GRID_FLAGS} do not combine with --patch_maps / --patch_maps_from: run one cell at a time")
    if args.loader_seed_draw:
        raise SystemExit(f"{OPT_GRID_FLAGS} do not combine with --loader_seed_draw: the runs draw their masks from private "
                         "generators (no DataLoader base-seed draw)")
    if args.ablation_study != "none":
        raise SystemExit(f"{OPT_GRID_FLAGS} do not combine with --ablation_study: the grid trains the meta-learner, the ablation "
                         "study trains none")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit(f"{OPT_GRID_FLAGS} are one-GPU options (WORLD_SIZE > 1): run the grid without a launcher")
    optgrid_cells(args)


def optgrid_runs(args, cells, folds):
    """The runs' namespaces: cells in the given order, fold-major inside one (grid_runs)."""
    return grid_runs(args, cells, folds, lambda cell: dict(seed=cell[0], lr=cell[1], weight_decay=cell[2],
                                                           result_dir=optgrid_dir(args.result_dir, cell)))


def summary_row(result_dirs_and_folds, shot):
    """The columns the grids' summaries share: the number of runs and the mean and population standard deviation over them of
    the best validation AUC and of the test AUC at it, read from the runs' best_results_* files (`best_val`,
    `test_at_best_val`: the keys --summary reads them by)."""
    vals = []
    for result_dir, fold in result_dirs_and_folds:
        with open(os.path.join(result_dir, f"best_results_shot_{shot}_fold_{fold}.json")) as f:
            r = json.load(f)
        vals.append((r["best_val"], r["test_at_best_val"]))
    v = np.asarray(vals, dtype=np.float64)
    return {"runs": len(vals), "best_val_mean": v[:, 0].mean(), "best_val_std": v[:, 0].std(),
            "test_auc_mean": v[:, 1].mean(), "test_auc_std": v[:, 1].std()}


def write_optgrid_summary(result_dir, cells, folds, shot):
    """{result_dir}/opt_grid_summary.csv: one line per (lr, weight_decay) in order of first appearance over its runs (seeds x
    folds, seed-major): summary_row's columns.  -> path."""
    by_hp = {}
    for cell in cells:
        by_hp.setdefault((cell[1], cell[2]), []).extend((optgrid_dir(result_dir, cell), fold) for fold in folds)
    rows = [{"lr": format(lr, "g"), "weight_decay": format(wd, "g"), **summary_row(runs, shot)} for (lr, wd), runs in by_hp.items()]
    path = os.path.join(result_dir, "opt_grid_summary.csv")
    pd.DataFrame(rows).to_csv(path, index=False)        # (no float_format: pandas' shortest round-trip text, as this file has always had)
    return path


def cli_optgrid(args):
    """`--seeds / --lrs / --wds` (with --folds or the one --fold): every (cell, fold) run in this process."""
    cells = optgrid_cells(args)
    folds = folds_of_rank(args.folds, 0, 1) if args.folds else [int(args.fold)]
    device = grid_device()      # one GPU: check_optgrid_args refuses a launcher (the cells of a fold step in ONE chain)
    from . import runs as RUNS
    blocks = hgrid_blocks(len(cells), len(folds), RUNS.MAX_RUNS)
    refuse_unless_fits(f"--seeds x --lrs x --wds: a block of {len(blocks[0])} cell(s) x {len(folds)} fold(s)",
                       cells_block_bytes(args, len(blocks[0]), folds), device)
    # every run is seeded with ITS cell's seed and steps with ITS cell's rates (per_run_adam): the (lr, wd) cells of a (seed, fold)
    # start from equal parameters and equal generator states and share their masks
    out = train_blocks([optgrid_runs(args, [cells[i] for i in block], folds) for block in blocks], device, "an optimizer grid",
                       build=lambda a: build_run(a.seed, device, lr=a.lr, weight_decay=a.weight_decay), per_run_adam=True)
    print("optimizer grid summary:", write_optgrid_summary(args.result_dir, cells, folds, args.shot))
    return out


# ------------------------------------------------------------------ bank grids (--banks)
def bankgrid_requested(args):
    return getattr(args, "banks", None) is not None


def bankgrid_dir(result_dir, name):
    """Where the runs under bank NAME write: {result_dir}/bank_{NAME}."""
    return os.path.join(result_dir, f"bank_{name}")


def check_bankgrid_args(args):
    """Refusals of a bank grid, from the command line and the banks' files alone (before any bag is loaded) -> [(name, W,
    W_ext)] host tensors, or None without --banks."""
    if not bankgrid_requested(args):
        return None
    if args.seed is None:
        raise SystemExit("--banks needs --seed: the banks' runs of a fold start from one meta-learner and one mask stream")
    if getattr(args, "shots", ""):
        raise SystemExit("--banks does not combine with --shots: one --shot per grid")
    if hgrid_requested(args):
        raise SystemExit("--banks does not combine with --topjs / --topks / --discard_sets: one grid per command")
    if optgrid_requested(args):
        raise SystemExit(f"--banks does not combine with {OPT_GRID_FLAGS}: one grid per command")
    if patch_map_splits(args) or args.patch_maps_from:
        raise SystemExit("--banks does not combine with --patch_maps / --patch_maps_from: run one bank at a time")
    if args.loader_seed_draw:
        raise SystemExit("--banks does not combine with --loader_seed_draw: the runs draw their masks from private generators "
                         "(no DataLoader base-seed draw)")
    if args.cache_scores:
        raise SystemExit("--banks does not combine with --cache_scores: a score cache belongs to one bank")
    if args.ablation_study != "none":
        raise SystemExit("--banks trains the meta-learner: the ablation study trains none")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("--banks is a one-GPU option (WORLD_SIZE > 1): run the grid without a launcher")
    from .sweep import check_bank_names, load_bank_files
    check_bank_names(args.banks)
    return load_bank_files(args.banks, wide="a bank grid takes banks of at most {ce} (wide banks: one run_moc per bank)",
                           mixed="run one grid per class count")


def bankgrid_blocks(n_banks, n_folds, max_runs):
    """The folds cut into blocks trained one after the other: whole folds -- a fold's banks stay together, they share the
    score pass -- as many as fit `max_runs` runs (a fold is n_banks runs).  -> list of lists of fold positions.  Pure."""
    return grid_blocks(n_folds, n_banks, max_runs, f"--banks: {n_banks} banks in one process, at most {max_runs}")


def bankgrid_runs(args, names, folds):
    """The runs' namespaces, bank-major (the leaders of the folds are consecutive runs: one score launch serves them all),
    the folds inside a bank in the given order (grid_runs)."""
    return grid_runs(args, names, folds, lambda name: dict(bank=name, result_dir=bankgrid_dir(args.result_dir, name)))


def bankgrid_bytes(fold_footprints, D, itemsize, C, n_banks):
    """grid_bytes of n_banks runs per fold: the splits of a fold once, the work arrays -- per bank -- n_banks times."""
    from . import engine
    assert engine.bank_work_row_bytes(C) == 4 * (2 * C + 3) + 4 * (2 * C + 2) + 13 + 4 * C     # (grid_bytes' evaluation row)
    return grid_bytes([fp for _ in range(n_banks) for fp in fold_footprints], D, itemsize, C)


def write_bankgrid_summary(result_dir, names, folds, shot):
    """{result_dir}/bank_grid_summary.csv: one line per bank in the given order over its runs (the folds): summary_row's
    columns.  -> path."""
    rows = [{"bank": name, **summary_row([(bankgrid_dir(result_dir, name), fold) for fold in folds], shot)} for name in names]
    path = os.path.join(result_dir, "bank_grid_summary.csv")
    pd.DataFrame(rows).to_csv(path, index=False, float_format="%.17g")      # (moc_amd.sweep's bank_summary.csv format: the two tables are read side by side)
    return path


def main_banks(args_list, names, folds, models, optimizers, loaders_of_fold, device, generators, banks):
    """main() for the runs of a bank grid, bank-major (run g * len(folds) + i: bank g, fold folds[i]): the zero-shot numbers of
    all banks from one read of every split (zs_evaluation_banks), the training passes in one TrainRuns with one multi-bank score
    pass per mask group, and per epoch, fold and split one evaluation_banks over the models of that fold -- train and validation
    always, test for the banks whose validation AUC improved.  Every run prints (behind a [bank NAME] tag), saves and returns
    what main() does for it alone with its bank installed.  -> list of result dicts, in run order."""
    G, F = len(names), len(folds)
    run = lambda g, i: g * F + i
    a0 = args_list[0]
    books = [ResultBook(a, prefix=f"[bank {a.bank}] [fold {a.fold}] ") for a in args_list]
    if a0.check_zeroshot:
        for i in range(F):      # fold-major: one zs_evaluation_banks per split of a fold gives every bank's numbers
            zs = [M.zs_evaluation_banks(ld, device, a0, banks) for ld in loaders_of_fold[i]]
            for g in range(G):
                books[run(g, i)].zero_shot(zs[0][g], zs[1][g], zs[2][g])
    trains = [loaders_of_fold[i][0] for _ in range(G) for i in range(F)]
    of_run = [g for g in range(G) for _ in range(F)]
    for epoch in range(getattr(a0, "epochs", 25)):
        print("Epoch: ", epoch)
        M.train_runs(models, trains, optimizers, device, a0, generators=generators, banks=banks, bank_of_run=of_run)
        for i in range(F):
            tr, va, te = loaders_of_fold[i]
            ms = [models[run(g, i)] for g in range(G)]
            ev_tr = M.evaluation_banks(ms, tr, device, a0, banks)
            ev_va = M.evaluation_banks(ms, va, device, a0, banks)
            better = [g for g in range(G) if books[run(g, i)].improves(ev_va[g])]
            ev_te = dict(zip(better, M.evaluation_banks([ms[g] for g in better], te, device, a0, [banks[g] for g in better]))) if better else {}
            for g in range(G):
                books[run(g, i)].epoch(epoch, ms[g], ev_tr[g], ev_va[g], ev_te.get(g))
    out = [book.close() for book in books]
    print("\nEnd training.")
    return out


def cli_bankgrid(args, bank_files):
    """`--banks` (with --folds or the one --fold): every (bank, fold) run in this process."""
    names = [n for n, _, _ in bank_files]
    folds = folds_of_rank(args.folds, 0, 1) if args.folds else [int(args.fold)]
    C_, itemsize = task_shape(args)
    for name, W, _ in bank_files:
        if W.size(1) != C_ or W.size(0) != FEATURE_DIM:
            raise SystemExit(f"--banks: {name}: W is [{W.size(0)}, {W.size(1)}]; this task needs [{FEATURE_DIM}, {C_}]")
    device = grid_device()      # one GPU: check_bankgrid_args refuses a launcher
    from . import runs as RUNS
    # whole FOLDS per block, not whole banks as the other grids cut whole cells: a fold's banks share the score pass
    blocks = bankgrid_blocks(len(names), len(folds), RUNS.MAX_RUNS)
    fps = fold_footprints(args, folds)
    refuse_unless_fits(f"--banks: a block of {len(names)} bank(s) x {len(blocks[0])} fold(s)",
                       bankgrid_bytes([fps[folds[i]] for i in blocks[0]], FEATURE_DIM, itemsize, C_, len(names)), device)
    banks = [(W.to(device), We.to(device)) for _, W, We in bank_files]
    adam = {"lr": args.lr, "weight_decay": args.weight_decay}
    out = {}
    # The block loop stands here and not in train_blocks: the splits belong to a fold, not to a run (prepare() also installs
    # and prints a classifier bank, so it runs once per fold, not once per run), and the block goes to main_banks.
    for block in blocks:
        fs = [folds[i] for i in block]
        args_list = bankgrid_runs(args, names, fs)
        share = {}              # fresh per block: the blocks name different folds, so nothing recurs and the last block's splits can go
        loaders_of_fold = [resident_splits(a, device, share, True, "a bank grid") for a in args_list[:len(fs)]]
        models, optimizers, gens = [], [], []
        for a in args_list:
            a.n_classes = args_list[0].n_classes        # (prepare() left it on the first bank's namespaces only)
            # every bank's run of a fold is seeded with --seed: equal parameters, equal generator states, shared masks
            model, optimizer, g = build_run(args.seed, device, **adam)
            models.append(model)
            optimizers.append(optimizer)
            gens.append(g)
        res = main_banks(args_list, names, fs, models, optimizers, loaders_of_fold, device, gens, banks)
        for a, r in zip(args_list, res):
            out[(a.bank, a.fold)] = r
    print("bank grid summary:", write_bankgrid_summary(args.result_dir, names, folds, args.shot))
    return [out[(n, f)] for n in names for f in folds]         # bank-major over ALL folds, whatever the blocks were


def cli(argv=None):
    args = get_args(argv)
    if args.summary:
        summary(args)
        return None
    bank_files = check_bankgrid_args(args)
    check_optgrid_args(args)
    check_hgrid_args(args)
    check_patch_map_args(args)
    if not torch.cuda.is_available():
        raise RuntimeError("moc_amd needs a GPU: there is no CPU fallback")
    if bank_files is not None:
        return cli_bankgrid(args, bank_files)
    if optgrid_requested(args):
        return cli_optgrid(args)
    if hgrid_requested(args):
        return cli_hgrid(args)
    if args.folds or args.shots:
        return cli_folds(args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:                                   # one process per GPU under a launcher (torch.distributed.run)
        import torch.distributed as dist
        # everything that can be refused from the command line alone is refused HERE, on every rank alike, before the
        # process group exists: a rank that leaves later would strand its peers inside a collective
        if args.seed is None:
            raise SystemExit("multi-GPU runs need --seed: every rank must build the same meta-learner and draw the same masks")
        if args.loader_seed_draw:
            raise SystemExit("--loader_seed_draw is a one-GPU option: the sharded splits do not make the DataLoader's per-pass "
                             "base-seed draw, so the mask stream would differ from the same command on one GPU")
        if args.synthetic and world > args.shot * (2 if args.dataset == "nsclc" else 3 if args.dataset == "rcc" else 12 if args.dataset == "ebrains12" else 30):
            raise SystemExit(f"the train split has fewer slides than the job has ranks ({world}): every rank must hold at least one")
        # (RCCL sets up its own IPC; this script maps no peer memory by hand and leaves HSA_ENABLE_IPC_MODE_LEGACY as the
        # launcher's environment has it)
        device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
        torch.cuda.set_device(device)
        dist.init_process_group("nccl", device_id=device)
    else:
        device = torch.device("cuda")
    train_loader, val_loader, test_loader = prepare(args, device)
    if args.seed is not None:
        torch.manual_seed(args.seed)
    model = M.senet(FEATURE_DIM, 4).to(device)                                                   # main_moc.py:315
    optimizer = torch.optim.Adam(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)   # main_moc.py:316 (1e-3, 1e-4)
    loaders = (train_loader, val_loader, test_loader)
    if args.patch_maps_from:
        return patch_maps_from(args, model, loaders, device)
    try:
        res = main(args, model, optimizer, train_loader, val_loader, test_loader, device)
        if patch_map_splits(args):        # the best checkpoint, or the final model when none was written
            if os.path.exists(res["best_model_path"]):
                model.load_state_dict(torch.load(res["best_model_path"], map_location="cpu"))
            write_split_maps(args, model, loaders, device)
        return res
    finally:
        if world > 1:
            import torch.distributed as dist
            mdist.shutdown()
            dist.destroy_process_group()


if __name__ == "__main__":
    cli()
