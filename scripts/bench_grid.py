"""Wall time per epoch of a folds (x shots) grid trained in one process: the training pass (main_moc.train_runs) and the
evaluation block behind it, timed separately with the host clock and one torch.cuda.synchronize() each.

    python scripts/bench_grid.py --shots 16 --folds 5                    # five 16-shot folds at the NSCLC-16 shape
    python scripts/bench_grid.py --shots 1,2,4,8,16 --folds 5            # the whole grid
    python scripts/bench_grid.py --shots 1,2,4,8,16 --folds 5 --per_shot # ... as five --folds commands one after the other

The bags are random rows generated on the device (train splits of `2 x shot` slides, 49 validation and 202
test slides of 15,000 x 512 per fold; the validation / test splits of a fold are shared by its shot counts, as on RCC).
The epoch is run_moc.main_runs': the training pass, the train and validation split of every run, then the test split of
the runs whose validation AUC "improved" -- here a fixed pseudo-random schedule (`improved`): every run in the first epoch,
then a set that changes from epoch to epoch and thins out (85 %, 70 %, ... never below 10 % of the runs), as best-so-far
bookkeeping does; the same sets whatever tree runs the script.  `--test_every_epoch`: every run's test split every epoch.
Works on trees without main_moc.evaluation_runs too (then the evaluations run per run, as run_moc.main_runs did): the
same script measures the commit before and after.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from moc_amd import main_moc as M, synth  # noqa: E402
from moc_amd.runs import TrainRuns  # noqa: E402


def split(dev, seed, n, rows, D, dtype, repeat=None):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    bags = [torch.randn((rows, D), generator=g, device=dev, dtype=torch.float32).to(dtype) for _ in range(n)]
    return M.ResidentBags(bags, [i % 2 for i in range(n)], dev, dtype=dtype, repeat_num=repeat)


def improved(e, r, always):
    """Whether run r's validation AUC improves in epoch e (a schedule, not a measurement)."""
    if always or e == 0:
        return True
    return ((r * 2654435761 + e * 40503) >> 7) % 100 < max(10, 100 - 15 * e)


def epoch(e, always, models, opts, loaders, gens, rs, dev, args, one_pass):
    R = len(models)
    better = [r for r in range(R) if improved(e, rs_base(rs) + r, always)]
    trains = [ls[0] for ls in loaders]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if rs[0] is None:                                 # (kept by the caller: main_moc.train_runs caches only a few sets)
        rs[0] = TrainRuns(models, opts, trains, dev, args, generators=gens)
    rs[0].train_pass()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    if one_pass:
        M.evaluation_runs(list(models) + list(models), trains + [ls[1] for ls in loaders], dev, args)
        if better:
            M.evaluation_runs([models[r] for r in better], [loaders[r][2] for r in better], dev, args)
    else:
        for r in range(R):
            for ld in loaders[r][:2] + ((loaders[r][2],) if r in better else ()):
                M.evaluation(models[r], ld, dev, args)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1


def rs_base(rs):
    """The position of a set's first run in the whole grid (a --per_shot set is a slice of it): rs[1] when given."""
    return rs[1] if len(rs) > 1 else 0


def grid(dev, shots, folds, a, shared, base=0):
    models, opts, loaders, gens = [], [], [], []
    for shot in shots:
        for fold in range(folds):
            key = fold
            if key not in shared:
                shared[key] = (split(dev, 5000 + fold, a.val, a.rows, 512, a.dtype), split(dev, 9000 + fold, a.test, a.rows, 512, a.dtype))
            torch.manual_seed(1)
            m = M.senet(512, 4).to(dev)
            g = torch.Generator()
            g.set_state(torch.get_rng_state())
            models.append(m)
            opts.append(torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-4))
            loaders.append((split(dev, 100 + 17 * fold + shot, 2 * shot, a.rows, 512, a.dtype, repeat=2 * shot),) + shared[key])
            gens.append(g)
    return models, opts, loaders, gens, [None, base]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shots", default="16")
    p.add_argument("--folds", type=int, default=5)
    p.add_argument("--rows", type=int, default=15000)
    p.add_argument("--val", type=int, default=49)
    p.add_argument("--test", type=int, default=202)
    p.add_argument("--epochs", type=int, default=10)
    p.add_argument("--test_every_epoch", action="store_true", help="every run's test split every epoch (the upper bound)")
    p.add_argument("--bag_dtype", default="fp32")
    p.add_argument("--per_shot", action="store_true", help="one lockstep set per shot count, one after the other")
    p.add_argument("--per_run_eval", action="store_true", help="evaluate run by run even where evaluation_runs exists")
    a = p.parse_args()
    a.dtype = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[a.bag_dtype]
    dev = torch.device("cuda")
    shots = [int(v) for v in a.shots.split(",")]
    W, We = synth.make_bank(1234, 512, 2)
    M.set_classifier_bank(W.to(dev), We.to(dev))
    args = types.SimpleNamespace(disable_tqdm=True, n_classes=2, topj=400, topk=10, discard_classifiers=[], pretrain="conch",
                                 ablation_study="none")
    one_pass = hasattr(M, "evaluation_runs") and not a.per_run_eval
    shared = {}
    sets = [grid(dev, [s], a.folds, a, shared, base=i * a.folds) for i, s in enumerate(shots)] if a.per_shot \
        else [grid(dev, shots, a.folds, a, shared)]
    times = []
    for e in range(a.epochs + 1):                     # (the first epoch builds the plans and packs the splits: not reported)
        tr = ev = 0.0
        for s in sets:
            t, v = epoch(e, a.test_every_epoch, *s, dev, args, one_pass)
            tr, ev = tr + t, ev + v
        if e:
            times.append({"train_ms": round(tr * 1e3, 2), "eval_ms": round(ev * 1e3, 2), "epoch_ms": round((tr + ev) * 1e3, 2)})
    ep = [t["epoch_ms"] for t in times]
    print(json.dumps({"shots": shots, "folds": a.folds, "runs": len(shots) * a.folds, "per_shot": a.per_shot,
                      "one_pass_eval": one_pass, "test_every_epoch": a.test_every_epoch, "bag_dtype": a.bag_dtype,
                      "epoch_ms_mean": round(sum(ep) / len(ep), 2), "epoch_ms_min": min(ep), "epoch_ms_max": max(ep),
                      "train_ms_mean": round(sum(t["train_ms"] for t in times) / len(times), 2),
                      "eval_ms_mean": round(sum(t["eval_ms"] for t in times) / len(times), 2), "epochs": times}))


if __name__ == "__main__":
    main()
