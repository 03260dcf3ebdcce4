#!/usr/bin/env python3
"""A bank grid -- G = 4 prompt banks of Ce = 6 x five NSCLC-16-shaped folds (32 slides x 15,000 x 512 each) -- trained in one
TrainRuns against the ways it replaces:
    python scripts/bench_bankgrid.py [dtype fp32|bf16] [which: all|grid|unfused|successive] [slides] [rows] [timed passes]
  (1) one TrainRuns(banks=...) over the 20 runs: five mask groups, one moc_scores_banks launch per pass of the bank set over
      the five leaders' slides, the statistics written straight into every run's slots;
  (2) the same with MOC_RUNS_BANKS_FUSED=0: one moc_scores launch per (fold, bank) over that run's slides;
  (3) G successive five-fold TrainRuns, each after set_classifier_bank of its bank: what a tree without bank grids does.  To
      time (3) with ANOTHER tree's package and library (the parent commit's, built), name its root in MOC_BENCH_TREE:
          MOC_BENCH_TREE=/path/to/parent python scripts/bench_bankgrid.py fp32 successive
Host clock around train_pass with a final synchronize; three untimed passes, then ten timed ones; one line per way:
ms per pass of all 20 runs and meta-steps/s = runs x slides x passes / s."""
import os, sys, time, types
ROOT = os.environ.get("MOC_BENCH_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
torch.set_num_threads(8)
from moc_amd import main_moc as M, synth
from moc_amd.runs import TrainRuns

dt = {"fp32": torch.float32, "bf16": torch.bfloat16}[sys.argv[1] if len(sys.argv) > 1 else "fp32"]
which = sys.argv[2] if len(sys.argv) > 2 else "all"
n = int(sys.argv[3]) if len(sys.argv) > 3 else 32
rows = int(sys.argv[4]) if len(sys.argv) > 4 else 15000
assert which in ("all", "grid", "unfused", "successive")
WARM, PASSES = 3, int(sys.argv[5]) if len(sys.argv) > 5 else 10       # (one timed pass: under rocprofv3 --kernel-trace --stats)
dev = torch.device("cuda:0")
C, D, G, FOLDS, CE = 2, 512, 4, 5, 6
banks = [tuple(t.to(dev) for t in synth.make_bank(1234 + g, D, C, n_bg=CE - C)) for g in range(G)]
splits = []
for f in range(FOLDS):
    bags = [synth.make_bag_device(777 + 1000 * f + i, rows, D, banks[0][1].cpu(), C, i % C, dev, dt) for i in range(n)]
    splits.append(M.ResidentBags(bags, [i % C for i in range(n)], dev))
    del bags
args = types.SimpleNamespace(disable_tqdm=True, n_classes=C, topj=400, topk=10, discard_classifiers=[], pretrain="conch",
                             ablation_study="none")


def runs_of(n_banks):
    """Bank-major: (models, optimizers, splits, generators, bank of every run)."""
    models, opts, sps, gens, of_run = [], [], [], [], []
    for g in range(n_banks):
        for f in range(FOLDS):
            torch.manual_seed(100 + f)
            m = M.senet(D, 4).to(dev)
            models.append(m)
            opts.append(torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-4))
            sps.append(splits[f])
            gens.append(torch.Generator().manual_seed(7000 + f))
            of_run.append(g)
    return models, opts, sps, gens, of_run


def timed(what, one_pass):
    for _ in range(WARM):
        one_pass()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(PASSES):
        one_pass()
    torch.cuda.synchronize()
    s = (time.perf_counter() - t0) / PASSES
    rate = G * FOLDS * n / s
    print(f"{what}: {s * 1e3:.3f} ms per pass of {G * FOLDS} runs, {rate / 1e3:.1f} k meta-steps/s", flush=True)
    return rate


print(f"shape: {FOLDS} folds of {n} slides x {rows} x {D} {dt}, {G} banks of Ce = {CE}, C = {C}; tree {ROOT}", flush=True)
res = {}
for name, fused in (("grid", "1"), ("unfused", "0")):
    if which in ("all", name):
        os.environ["MOC_RUNS_BANKS_FUSED"] = fused
        models, opts, sps, gens, of_run = runs_of(G)
        rs = TrainRuns(models, opts, sps, dev, args, generators=gens, banks=banks, bank_of_run=of_run)
        res[name] = timed("(1) one grid, one multi-bank score pass  " if fused == "1" else "(2) one grid, a score launch per bank    ", rs.train_pass)
        print(f"    chains {[g_['runs'].n_runs for g_ in rs.groups]}, phase A {rs.trained_phase_a}", flush=True)
        del rs, models, opts
if which in ("all", "successive"):
    sets = []
    for g in range(G):
        M.set_classifier_bank(*banks[g])
        models, opts, sps, gens, _ = runs_of(1)
        sets.append(TrainRuns(models, opts, sps, dev, args, generators=gens))      # (the bank's image is taken at construction)

    def in_turn():
        for rs_ in sets:
            rs_.train_pass()
    res["successive"] = timed("(3) G five-fold TrainRuns in turn        ", in_turn)
if "grid" in res:
    print("   ".join(f"(1)/{k} = {res['grid'] / v:.2f}" for k, v in res.items() if k != "grid"), flush=True)
