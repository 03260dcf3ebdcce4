#!/usr/bin/env python3
"""A hyper-parameter grid trained in one TrainRuns against the ways it replaces, on the NSCLC-16 train shape
(32 slides x 15,000 x 512 per fold, five folds):
    python scripts/bench_hgrid.py [dtype fp32|bf16] [slides per fold] [rows]
For H = 4 and H = 6 configurations (H x 5 runs), three ways:
  (1) one TrainRuns over all H x 5 runs, the configurations of a fold sharing one mask draw and one score pass;
  (2) the same with MOC_RUNS_SHARE=0 (every run drawn and scored for itself);
  (3) H successive five-fold TrainRuns, one per configuration, a pass of each after the other.
Host clock around train_pass with a final synchronize; three untimed passes, then ten timed ones; the mean per pass and the
scored slides per pass of each way are printed."""
import os, sys, time, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
torch.set_num_threads(8)
from moc_amd import main_moc as M, synth
from moc_amd.runs import TrainRuns

dt = {"fp32": torch.float32, "bf16": torch.bfloat16}[sys.argv[1] if len(sys.argv) > 1 else "fp32"]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 32
rows = int(sys.argv[3]) if len(sys.argv) > 3 else 15000
FOLDS, WARM, PASSES = 5, 3, 10
dev = torch.device("cuda:0")
C, D = 2, 512
CONFIGS = [(100, 5, ()), (100, 10, ()), (400, 5, ()), (400, 10, ()), (400, 10, ("topk",)), (400, 10, ("bottomk",))]
W, We = synth.make_bank(1234, D, C)
M.set_classifier_bank(W.to(dev), We.to(dev))
splits = []
for f in range(FOLDS):
    bags = [synth.make_bag_device(777 + 1000 * f + i, rows, D, We, C, i % C, dev, dt) for i in range(n)]
    splits.append(M.ResidentBags(bags, [i % C for i in range(n)], dev))
    del bags


def mk(cfg):
    return types.SimpleNamespace(disable_tqdm=True, n_classes=C, topj=cfg[0], topk=cfg[1], discard_classifiers=list(cfg[2]),
                                 pretrain="conch", ablation_study="none")


def build(configs, share):
    """One TrainRuns over configs x folds: fold-major inside a configuration, a seed per fold."""
    os.environ["MOC_RUNS_SHARE"] = "1" if share else "0"
    models, opts, sps, gens, args = [], [], [], [], []
    for cfg in configs:
        for f in range(FOLDS):
            torch.manual_seed(100 + f)
            model = M.senet(D, 4).to(dev)
            models.append(model)
            opts.append(torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-4))
            sps.append(splits[f])
            g = torch.Generator()
            g.manual_seed(7000 + f)
            gens.append(g)
            args.append(mk(cfg))
    return TrainRuns(models, opts, sps, dev, args if len(configs) > 1 else args[0], generators=gens)


def timed(what, sets):
    for _ in range(WARM):
        for rs in sets:
            rs.train_pass()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(PASSES):
        for rs in sets:
            rs.train_pass()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / PASSES * 1e3
    scored = sum(rs.trained_phase_a["scored_slides"] for rs in sets)
    slides = sum(rs.trained_phase_a["slides"] for rs in sets)
    print(f"{what}: {ms:.3f} ms per pass, scored_slides {scored} of {slides}", flush=True)
    return ms


print(f"shape: {FOLDS} folds x {n} slides x {rows} x {D} {dt}, C = {C}", flush=True)
for H in (4, 6):
    cfgs = CONFIGS[:H]
    a = timed(f"H={H} (1) one grid, shared score pass", [build(cfgs, True)])
    b = timed(f"H={H} (2) one grid, MOC_RUNS_SHARE=0  ", [build(cfgs, False)])
    c = timed(f"H={H} (3) {H} five-fold TrainRuns in turn ", [build([cfg], True) for cfg in cfgs])
    print(f"H={H}: (3)/(1) = {c / a:.2f}, (2)/(1) = {b / a:.2f}", flush=True)
    torch.cuda.empty_cache()
