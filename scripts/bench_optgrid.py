#!/usr/bin/env python3
"""A 3 x 3 (lr, weight decay) grid on one NSCLC-16-shaped fold (32 slides x 15,000 x 512) in one TrainRuns against the
ways it replaces:
    python scripts/bench_optgrid.py [dtype fp32|bf16] [slides] [rows]
  (1) one TrainRuns(per_run_adam=True) over the nine cells: one mask group, lockstep chains of 5 + 4 with per-run Adam;
  (2) the nine cells one after the other through main_moc.train (what nine processes do, minus their start-up);
  (3) nine runs with EQUAL hyper-parameters on the same split through moc_train_steps_runs, and
  (4) the same nine through moc_train_steps_runs_hp: what the per-run coefficients cost a launch.
Host clock with a final synchronize; three untimed passes, then ten timed ones; meta-steps/s = cells x slides x passes / s."""
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
WARM, PASSES = 3, 10
dev = torch.device("cuda:0")
C, D = 2, 512
CELLS = [(lr, wd) for lr in (3e-4, 1e-3, 3e-3) for wd in (0.0, 1e-4, 1e-2)]
W, We = synth.make_bank(1234, D, C)
M.set_classifier_bank(W.to(dev), We.to(dev))
bags = [synth.make_bag_device(777 + i, rows, D, We, C, i % C, dev, dt) for i in range(n)]
split = M.ResidentBags(bags, [i % C for i in range(n)], dev)
del bags
args = types.SimpleNamespace(disable_tqdm=True, n_classes=C, topj=400, topk=10, discard_classifiers=[], pretrain="conch",
                             ablation_study="none")


def cell(lr, wd):
    torch.manual_seed(100)
    model = M.senet(D, 4).to(dev)
    return model, torch.optim.Adam(model.parameters(), lr=lr, weight_decay=wd)


def grid(cells, per_run_adam):
    models, opts, gens = [], [], []
    for lr, wd in cells:
        m, o = cell(lr, wd)
        models.append(m)
        opts.append(o)
        gens.append(torch.Generator().manual_seed(7000))
    return TrainRuns(models, opts, [split] * len(cells), dev, args, generators=gens, per_run_adam=per_run_adam)


def timed(what, one_pass):
    for _ in range(WARM):
        one_pass()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(PASSES):
        one_pass()
    torch.cuda.synchronize()
    s = (time.perf_counter() - t0) / PASSES
    rate = len(CELLS) * n / s
    print(f"{what}: {s * 1e3:.3f} ms per pass of nine cells, {rate / 1e3:.1f} k meta-steps/s", flush=True)
    return rate


print(f"shape: one fold, {n} slides x {rows} x {D} {dt}, C = {C}, nine (lr, wd) cells", flush=True)
rs = grid(CELLS, True)
a = timed("(1) one grid, per-run Adam, one mask group ", rs.train_pass)
print(f"    groups {[g['runs'].n_runs for g in rs.groups]}, phase A {rs.trained_phase_a}", flush=True)
del rs
alone = [cell(lr, wd) for lr, wd in CELLS]


def in_turn():
    for m, o in alone:
        M.train(m, split, o, dev, args)
b = timed("(2) nine cells in turn, main_moc.train      ", in_turn)
del alone
same = [(1e-3, 1e-4)] * len(CELLS)
rs = grid(same, False)
c = timed("(3) nine equal cells, moc_train_steps_runs   ", rs.train_pass)
del rs
rs = grid(same, True)
d = timed("(4) nine equal cells, moc_train_steps_runs_hp", rs.train_pass)
print(f"(1)/(2) = {a / b:.2f}   (4)/(3) = {d / c:.3f}", flush=True)
