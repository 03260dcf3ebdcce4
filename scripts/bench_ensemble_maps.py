#!/usr/bin/env python3
"""Time moc_meta_forward_dense_models (R meta-learners over every row, reduced on the device) against R single
moc_meta_forward_dense launches plus the torch softmax / mean / std over their R slabs:
python scripts/bench_ensemble_maps.py [dtype] [C] [R ...].  Default: the NSCLC-16 test-split shape (202 x 15,000 x 512,
two classes, topj 400, topk 10), fp32, R = 1 5 16.  Host events around 3 calls per arm (W1 image builds included); run it
under rocprofv3 --kernel-trace --stats for the kernels' own times."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from moc_amd import engine as E, main_moc as M, synth  # noqa: E402

dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[sys.argv[1] if len(sys.argv) > 1 else "fp32"]
C = int(sys.argv[2]) if len(sys.argv) > 2 else 2
Rs = [int(v) for v in sys.argv[3:]] or [1, 5, 16]
ns, rows = 202, 15000
dev = torch.device("cuda:0")
W, We = synth.make_bank(1, 512, C)
X = torch.cat([synth.make_bag_device(10 + i, rows, 512, We, C, i % C, dev, dt) for i in range(ns)])
bank = E.Bank.get(W.to(dev), We.to(dev), dt, dev)
b = E.SlideBatch(X, [rows] * ns, C, C + 4, 400, 10)
b.phase_a(bank, for_eval=True)
models = []
for r in range(max(Rs)):
    torch.manual_seed(r)
    models.append(M.senet(512, 4).to(dev))
metas = [E.MetaState(m) for m in models]
arena = E.ModelArena([m.state_dict() for m in models], dev)
T = b.total
scale = M.CONCH_TEMPERATURE
slabs = torch.empty((max(Rs), C, T), dtype=torch.float32, device=dev)
gslabs = torch.empty((max(Rs), T, 4), dtype=torch.float32, device=dev)
pm = torch.empty((C, T), dtype=torch.float32, device=dev)
ps = torch.empty((C, T), dtype=torch.float32, device=dev)
gm = torch.empty((T, 4), dtype=torch.float32, device=dev)
torch.cuda.synchronize()


def separate(R):
    for r in range(R):
        E.meta_forward_dense(b, metas[r], 0, ns, 15, gslabs[r], slabs[r])
    p = torch.softmax(slabs[:R] * scale, dim=1)
    return p.mean(dim=0), p.std(dim=0, unbiased=False), gslabs[:R].mean(dim=0)


def fused(R):
    E.meta_forward_dense_models(b, arena, R, scale, pm, ps, gm, 0, ns, 15)


def timed(fn, reps=3):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


for R in Rs:
    sep = timed(lambda: separate(R))
    one = timed(lambda: fused(R))
    mean, std, g = separate(R)
    fused(R)
    torch.cuda.synchronize()
    err = max(float((mean - pm).abs().max()), float((std - ps).abs().max()))
    print(f"{dt} C={C} R={R} rows={T}: {R} dense launches + torch {sep:.1f} us, one dense-models launch {one:.1f} us "
          f"(ratio {one / sep:.2f}); max |diff| {err:.2e}", flush=True)
