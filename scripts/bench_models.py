#!/usr/bin/env python3
"""Time moc_meta_forward_models (R meta-learners in one launch) against R single moc_meta_forward launches on an
evaluation-sized batch: python scripts/bench_models.py [dtype] [R ...].  Default: the NSCLC-16 test-split shape (202 x
15,000 x 512, two classes, topj 400, topk 10), fp32, R = 1 5 16.  Run it under rocprofv3 --kernel-trace --stats for the
kernels' own times; the lines printed here are host events around each arm (W1 image builds included)."""
import os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from moc_amd import engine as E, main_moc as M, synth
dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[sys.argv[1] if len(sys.argv) > 1 else "fp32"]
Rs = [int(v) for v in sys.argv[2:]] or [1, 5, 16]
C, ns, rows = 2, 202, 15000
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
mixed = torch.empty((max(Rs), C, b.total), dtype=torch.float32, device=dev)
torch.cuda.synchronize()
S = int(b.n_sel.sum())


def timed(fn, reps=5):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


for R in Rs:
    sep = timed(lambda: [E.meta_forward(b, metas[r], 0, ns, 15, keep_hidden=False) for r in range(R)])
    one = timed(lambda: E.meta_forward_models(b, arena, R, mixed[:R], 0, ns, 15))
    print(f"{dt} R={R} selected={S}: {R} single launches {sep:.1f} us, one R-model launch {one:.1f} us "
          f"(ratio {one / sep:.2f})", flush=True)
