#!/usr/bin/env python3
"""Sensitivity sweeps against the loops they replace, on the NSCLC-16 test shape (202 slides x 15,000 x 512):
    python scripts/bench_sweep.py [dtype fp32|bf16] [slides] [rows]
(a) moc_topk_mean_multi at Ks = 1, 5, 10, 20, 50 against five moc_topk_mean launches, over the slides' mixed scores and
    over their 15,000-row zero-shot statistics;
(b) evaluation_sweep for 4 topj x 3 discard sets x 5 topk against 60 evaluation() calls;
(c) zs_evaluation_sweep for 4 functions x 5 K against 20 zs_evaluation() calls.
Host clock around whole calls (the device idle before and after), two untimed calls first, three repeats, every repeat
printed."""
import os, sys, time, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
torch.set_num_threads(8)
from moc_amd import engine as E, main_moc as M, synth

dt = {"fp32": torch.float32, "bf16": torch.bfloat16}[sys.argv[1] if len(sys.argv) > 1 else "fp32"]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 202
rows = int(sys.argv[3]) if len(sys.argv) > 3 else 15000
dev = torch.device("cuda:0")
C, D = 2, 512
KS = [1, 5, 10, 20, 50]
TOPJS = [100, 200, 400, 800]
DISCARDS = [(), ("delta_softmax",), ("topk", "bottomk")]
W, We = synth.make_bank(1234, D, C)
M.set_classifier_bank(W.to(dev), We.to(dev))
bags = [synth.make_bag_device(777 + i, rows, D, We, C, i % C, dev, dt) for i in range(n)]
res = M.ResidentBags(bags, [i % C for i in range(n)], dev)
del bags
torch.manual_seed(0)
model = M.senet(D, 4).to(dev)


def mk(j=400, k=10, d=()):
    return types.SimpleNamespace(disable_tqdm=True, n_classes=C, topj=j, topk=k, discard_classifiers=list(d), pretrain="conch",
                                 ablation_study="none")


def timed(what, fn, inner=1):
    for _ in range(2):
        fn()
    out = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / inner * 1e6)
    print(f"{what}: " + "  ".join(f"{v:.0f}" for v in out) + " us", flush=True)
    return out


print(f"shape: {n} slides x {rows} x {D} {dt}, C = {C}", flush=True)
# (a) the kernel
bank = M._bank_for(res.X, dev)
batch = res.eval_plan(bank.C, bank.Ce, 400, 10, [])["batch"]
batch.phase_a(bank, for_eval=True)
E.meta_forward(batch, E.MetaState(model), 0, batch.n_slides, E.eval_use_bits(()), keep_hidden=False)
mixed = batch.meta_ws()[0]["mixed"]
timed("(a) mixed scores (topj 400): moc_topk_mean_multi, Ks 1 5 10 20 50",
      lambda: E.topk_mean_multi(mixed, mixed, KS, seg_off=batch.row_off, seg_len=batch.n_sel), inner=20)
lib = E.lib()


def five_mixed():
    for k in KS:
        p = torch.empty((batch.n_slides, C), dtype=torch.float32, device=dev)
        E.check(lib.moc_topk_mean(E.ptr(mixed), batch.total, E.ptr(mixed), batch.total, E.ptr(batch.row_off), E.ptr(batch.n_sel),
                                  batch.n_slides, C, k, 0, E.ptr(p), None, None, E._stream()), "moc_topk_mean")


timed("(a) mixed scores (topj 400): five moc_topk_mean launches", five_mixed, inner=20)
batch.scores(bank)
st = batch.stats[:C]
timed(f"(a) zero-shot statistics ({rows} rows): moc_topk_mean_multi, Ks 1 5 10 20 50",
      lambda: E.topk_mean_multi(st, st, KS, seg_off=batch.row_off), inner=20)
timed(f"(a) zero-shot statistics ({rows} rows): five moc_topk_mean launches",
      lambda: [E.topk_mean(st, st, k, seg_off=batch.row_off) for k in KS], inner=20)
# (b) the evaluation table
cells = len(TOPJS) * len(DISCARDS) * len(KS)
timed(f"(b) evaluation_sweep, {cells} cells", lambda: M.evaluation_sweep(model, res, dev, mk(), TOPJS, KS, DISCARDS))
timed(f"(b) {cells} evaluation() calls",
      lambda: [M.evaluation(model, res, dev, mk(j, k, d)) for j in TOPJS for d in DISCARDS for k in KS])
# (c) the zero-shot table
timed("(c) zs_evaluation_sweep, 20 cells", lambda: M.zs_evaluation_sweep(res, dev, mk(), KS))
timed("(c) 20 zs_evaluation() calls",
      lambda: [M.zs_evaluation(res, dev, mk(k=k), pooling_func=f) for f in M.ZS_POOLING_FUNCS for k in KS])
