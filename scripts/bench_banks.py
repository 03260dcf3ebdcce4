#!/usr/bin/env python3
"""Bank sweeps against the loops they replace, on the NSCLC-16 test shape (202 slides x 15,000 x 512):
    python scripts/bench_banks.py [dtype fp32|bf16] [slides] [rows]
    MOC_HIP_LIB=<the parent commit's libmoc_hip.so> python scripts/bench_banks.py ...     # the reference side of (a)
(a) for G = 1 .. moc_scores_banks_max: one moc_scores_banks launch over G banks against G moc_scores launches.  The
    library is loaded here by hand (ctypes, the path moc_amd._lib would take), so the same script times the G moc_scores
    launches of a library that has no moc_scores_banks -- the parent commit's, through MOC_HIP_LIB; with this tree's
    library both sides are printed.
(b) five banks: zs_evaluation_sweep_banks (4 functions x 5 K per bank) against five set_classifier_bank +
    zs_evaluation_sweep calls (this tree's library only).
Host clock around whole calls (the device idle before and after), two untimed calls first, three repeats, every repeat
printed."""
import ctypes as C
import os, sys, time, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
torch.set_num_threads(8)
from moc_amd import _lib, engine as E, synth

dt = {"fp32": torch.float32, "bf16": torch.bfloat16}[sys.argv[1] if len(sys.argv) > 1 else "fp32"]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 202
rows = int(sys.argv[3]) if len(sys.argv) > 3 else 15000
dev = torch.device("cuda:0")
Cn, D = 2, 512
KS = [1, 5, 10, 20, 50]
CES = [6, 3, 16, 4, 6]                                   # five banks: widths C+4, C+1, 16, C+2, C+4
code = E._dtype_code(dt)

h = C.CDLL(_lib.LIB_PATH)
has_banks = hasattr(h, "moc_scores_banks")
for name in ("moc_bank_bytes", "moc_prepare_bank", "moc_mask_compact", "moc_scores") + \
        (("moc_scores_banks_max", "moc_scores_banks") if has_banks else ()):
    getattr(h, name).restype, getattr(h, name).argtypes = _lib.SIGNATURES[name]
print(f"library: {_lib.LIB_PATH} ({'with' if has_banks else 'without'} moc_scores_banks)", flush=True)

banks = [synth.make_bank(1234 + 10 * b, D, Cn, n_bg=ce - Cn) for b, ce in enumerate(CES)]
banks = [(W.to(dev), We.to(dev)) for W, We in banks]
X = torch.cat([synth.make_bag_device(777 + i, rows, D, banks[0][1], Cn, i % Cn, dev, dt) for i in range(n)], 0)
sizes = [rows] * n
print(f"shape: {n} slides x {rows} x {D} {dt}, C = {Cn}: {X.numel() * X.element_size() / 1e9:.2f} GB of bags", flush=True)


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


def check(rc, what):
    assert rc == 0, (what, rc)


# (a) the score pass: per bank its own batch (statistics, flags) and image, as G evaluations hold them
tile = h.moc_bank_bytes(D, 16, code)
gmax = h.moc_scores_banks_max(D, code) if has_banks else (4 if dt == torch.float32 else 3)
image = torch.empty(gmax * tile, dtype=torch.uint8, device=dev)
batches = []
for g in range(gmax):
    W, We = banks[g]
    check(h.moc_prepare_bank(E.ptr(W), E.ptr(We), D, Cn, CES[g], code, 0, image.data_ptr() + g * tile, E._stream()), "moc_prepare_bank")
    batches.append(E.SlideBatch(X, sizes, Cn, CES[g], 400, 10))
torch.cuda.synchronize()
for G in range(1, gmax + 1):
    def loop(G=G):
        for g in range(G):
            check(h.moc_scores(C.byref(batches[g].c), image.data_ptr() + g * tile, E._stream()), "moc_scores")
    timed(f"(a) G = {G}: {G} moc_scores launches", loop, inner=5)
    if has_banks:
        S = _lib.MocBankSet(n_banks=G, C=Cn, image=image.data_ptr())
        for g in range(G):
            S.Ce[g], S.stats[g], S.sel_flag[g] = CES[g], E.ptr(batches[g].stats), E.ptr(batches[g].sel_flag)
        timed(f"(a) G = {G}: one moc_scores_banks launch",
              lambda S=S: check(h.moc_scores_banks(C.byref(batches[0].c), C.byref(S), E._stream()), "moc_scores_banks"), inner=5)
del batches
if not has_banks:
    sys.exit(0)

# (b) the zero-shot table of five banks
from moc_amd import main_moc as M
res = M.ResidentBags([X[i * rows:(i + 1) * rows] for i in range(n)], [i % Cn for i in range(n)], dev)
del X
args = types.SimpleNamespace(disable_tqdm=True, n_classes=Cn, topj=400, topk=10, discard_classifiers=[], pretrain="conch",
                             ablation_study="none")


def five_calls():
    out = []
    for W, We in banks:
        M.set_classifier_bank(W, We)
        out.append(M.zs_evaluation_sweep(res, dev, args, KS))
    return out


timed("(b) zs_evaluation_sweep_banks, five banks x 20 cells", lambda: M.zs_evaluation_sweep_banks(res, dev, args, banks, KS))
timed("(b) five set_classifier_bank + zs_evaluation_sweep calls", five_calls)
assert M.zs_evaluation_sweep_banks(res, dev, args, banks, KS) == five_calls()
