"""Row f3: time the adapter heads' fused forward (forward_fused: moc_adapter_logits + the torch layers on the pooled rows)
against their torch path (`fused = False`: the op chain over the whole bag, unchanged from before the kernel existed), forward
only and forward + backward, for Conch_CLIP_Ada (E = 1) and Conch_MOE_CLIP_Ada (E = 5); and the kernel alone against its
bounds -- the bag's bytes at E = 1, the six-term bf16 matrix rate (4 N c h E 6 flops) at E = 5.

Each figure is the median of `--iters` single runs, each between two events, after `--warmup` untimed runs.

    python scripts/bench_adapter.py [--n 15000] [--classes 2] [--iters 30] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from moc_amd import engine  # noqa: E402
from moc_amd import model_adapters as A  # noqa: E402

BF16_MFMA_PEAK = 2.5e15       # dense bf16 (v_mfma_f32_16x16x32_bf16 = 16 cycles per SIMD)
HBM_PEAK = 8.0e12


def median_us(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=15000)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert a.iters >= 20
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    x = torch.randn(a.n, 512, generator=g).to(dev)
    cls = torch.nn.functional.normalize(torch.randn(512, a.classes, generator=g), dim=0).to(dev)
    rows = []
    for E in (1, 5):
        torch.manual_seed(1)
        model = (A.Conch_CLIP_Ada(num_classes=a.classes, classifier_tensor=cls) if E == 1
                 else A.Conch_MOE_CLIP_Ada(ada_num=E, classifier_tensor=cls)).to(dev)
        nets = [model.adapter] if E == 1 else [getattr(model, f"adapter_{i}") for i in range(E)]
        W1s, W2s = [n[0].weight for n in nets], [n[2].weight for n in nets]
        gate = None if E == 1 else model.ada_router.gate.weight
        w = torch.arange(1, a.classes + 1, device=dev, dtype=torch.float32)

        def fwd():
            with torch.no_grad():
                return model(x)

        def fwd_bwd():
            model.zero_grad(set_to_none=True)
            (model(x) * w).sum().backward()

        r = {"E": E, "N": a.n, "C": a.classes}
        for fused in (False, True):
            model.fused = fused
            tag = "fused" if fused else "torch"
            r[f"{tag}_fwd_us"] = median_us(fwd, a.iters, a.warmup)
            r[f"{tag}_fwd_bwd_us"] = median_us(fwd_bwd, a.iters, a.warmup)
        r["kernel_us"] = median_us(lambda: engine.adapter_logits(x, W1s, W2s, gate, cls, model.clip_ratio), a.iters, a.warmup)
        r["kernel_bag_bytes_per_s"] = a.n * 512 * 4 / (r["kernel_us"] * 1e-6)
        r["kernel_six_term_flops"] = 4.0 * a.n * 512 * 128 * E * 6 / (r["kernel_us"] * 1e-6)
        rows.append(r)
        print(f"E={E} N={a.n} C={a.classes}")
        print(f"  forward            : torch {r['torch_fwd_us']:9.1f} us   fused {r['fused_fwd_us']:9.1f} us")
        print(f"  forward + backward : torch {r['torch_fwd_bwd_us']:9.1f} us   fused {r['fused_fwd_bwd_us']:9.1f} us")
        print(f"  moc_adapter_logits : {r['kernel_us']:9.1f} us   bag at {r['kernel_bag_bytes_per_s'] / 1e12:.3f} TB/s "
              f"({r['kernel_bag_bytes_per_s'] / HBM_PEAK:.2f} of HBM peak)   six-term products at "
              f"{r['kernel_six_term_flops'] / 1e12:.1f} TFLOP/s ({r['kernel_six_term_flops'] / BF16_MFMA_PEAK:.3f} of the bf16 matrix peak)")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
