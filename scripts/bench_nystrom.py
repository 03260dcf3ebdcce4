"""Row f3: time TransMIL's fused Nystrom forward (NystromAttention.forward_fused: moc_nystrom_landmark_values +
moc_nystrom_token_values around the torch pieces) against the torch path (`fused = False`, unchanged from before the
kernels existed), and the same with the pseudo-inverse on moc_nystrom_pinv (`fused_pinv = True`) against `fused` alone,
all under no_grad: the whole model on one bag, one attention layer alone, and each kernel alone against its two bounds --
the bytes it must move and its products at the fp32 matrix peak (v_mfma_f32_16x16x4_f32); moc_nystrom_pinv also against
moore_penrose_iter_pinv on the same attn2.

Each figure is the median and the minimum of `--iters` single runs, each between two events, after `--warmup` untimed
runs.  "faster" is claimed only where a median is below the minimum of the path it is compared with.

With --train: forward + backward of one attention layer and of the whole model on the same bag, the torch path (autograd
keeps both [8, n, 256] score matrices and their softmax outputs) against `fused` + `fused_train` (LandmarkValues /
TokenValues: the backward of moc_nystrom_bwd.hip recomputes the weights) and against those two with `fused_conv` on top
(TokenValuesResidual: the residual convolution stays in kernel B, its gradients are moc_nystrom_conv_bwd.hip's) and against
all three with `fused_pinv_train` on top (LandmarkPinv: the pseudo-inverse and its gradient on moc_nystrom_pinv.hip), all four
in the same run and timed the same way, each with the peak of torch.cuda.max_memory_allocated over one step, above what was
allocated before it.  Then each backward entry alone against its two bounds, and the torch pieces all paths share, each
alone, forward + backward: res_conv, moore_penrose_iter_pinv, to_qkv, and the model's pos_layer (PPEG) -- that one also on
moc_ppeg.hip (`PPEG.fused`), with the two entries alone against the bytes they must move, and the whole model with
`fused_ppeg` on top of the other four switches; without --train the no-grad model pass and pos_layer with and without
`fused_ppeg`; beside
moore_penrose_iter_pinv, on the same attn2, moc_nystrom_pinv_iterates + moc_nystrom_pinv_backward with independent products
sharing launches (the default) and with one product per launch.

With --maps: moc_nystrom_attention_rows alone (R = 1 and R = 16) against its two bounds, then TransMIL.attention_maps on
the same bag with `fused` + `fused_pinv` + `fused_ppeg` against the same call with `fused = False` (the torch rows path, which
forms attn3, the [8, 256, n_pad] score matrix), each with its peak memory, and the plain no-grad forward under the same three
switches, which is what the maps are an addition to.

    python scripts/bench_nystrom.py [--n 15000] [--iters 30] [--json out.json] [--train | --maps]
    rocprofv3 --kernel-trace --stats ... -- python scripts/bench_nystrom.py --trace-layers 8
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from moc_amd import engine  # noqa: E402
from moc_amd.model_mil import TransMIL  # noqa: E402
from moc_amd.nystrom import moore_penrose_iter_pinv  # noqa: E402

F32_MFMA_PEAK = 157.3e12      # v_mfma_f32_16x16x4_f32: 64 flop / clock / SIMD
HBM_PEAK = 8.0e12
H, D, M, TAPS = 8, 64, 256, 33


def times_us(fn, iters, warmup):
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
    return {"median_us": statistics.median(out), "min_us": min(out)}


def pair(label, fn, switch, iters, warmup):
    """fn timed on the torch path, with `fused`, and with `fused` + `fused_pinv`; switch(fused, fused_pinv) sets the flags."""
    r = {}
    for key, flags in (("torch", (False, False)), ("fused", (True, False)), ("fused_pinv", (True, True))):
        switch(*flags)
        r[key] = times_us(fn, iters, warmup)
    switch(False, False)
    t, f, p = r["torch"], r["fused"], r["fused_pinv"]
    r["fused_is_faster"] = f["median_us"] < t["min_us"]
    r["fused_pinv_is_faster_than_fused"] = p["median_us"] < f["min_us"]
    print(f"{label:24s}: torch median {t['median_us']:9.1f} us (min {t['min_us']:9.1f})   fused median {f['median_us']:9.1f} us "
          f"(min {f['min_us']:9.1f})   {'fused faster' if r['fused_is_faster'] else 'NOT faster'} "
          f"(x{t['median_us'] / f['median_us']:.2f} on the medians)")
    print(f"{'':24s}  fused + fused_pinv median {p['median_us']:9.1f} us (min {p['min_us']:9.1f})   "
          f"{'faster than fused' if r['fused_pinv_is_faster_than_fused'] else 'NOT faster than fused'} "
          f"(x{f['median_us'] / p['median_us']:.2f} on the medians)")
    return r


def kernel(label, fn, nbytes, flops, iters, warmup):
    r = times_us(fn, iters, warmup)
    sec = r["median_us"] * 1e-6
    r.update(bytes=nbytes, flops=flops, bytes_per_s=nbytes / sec, flops_per_s=flops / sec,
             hbm_bound_us=nbytes / HBM_PEAK * 1e6, mfma_bound_us=flops / F32_MFMA_PEAK * 1e6)
    nearer = max(r["hbm_bound_us"], r["mfma_bound_us"])
    r["fraction_of_nearer_bound"] = nearer / r["median_us"]
    print(f"{label:24s}: median {r['median_us']:8.1f} us (min {r['min_us']:8.1f})   {nbytes / 1e6:6.1f} MB at "
          f"{r['bytes_per_s'] / 1e12:.3f} TB/s (bound {r['hbm_bound_us']:.1f} us)   {flops / 1e9:5.2f} GFLOP at "
          f"{r['flops_per_s'] / 1e12:.1f} TFLOP/s (bound {r['mfma_bound_us']:.1f} us)   {r['fraction_of_nearer_bound']:.2f} of the nearer bound")
    return r


def train_pair(label, step, switch, iters, warmup, ppeg=False):
    """step() -- one forward + backward -- timed and its peak memory taken on the torch path, with `fused` + `fused_train`,
    with `fused_conv` on top of those, with `fused_pinv_train` on top of all three and, for the model (`ppeg`), with
    `fused_ppeg` on top of all four; switch(fused_train, fused_conv, fused_pinv_train, fused_ppeg) sets the flags."""
    r = {}
    configs = [("torch", (False, False, False, False)), ("fused_train", (True, False, False, False)),
               ("fused_conv", (True, True, False, False)), ("fused_pinv_train", (True, True, True, False))]
    if ppeg:
        configs.append(("fused_ppeg", (True, True, True, True)))
    for key, flags in configs:
        switch(*flags)
        r[key] = times_us(step, iters, warmup)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step()
        torch.cuda.synchronize()
        r[key]["peak_bytes"] = torch.cuda.max_memory_allocated() - base
    switch(False, False, False, False)
    t, f, c, p = r["torch"], r["fused_train"], r["fused_conv"], r["fused_pinv_train"]
    r["fused_train_is_faster"] = f["median_us"] < t["min_us"]
    r["fused_conv_is_faster_than_fused_train"] = c["median_us"] < f["min_us"]
    r["fused_pinv_train_is_faster_than_fused_conv"] = p["median_us"] < c["min_us"]
    print(f"{label:32s}: torch median {t['median_us']:9.1f} us (min {t['min_us']:9.1f}) peak {t['peak_bytes'] / 2**20:8.1f} MiB   "
          f"fused_train median {f['median_us']:9.1f} us (min {f['min_us']:9.1f}) peak {f['peak_bytes'] / 2**20:8.1f} MiB   "
          f"{'fused_train faster' if r['fused_train_is_faster'] else 'NOT faster'} (x{t['median_us'] / f['median_us']:.2f} on the "
          f"medians, x{t['peak_bytes'] / max(f['peak_bytes'], 1):.2f} on the peaks)")
    print(f"{'':32s}  fused_train + fused_conv median {c['median_us']:9.1f} us (min {c['min_us']:9.1f}) peak "
          f"{c['peak_bytes'] / 2**20:8.1f} MiB   "
          f"{'faster than fused_train' if r['fused_conv_is_faster_than_fused_train'] else 'NOT faster than fused_train'} "
          f"(x{f['median_us'] / c['median_us']:.2f} on the medians, x{t['median_us'] / c['median_us']:.2f} on the torch path's)")
    print(f"{'':32s}  ... + fused_pinv_train median {p['median_us']:9.1f} us (min {p['min_us']:9.1f}) peak "
          f"{p['peak_bytes'] / 2**20:8.1f} MiB   "
          f"{'faster than fused_conv' if r['fused_pinv_train_is_faster_than_fused_conv'] else 'NOT faster than fused_conv'} "
          f"(x{c['median_us'] / p['median_us']:.2f} on the medians, x{t['median_us'] / p['median_us']:.2f} on the torch path's)")
    if ppeg:
        q = r["fused_ppeg"]
        r["fused_ppeg_is_faster_than_fused_pinv_train"] = q["median_us"] < p["min_us"]
        print(f"{'':32s}  ... + fused_ppeg median {q['median_us']:9.1f} us (min {q['min_us']:9.1f}) peak "
              f"{q['peak_bytes'] / 2**20:8.1f} MiB   "
              f"{'faster than fused_pinv_train' if r['fused_ppeg_is_faster_than_fused_pinv_train'] else 'NOT faster than fused_pinv_train'} "
              f"(x{p['median_us'] / q['median_us']:.2f} on the medians, x{t['median_us'] / q['median_us']:.2f} on the torch path's)")
    return r


def stream_kernel(label, fn, nbytes, iters, warmup):
    """A kernel with no matrix products (moc_ppeg_*) against the bytes it must move."""
    r = times_us(fn, iters, warmup)
    sec = r["median_us"] * 1e-6
    r.update(bytes=nbytes, bytes_per_s=nbytes / sec, hbm_bound_us=nbytes / HBM_PEAK * 1e6)
    r["fraction_of_bound"] = r["hbm_bound_us"] / r["median_us"]
    print(f"{label:24s}: median {r['median_us']:8.1f} us (min {r['min_us']:8.1f})   {nbytes / 1e6:6.1f} MB at "
          f"{r['bytes_per_s'] / 1e9:.0f} GB/s (bound {r['hbm_bound_us']:.1f} us)   {r['fraction_of_bound']:.2f} of the bound")
    return r


def ppeg_entries(ppeg, x, side, cot, out, iters, warmup):
    """The two PPEG entries alone on x [1, 1 + side^2, 512].  Bytes: the forward reads x and writes out, the backward reads x
    and dout and writes dx; weights, gradients of weights and the workspace are below 1% of either."""
    row = x.shape[1] * 512 * 4
    p = [t.detach() for t in (ppeg.proj.weight, ppeg.proj.bias, ppeg.proj1.weight, ppeg.proj1.bias, ppeg.proj2.weight, ppeg.proj2.bias)]
    out["ppeg_forward"] = stream_kernel("moc_ppeg_forward", lambda: engine.ppeg_forward(x, side, side, *p), 2 * row, iters, warmup)
    out["ppeg_backward"] = stream_kernel("moc_ppeg_backward", lambda: engine.ppeg_backward(x, side, side, p[0], p[2], p[4], cot),
                                         3 * row, iters, warmup)


def piece(label, step, iters, warmup):
    """One torch piece of the layer or the model alone, forward + backward, on the shape the model gives it."""
    r = times_us(step, iters, warmup)
    print(f"{label:32s}: fwd + bwd median {r['median_us']:9.1f} us (min {r['min_us']:9.1f})")
    return r


def train(a, dev, g, bag, model, attn, out):
    side = math.ceil(math.sqrt(a.n))
    n_tok = side * side + 1
    out["tokens"] = n_tok
    x = torch.nn.functional.layer_norm(torch.randn(1, n_tok, 512, generator=g), (512,)).to(dev)
    cot = torch.randn(1, n_tok, 512, generator=g).to(dev)
    label = torch.tensor([1], device=dev)

    def flags(module):
        return lambda on, conv, pinv, ppeg: (setattr(module, "fused", on), setattr(module, "fused_train", on),
                                             setattr(module, "fused_conv", conv), setattr(module, "fused_pinv_train", pinv),
                                             hasattr(module, "pos_layer") and setattr(module, "fused_ppeg", ppeg))

    def layer_step():
        attn.zero_grad(set_to_none=True)
        xi = x.detach().requires_grad_(True)
        (attn(xi) * cot).sum().backward()

    def model_step():
        model.zero_grad(set_to_none=True)
        torch.nn.functional.cross_entropy(model(bag)[0], label).backward()
    out["train_model"] = train_pair(f"TransMIL {a.n} x 512, fwd + bwd", model_step, flags(model), a.iters, a.warmup, ppeg=True)
    out["train_layer"] = train_pair(f"one layer, {n_tok} tokens, fwd + bwd", layer_step, flags(attn), a.iters, a.warmup)

    # each backward entry alone against its two bounds.  Bytes: qkv's columns it reads, twice (once per kernel), dout likewise,
    # and the dqkv it writes; products: [256, n] x 64 per head, 7 on the landmark side (S, dP twice; dv, dk, dq_l), 8 on the
    # token side (S twice, dP three times -- delta takes a walk of its own --; dq, dk_l, dY)
    with torch.no_grad():
        n_pad = -(-n_tok // M) * M
        out["n_pad"] = n_pad
        qkv = attn.to_qkv(torch.nn.functional.pad(x, (0, 0, n_pad - n_tok, 0)))[0].contiguous()
        l = n_pad // M
        q_l = ((qkv[:, :512] * attn.scale).reshape(M, l, H, D).sum(1) / l).transpose(0, 1).contiguous()
        k_l = (qkv[:, 512:1024].reshape(M, l, H, D).sum(1) / l).transpose(0, 1).contiguous()
        W, lse = engine.nystrom_landmark_values_lse(qkv, q_l)
        dW = torch.randn(H, M, D, generator=g).to(dev)
        dout = torch.randn(n_pad, H * D, generator=g).to(dev)
        scores = 2.0 * H * M * n_pad * D
        out["landmark_backward"] = kernel("moc_nystrom_landmark_backward",
                                          lambda: engine.nystrom_landmark_backward(qkv, q_l, W, lse, dW),
                                          (2 * 2 + 3) * n_pad * 512 * 4, 7 * scores, a.iters, a.warmup)
        out["token_backward"] = kernel("moc_nystrom_token_backward",
                                       lambda: engine.nystrom_token_backward(qkv, k_l, W, attn.scale, dout),
                                       (2 * 2 + 3) * n_pad * 512 * 4, 8 * scores, a.iters, a.warmup)
        # the residual convolution's backward alone: it reads dout and qkv's v columns and writes dv; two banded products of
        # 48 rows per 16-token tile (dv, and the [48, 16] tile whose diagonals are the tap gradients)
        w = attn.res_conv.weight.detach().reshape(H, TAPS).contiguous()
        dqkv = torch.zeros_like(qkv)
        out["conv_backward"] = kernel("moc_nystrom_conv_backward", lambda: engine.nystrom_conv_backward(qkv, w, dout, dqkv),
                                      3 * n_pad * 512 * 4, 2 * 2.0 * n_pad * 512 * 48, a.iters, a.warmup)

    # the torch pieces every path shares, each alone, forward + backward, on the shapes the model gives them: by these
    # numbers the next kernel on this path is chosen
    def backward_of(make, *leaves):
        def step():
            for t in leaves:
                t.grad = None
            make().sum().backward()
        return step

    v = torch.randn(1, H, n_pad, D, generator=g).to(dev).requires_grad_(True)
    out["piece_res_conv"] = piece(f"res_conv on [1, 8, {n_pad}, 64]", backward_of(lambda: attn.res_conv(v), v, attn.res_conv.weight),
                                  a.iters, a.warmup)
    attn2 = (q_l @ k_l.transpose(-1, -2)).softmax(dim=-1).requires_grad_(True)
    out["piece_pinv"] = piece("moore_penrose_iter_pinv [8, 256, 256]",
                              backward_of(lambda: moore_penrose_iter_pinv(attn2.unsqueeze(0), attn.pinv_iterations), attn2),
                              a.iters, a.warmup)
    # the same on the kernels: the iterates and their backward, 2 + 4 iters launches, then 7 + 4 iters with independent
    # products side by side, or 4 + 8 iters with one product per launch (the diagnostic switch is read on every call)
    its, x2, dz = attn.pinv_iterations, attn2.detach(), torch.randn(H, M, M, generator=g).to(dev)

    def pinv_step():
        engine.nystrom_pinv_backward(x2, engine.nystrom_pinv_iterates(x2, its), dz, its)
    for key, env, launches in (("grouped", "1", 7 + 4 * its), ("ungrouped", "0", 4 + 8 * its)):
        os.environ["MOC_PINV_BWD_GROUPED"] = env
        r = piece(f"moc_nystrom_pinv_iterates + _backward, {key}", pinv_step, a.iters, a.warmup)
        r["launches"] = 2 + 4 * its + launches
        out["pinv_train_" + key] = r
    del os.environ["MOC_PINV_BWD_GROUPED"]
    gr, un, tp = out["pinv_train_grouped"], out["pinv_train_ungrouped"], out["piece_pinv"]
    out["pinv_train_grouped_is_faster_than_ungrouped"] = gr["median_us"] < un["min_us"]
    out["pinv_train_is_faster_than_torch"] = gr["median_us"] < tp["min_us"]
    print(f"{'':32s}  grouped ({gr['launches']} launches) {'faster' if gr['median_us'] < un['min_us'] else 'NOT faster'} than ungrouped "
          f"({un['launches']}); {'faster' if gr['median_us'] < tp['min_us'] else 'NOT faster'} than torch "
          f"(x{tp['median_us'] / gr['median_us']:.2f} on the medians)")
    xp = torch.nn.functional.pad(x, (0, 0, n_pad - n_tok, 0)).requires_grad_(True)
    out["piece_to_qkv"] = piece(f"to_qkv on [1, {n_pad}, 512]", backward_of(lambda: attn.to_qkv(xp), xp, attn.to_qkv.weight),
                                a.iters, a.warmup)
    xt = x.detach().clone().requires_grad_(True)
    ppeg = model.pos_layer
    out["piece_pos_layer"] = piece(f"pos_layer (PPEG) on [1, {n_tok}, 512]",
                                   backward_of(lambda: ppeg(xt, side, side), xt, *ppeg.parameters()), a.iters, a.warmup)
    # the same on moc_ppeg.hip (PPEG.fused), then its two entries alone
    ppeg.fused = True
    out["piece_pos_layer_fused"] = piece("pos_layer (PPEG), fused", backward_of(lambda: ppeg(xt, side, side), xt, *ppeg.parameters()),
                                         a.iters, a.warmup)
    ppeg.fused = False
    tp, fp = out["piece_pos_layer"], out["piece_pos_layer_fused"]
    out["pos_layer_fused_is_faster"] = fp["median_us"] < tp["min_us"]
    print(f"{'':32s}  fused {'faster' if out['pos_layer_fused_is_faster'] else 'NOT faster'} than torch "
          f"(x{tp['median_us'] / fp['median_us']:.2f} on the medians)")
    ppeg_entries(ppeg, x, side, cot, out, a.iters, a.warmup)


def maps(a, dev, g, bag, model, attn, out):
    side = math.ceil(math.sqrt(a.n))
    n_tok = side * side + 1
    n_pad = -(-n_tok // M) * M
    out.update(tokens=n_tok, n_pad=n_pad)
    with torch.no_grad():
        x = torch.nn.functional.layer_norm(torch.randn(1, n_tok, 512, generator=g), (512,)).to(dev)
        qkv = attn.to_qkv(torch.nn.functional.pad(x, (0, 0, n_pad - n_tok, 0)))[0].contiguous()
        l = n_pad // M
        q_l = ((qkv[:, :512] * attn.scale).reshape(M, l, H, D).sum(1) / l).transpose(0, 1).contiguous()
        k_l = (qkv[:, 512:1024].reshape(M, l, H, D).sum(1) / l).transpose(0, 1).contiguous()
        pinv = moore_penrose_iter_pinv((q_l @ k_l.transpose(-1, -2)).softmax(dim=-1).unsqueeze(0), attn.pinv_iterations)[0]
        _, lse = engine.nystrom_landmark_values_lse(qkv, q_l)
        # the entry alone.  Bytes: qkv's k columns and the rows it writes; products: the [256, n] x 64 scores per head and the
        # second product at the 16 rows of its MFMA tile, whatever R is
        for R in (1, 16):
            q_r = qkv[n_pad - n_tok:n_pad - n_tok + R, :512].reshape(R, H, D).transpose(0, 1) * attn.scale
            coef = ((q_r @ k_l.transpose(-1, -2)).softmax(dim=-1) @ pinv).contiguous()
            out[f"attention_rows_R{R}"] = kernel(f"moc_nystrom_attention_rows R={R}",
                                                 lambda: engine.nystrom_attention_rows(qkv, q_l, lse, coef),
                                                 n_pad * 512 * 4 + H * R * n_pad * 4, 2.0 * H * M * n_pad * (D + 16), a.iters, a.warmup)
    model.fused_pinv = model.fused_ppeg = True
    r = {}
    for key, fused, fn in (("torch", False, lambda: model.attention_maps(bag)), ("fused", True, lambda: model.attention_maps(bag)),
                           ("forward", True, lambda: model(bag))):
        model.fused = fused
        with torch.no_grad():
            r[key] = times_us(fn, a.iters, a.warmup)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            r[key]["peak_bytes"] = torch.cuda.max_memory_allocated() - base
    model.fused = model.fused_pinv = model.fused_ppeg = False
    t, f, p = r["torch"], r["fused"], r["forward"]
    r["fused_is_faster"] = f["median_us"] < t["min_us"]
    r["over_forward_us"] = f["median_us"] - p["median_us"]
    out["attention_maps"] = r
    print(f"{'attention_maps ' + str(a.n) + ' x 512':24s}: torch rows median {t['median_us']:9.1f} us (min {t['min_us']:9.1f}) peak "
          f"{t['peak_bytes'] / 2**20:8.1f} MiB   fused median {f['median_us']:9.1f} us (min {f['min_us']:9.1f}) peak "
          f"{f['peak_bytes'] / 2**20:8.1f} MiB   {'fused faster' if r['fused_is_faster'] else 'NOT faster'} "
          f"(x{t['median_us'] / f['median_us']:.2f} on the medians, x{t['peak_bytes'] / max(f['peak_bytes'], 1):.2f} on the peaks)")
    print(f"{'':24s}  the plain no-grad forward, same switches: median {p['median_us']:9.1f} us (min {p['min_us']:9.1f}) peak "
          f"{p['peak_bytes'] / 2**20:8.1f} MiB: the maps cost {r['over_forward_us']:.1f} us over it on the medians")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", action="store_true", help="time moc_nystrom_attention_rows and TransMIL.attention_maps, fused against the torch rows path")
    ap.add_argument("--train", action="store_true", help="time forward + backward: the torch path against fused_train, + fused_conv and + fused_pinv_train")
    ap.add_argument("--n", type=int, default=15000)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace-layers", type=int, default=0,
                    help="time nothing: run this many layers with fused + fused_pinv and exit (for a kernel trace of the layer)")
    a = ap.parse_args()
    assert a.iters >= 20
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    bag = torch.randn(a.n, 512, generator=g).to(dev)
    torch.manual_seed(1)
    model = TransMIL(n_classes=2, size_arg="conch").to(dev).eval()
    attn = model.layer1.attn
    out = {"n": a.n}
    if a.train or a.maps:
        (train if a.train else maps)(a, dev, g, bag, model, attn, out)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)
        return
    with torch.no_grad():
        side = math.ceil(math.sqrt(a.n))                                  # TransMIL pads the bag to a square, + class token
        n_tok = side * side + 1
        out["tokens"] = n_tok
        x = torch.nn.functional.layer_norm(torch.randn(1, n_tok, 512, generator=g), (512,)).to(dev)
        if a.trace_layers:
            attn.fused = attn.fused_pinv = True
            for _ in range(a.trace_layers):
                attn(x)
            torch.cuda.synchronize()
            return

        def flags(module):
            return lambda on, pv: (setattr(module, "fused", on), setattr(module, "fused_pinv", pv))
        out["model"] = pair(f"TransMIL {a.n} x 512", lambda: model(bag), flags(model), a.iters, a.warmup)
        out["layer"] = pair(f"one layer, {n_tok} tokens", lambda: attn(x), flags(attn), a.iters, a.warmup)

        n_pad = -(-n_tok // M) * M
        out["n_pad"] = n_pad
        qkv = attn.to_qkv(torch.nn.functional.pad(x, (0, 0, n_pad - n_tok, 0)))[0].contiguous()
        l = n_pad // M
        q_l = ((qkv[:, :512] * attn.scale).reshape(M, l, H, D).sum(1) / l).transpose(0, 1).contiguous()
        k_l = (qkv[:, 512:1024].reshape(M, l, H, D).sum(1) / l).transpose(0, 1).contiguous()
        Y = engine.nystrom_landmark_values(qkv, q_l)
        w = attn.res_conv.weight.reshape(H, TAPS).contiguous()
        scores = 2.0 * H * M * n_pad * D                                  # one [256, n] x 64 product per head
        out["landmark_values"] = kernel("moc_nystrom_landmark_values", lambda: engine.nystrom_landmark_values(qkv, q_l),
                                        2 * n_pad * 512 * 4, 2 * scores, a.iters, a.warmup)
        out["token_values"] = kernel("moc_nystrom_token_values", lambda: engine.nystrom_token_values(qkv, k_l, Y, w, attn.scale),
                                     3 * n_pad * 512 * 4, 2 * scores + 2.0 * n_pad * 512 * 48, a.iters, a.warmup)
        # the pseudo-inverse alone: 2 + 4 x 6 launches, each reading or writing two to three 2 MiB matrices (counted as 4 MiB
        # a launch), 24 products of 8 x 256^3 multiply-adds; beside it the torch function on the same attn2
        attn2 = (q_l @ k_l.transpose(-1, -2)).softmax(dim=-1).contiguous()
        its = attn.pinv_iterations
        out["pinv"] = kernel("moc_nystrom_pinv", lambda: engine.nystrom_pinv(attn2, its), (2 + 4 * its) * 4 * 2 ** 20,
                             4 * its * 2.0 * H * M ** 3, a.iters, a.warmup)
        out["pinv_torch"] = times_us(lambda: moore_penrose_iter_pinv(attn2.unsqueeze(0), its), a.iters, a.warmup)
        k, t = out["pinv"], out["pinv_torch"]
        out["pinv_is_faster"] = k["median_us"] < t["min_us"]
        print(f"{'moore_penrose_iter_pinv':24s}: median {t['median_us']:8.1f} us (min {t['min_us']:8.1f})   moc_nystrom_pinv "
              f"{'faster' if out['pinv_is_faster'] else 'NOT faster'} (x{t['median_us'] / k['median_us']:.2f} on the medians)")
        # the no-grad model pass with `fused` + `fused_pinv`, without and with `fused_ppeg` on top; pos_layer alone likewise
        model.fused = model.fused_pinv = True
        ppeg = model.pos_layer
        for key, fn in (("model", lambda: model(bag)), ("pos_layer", lambda: ppeg(x, side, side))):
            r = {}
            for on in (False, True):
                model.fused_ppeg = on
                r["fused_ppeg" if on else "torch_ppeg"] = times_us(fn, a.iters, a.warmup)
            t, f = r["torch_ppeg"], r["fused_ppeg"]
            r["fused_ppeg_is_faster"] = f["median_us"] < t["min_us"]
            out["nograd_ppeg_" + key] = r
            print(f"{'no-grad ' + key:24s}: torch pos_layer median {t['median_us']:9.1f} us (min {t['min_us']:9.1f})   fused_ppeg median "
                  f"{f['median_us']:9.1f} us (min {f['min_us']:9.1f})   {'fused_ppeg faster' if r['fused_ppeg_is_faster'] else 'NOT faster'} "
                  f"(x{t['median_us'] / f['median_us']:.2f} on the medians)")
        model.fused = model.fused_pinv = model.fused_ppeg = False
        ppeg_entries(ppeg, x, side, torch.randn(1, n_tok, 512, generator=g).to(dev), out, a.iters, a.warmup)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
