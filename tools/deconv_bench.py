#!/usr/bin/env python3
"""Sparse Deconvolution layers on the MI355X through plan option "deconv", beside the two routes that exist without it,
three routes per layer in the same call:

  deconv   option "deconv" = 1, KERNEL_AUTO: the inner stride-1 plan on the bottom + escoin_d2s_unpack_kernel (forward);
           escoin_d2s_pack_kernel + the inner plan's backward (data gradient)
  mirror   the route without the option: the MIRROR convolution's plan (M <-> C, H x W <-> OH x OW) with "s2d" = 1, and
           escoin_backward for bottom_diff alone with the activations as top_diff -- a deconvolution forward without bias
           and ReLU.  (Its data-gradient column is that plan's FORWARD: the deconvolution's data gradient is the mirror
           convolution itself.)
  torch    torch.nn.functional.conv_transpose2d on the dense weights (MIOpen), forward; its data gradient is conv2d

The routes alternate region by region, each region being `--reps` back-to-back calls between device events after a
warm-up; the median of `--regions` regions per route is reported with its spread (min .. max).  The forward of the "deconv"
route is also split into its inner launch and the unpack kernel alone (escoin_plan_d2s_unpack), timed the same way, and the
align times are the new plan's against the mirror route's three (outer + s2d inner, then the inner plan's transposed plan,
built by the first backward).

Decoder layers at 90 % sparsity: DCGAN 512 -> 256 k4 s2 p1 @ 8 x 8 and 256 -> 128 @ 16 x 16, U-Net 256 -> 128 k2 s2 @ 28 x 28,
FCN 21 -> 21 k4 s2 p1 g21 @ 34 x 34 and FCN 21 -> 21 k16 s8 @ 16 x 16.  --only keeps the layers whose name contains one of the
given substrings.  Prints one JSON line (progress on stderr); --markdown FILE also writes the tables of
profiles/deconv_mi355x.md.

    python tools/deconv_bench.py [--batch 64] [--only a,b] [--regions 7] [--reps 3] [--markdown FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402

# name: (C, M, H, W, K, stride, pad, group)
LAYERS = [
    ("dcgan_512_256_k4s2", 512, 256, 8, 8, 4, 2, 1, 1),
    ("dcgan_256_128_k4s2", 256, 128, 16, 16, 4, 2, 1, 1),
    ("unet_256_128_k2s2", 256, 128, 28, 28, 2, 2, 0, 1),
    ("fcn_21_k4s2_g21", 21, 21, 34, 34, 4, 2, 1, 21),
    ("fcn_21_k16s8", 21, 21, 16, 16, 16, 8, 0, 1),
]


def region(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def alternating(fns, regions, reps):
    """{name: sorted per-call times (us)}: `regions` rounds, each timing one region of every route in turn."""
    import torch
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(regions):
        for k, fn in fns.items():
            out[k].append(region(fn, reps))
    return {k: sorted(v) for k, v in out.items()}


def summary(ts):
    return dict(median_us=round(float(np.median(ts)), 1), min_us=round(ts[0], 1), max_us=round(ts[-1], 1))


def pruned(shape, sparsity, seed):
    rs = np.random.RandomState(seed)
    w = rs.uniform(-1, 1, shape).astype(np.float32)
    w[w == 0] = 0.5
    return w * (rs.uniform(0, 1, shape) >= sparsity)


def timed_ms(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def bench_layer(pkg, layer, n, regions, reps):
    import torch
    F = torch.nn.functional
    name, C, M, H, W, K, S, P, G = layer
    dev = torch.device("cuda:0")
    w = pruned((C, M // G, K, K), 0.9, 11)
    rs = np.random.RandomState(12)
    x = torch.from_numpy(rs.uniform(-1, 1, (n, C, H, W)).astype(np.float32)).to(dev)
    d = pkg.ConvDesc.deconvolution(n, C, H, W, M, K, S, P, G, bias=False)
    oh, ow = pkg.deconv_out_shape(d)
    td = torch.from_numpy(rs.uniform(-1, 1, (n, M, oh, ow)).astype(np.float32)).to(dev)
    top, bd = torch.empty_like(td), torch.empty_like(x)
    wd = torch.from_numpy(w).to(dev)
    # the new plan
    plan = pkg.Plan(d, deconv=1)
    align_new = timed_ms(lambda: plan.weight_align(w))
    assert plan.stat("deconv") == 1
    # the route without the option: the mirror convolution with "s2d", its backward as the forward
    md = pkg.ConvDesc(n, M, oh, ow, C, K, K, P, P, S, S, 1, 1, G, 0, 0)
    mirror = pkg.Plan(md, s2d=1)
    align_mirror = timed_ms(lambda: mirror.weight_align(w))
    align_mirror_bwd = timed_ms(lambda: mirror.backward(x, bottom_diff=top))      # builds the backward state: the transposed plan
    fwd = alternating(dict(deconv=lambda: plan.forward(x, None, top),
                           mirror=lambda: mirror.backward(x, bottom_diff=top),
                           torch=lambda: F.conv_transpose2d(x, wd, None, stride=S, padding=P, groups=G)), regions, reps)
    plan.backward(td, bottom_diff=bd)
    bwd = alternating(dict(deconv=lambda: plan.backward(td, bottom_diff=bd),
                           mirror=lambda: mirror.forward(td, None, bd),
                           torch=lambda: F.conv2d(td, wd, None, stride=S, padding=P, groups=G)), regions, reps)
    inner = plan.kernel_name.split(" + escoin_d2s_unpack_kernel")[0]
    split = alternating(dict(unpack=lambda: plan.d2s_unpack(top)), regions, reps)
    unpack_us = float(np.median(split["unpack"]))
    row = dict(layer=name, N=n, C=C, M=M, H=H, W=W, K=K, stride=S, pad=P, group=G, nnz=plan.nnz(), inner_kernel=inner,
               mirror_kernel=mirror.kernel_name,
               forward={k: summary(v) for k, v in fwd.items()}, backward={k: summary(v) for k, v in bwd.items()},
               unpack=dict(summary(split["unpack"]), top_bytes=top.numel() * 4, scratch_bytes=plan.stat("deconv_scratch_bytes"),
                           gbps=round((top.numel() * 4 + plan.stat("deconv_scratch_bytes")) / unpack_us * 1e-3, 1)),
               align_ms=dict(deconv=round(align_new, 2), mirror=round(align_mirror, 2), mirror_first_backward=round(align_mirror_bwd, 2)),
               workspace_bytes=dict(deconv=plan.workspace_bytes, mirror=mirror.workspace_bytes))
    plan.close(), mirror.close()
    return row


def markdown(rows, dev_name, regions, reps):
    out = ["Box: %s.  Median of %d regions of %d back-to-back calls per route, routes alternating (min .. max in brackets), us." % (dev_name, regions, reps), ""]
    for what in ("forward", "backward"):
        out += ["### %s" % ("Forward" if what == "forward" else "Data gradient"), "",
                "| layer | N | deconv | mirror route | torch (MIOpen, dense) | mirror / deconv | torch / deconv |", "|---|---|---|---|---|---|---|"]
        for r in rows:
            c = r[what]
            cell = lambda k: "%.0f (%.0f .. %.0f)" % (c[k]["median_us"], c[k]["min_us"], c[k]["max_us"])  # noqa: E731
            out.append("| %s | %d | %s | %s | %s | %.2fx | %.2fx |" % (r["layer"], r["N"], cell("deconv"), cell("mirror"), cell("torch"),
                                                                 c["mirror"]["median_us"] / c["deconv"]["median_us"],
                                                                 c["torch"]["median_us"] / c["deconv"]["median_us"]))
        out.append("")
    out += ["### The forward's split: inner launch and unpack", "",
            "| layer | inner kernel | forward us | unpack alone us | inner (difference) us | unpack GB/s |", "|---|---|---|---|---|---|"]
    for r in rows:
        f, u = r["forward"]["deconv"]["median_us"], r["unpack"]["median_us"]
        out.append("| %s | `%s` | %.0f | %.0f | %.0f | %.0f |" % (r["layer"], r["inner_kernel"], f, u, f - u, r["unpack"]["gbps"]))
    out += ["", "### Align times (wall, ms)", "",
            "| layer | nnz | deconv plan | mirror plan (outer + s2d inner) | mirror's first backward (transposed plan) | mirror total / deconv |",
            "|---|---|---|---|---|---|"]
    for r in rows:
        a = r["align_ms"]
        out.append("| %s | %d | %.1f | %.1f | %.1f | %.2fx |" % (r["layer"], r["nnz"], a["deconv"], a["mirror"], a["mirror_first_backward"],
                                                            (a["mirror"] + a["mirror_first_backward"]) / a["deconv"]))
    out.append("")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--only", default="")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--markdown", default="")
    args = ap.parse_args()
    import torch
    pkg = ge.load_package()
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        raise SystemExit("deconv_bench needs a HIP device")
    keep = [k for k in args.only.split(",") if k]
    rows = []
    for layer in LAYERS:
        if keep and not any(k in layer[0] for k in keep):
            continue
        print("[deconv_bench] %s" % layer[0], file=sys.stderr, flush=True)
        rows.append(bench_layer(pkg, layer, args.batch, max(args.regions, 5), args.reps))
    dev_name = torch.cuda.get_device_name(0)
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write(markdown(rows, dev_name, max(args.regions, 5), args.reps))
    print(json.dumps(dict(tool="deconv_bench", device=dev_name, batch=args.batch, regions=max(args.regions, 5), reps=args.reps, layers=rows)))


if __name__ == "__main__":
    main()
