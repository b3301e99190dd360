#!/usr/bin/env python3
"""Strided sparse layers on the MI355X with and without plan option "s2d", four routes per layer in the same call:

  s2d      option "s2d" = 1, KERNEL_AUTO: escoin_s2d_pack_kernel + the inner stride-1 plan (forward), the inner plan's
           backward + escoin_s2d_unpack_kernel (data gradient)
  generic  "s2d" = 0, kernel = backward_kernel = GENERIC: the generic forward kernel and the gather data gradient
  dense    "s2d" = 0, kernel = DENSE, backward_kernel = BWD_MFMA: the dense MFMA forward and the MFMA data gradient
  auto     "s2d" = 0, everything automatic: what a strided layer gets today

The routes alternate region by region (s2d, generic, dense, auto, s2d, ...), each region being `--reps` back-to-back
calls between device events after a warm-up; the median of `--regions` regions per route is reported with its spread
(min .. max), forward and data gradient each.  The pack kernel alone (escoin_plan_s2d_pack) is timed the same way beside a
device-to-device copy of X''s bytes in the same process; its GB/s counts the bottom read once and X' written once, the
copy's counts its bytes read and written.

Layers at batch 256, 90 % sparsity: conv2 of res3a / res4a / res5a of ResNet-50 v1.5, the three down-sampling 3x3 layers
of ResNet-18 and, at 50 % sparsity, a 7x7 stride-2 stem.  --only keeps the layers whose name contains one of the given
substrings.  Prints one JSON line (progress on stderr); --markdown FILE also writes the tables of profiles/s2d_mi355x.md.

    python tools/strided_bench.py [--batch 256] [--only a,b] [--regions 7] [--reps 3] [--markdown FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402


def layers(synth, n):
    sh = synth.shape
    return [
        sh("r50_res3a_conv2", n, 128, 56, 56, 128, 3, pad=1, stride=2, bias=False, sparsity=0.9),
        sh("r50_res4a_conv2", n, 256, 28, 28, 256, 3, pad=1, stride=2, bias=False, sparsity=0.9),
        sh("r50_res5a_conv2", n, 512, 14, 14, 512, 3, pad=1, stride=2, bias=False, sparsity=0.9),
        sh("r18_layer2_down", n, 64, 56, 56, 128, 3, pad=1, stride=2, bias=False, sparsity=0.9),
        sh("r18_layer3_down", n, 128, 28, 28, 256, 3, pad=1, stride=2, bias=False, sparsity=0.9),
        sh("r18_layer4_down", n, 256, 14, 14, 512, 3, pad=1, stride=2, bias=False, sparsity=0.9),
        sh("stem_7x7_s2", n, 3, 224, 224, 64, 7, pad=3, stride=2, bias=False, sparsity=0.5),
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


def bench_layer(pkg, synth, s, regions, reps):
    import torch
    dev = torch.device("cuda:0")
    w = synth.pruned_weights(s, 11)
    x = torch.from_numpy(synth.activations(s, 12)).to(dev)
    oh, ow = synth.out_hw(s)
    td = torch.from_numpy(np.random.RandomState(21).uniform(-1, 1, (s.N, s.M, oh, ow)).astype(np.float32)).to(dev)
    top, bd = torch.empty_like(td), torch.empty_like(x)
    routes = dict(s2d=dict(s2d=1), generic=dict(kernel=pkg.KERNEL_GENERIC, backward_kernel=pkg.KERNEL_GENERIC),
                  dense=dict(kernel=pkg.KERNEL_DENSE, backward_kernel=pkg.BWD_MFMA), auto=dict())
    plans = {}
    for name, opts in routes.items():
        plans[name] = pkg.Plan(pkg.ConvDesc.from_shape(s), **opts)
        plans[name].weight_align(w)
    fwd = alternating({k: (lambda p=p: p.forward(x, None, top)) for k, p in plans.items()}, regions, reps)
    bwd = alternating({k: (lambda p=p: p.backward(td, bottom_diff=bd)) for k, p in plans.items()}, regions, reps)
    p = plans["s2d"]
    assert p.stat("s2d") == 1
    xi_bytes = p.stat("s2d_scratch_bytes")
    a, b = torch.empty(xi_bytes // 4, device=dev), torch.empty(xi_bytes // 4, device=dev)
    pk = alternating(dict(pack=lambda: p.s2d_pack(x), copy=lambda: b.copy_(a)), regions, reps)
    pack_us, copy_us = float(np.median(pk["pack"])), float(np.median(pk["copy"]))
    row = dict(layer=s.name, N=s.N, sparsity=s.sparsity, nnz=p.nnz(),
               forward={k: dict(summary(v), kernel=plans[k].kernel_name) for k, v in fwd.items()},
               backward={k: dict(summary(v), kernel=plans[k].stat("bwd_data_kernel")) for k, v in bwd.items()},
               pack=dict(summary(pk["pack"]), bottom_bytes=x.numel() * 4, xi_bytes=xi_bytes,
                         gbps=round((x.numel() * 4 + xi_bytes) / pack_us * 1e-3, 1)),
               copy=dict(summary(pk["copy"]), gbps=round(2 * xi_bytes / copy_us * 1e-3, 1)),
               s2d_workspace_bytes=p.workspace_bytes, auto_workspace_bytes=plans["auto"].workspace_bytes)
    for q in plans.values():
        q.close()
    return row


def markdown(rows, dev_name, regions, reps):
    out = ["Box: %s.  Median of %d regions of %d back-to-back calls per route, routes alternating (min .. max in brackets), us." % (dev_name, regions, reps), ""]
    for what in ("forward", "backward"):
        out += ["### %s" % ("Forward" if what == "forward" else "Data gradient"), "",
                "| layer | s2d | generic | dense | auto (s2d = 0) | s2d vs auto |", "|---|---|---|---|---|---|"]
        for r in rows:
            c = r[what]
            cell = lambda k: "%.0f (%.0f .. %.0f)" % (c[k]["median_us"], c[k]["min_us"], c[k]["max_us"])  # noqa: E731
            out.append("| %s | %s | %s | %s | %s | %.2fx |" % (r["layer"], cell("s2d"), cell("generic"), cell("dense"), cell("auto"),
                                                              c["auto"]["median_us"] / c["s2d"]["median_us"]))
        out.append("")
    out += ["### The pack kernel beside a device-to-device copy of X''s bytes", "",
            "| layer | bottom MB | X' MB | pack us | pack GB/s | copy us | copy GB/s | pack / copy rate |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append("| %s | %.1f | %.1f | %.0f | %.0f | %.0f | %.0f | %.2f |" % (
            r["layer"], r["pack"]["bottom_bytes"] / 1e6, r["pack"]["xi_bytes"] / 1e6, r["pack"]["median_us"], r["pack"]["gbps"],
            r["copy"]["median_us"], r["copy"]["gbps"], r["pack"]["gbps"] / r["copy"]["gbps"]))
    out.append("")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--only", default="")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--markdown", default="")
    args = ap.parse_args()
    import torch
    pkg = ge.load_package()
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        raise SystemExit("strided_bench needs a HIP device")
    keep = [k for k in args.only.split(",") if k]
    rows = []
    for s in layers(pkg.synth, args.batch):
        if keep and not any(k in s.name for k in keep):
            continue
        print("[strided_bench] %s" % s.name, file=sys.stderr, flush=True)
        rows.append(bench_layer(pkg, pkg.synth, s, max(args.regions, 5), args.reps))
    dev_name = torch.cuda.get_device_name(0)
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write(markdown(rows, dev_name, max(args.regions, 5), args.reps))
    print(json.dumps(dict(tool="strided_bench", device=dev_name, batch=args.batch, regions=max(args.regions, 5), reps=args.reps, layers=rows)))


if __name__ == "__main__":
    main()
