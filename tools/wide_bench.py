#!/usr/bin/env python3
"""Wide sparse stride-1 layers on the MI355X with and without plan option "w2b", five routes per layer in the same call:

  w2b      option "w2b" = 1, everything else automatic: escoin_w2b_pack_kernel + the inner plan of N * S column strips +
           escoin_w2b_unpack_kernel (the shipped rule: the fewest strips)
  w2b128   the same with "w2b_strip" set to the widest strip whose input row Wi stays at or below 128 columns
  auto     "w2b" = 0, everything automatic: what a wide layer gets without the option
  generic  "w2b" = 0, kernel = backward_kernel = GENERIC
  dense    "w2b" = 0, kernel = DENSE, backward_kernel = BWD_MFMA, wgrad_kernel = MFMA

Forward, data gradient and (compact) weight gradient are timed each: the routes alternate region by region, a region being
`--reps` back-to-back calls between device events after a warm-up, and the median of `--regions` regions per route is
reported with its spread.  The three rearrangements alone (escoin_plan_w2b_pack of the bottom, _unpack into the top,
_unpack_sum into bottom_diff) are timed the same way, each beside a device-to-device copy of as many bytes as it WRITES; a
rearrangement's GB/s counts its source read once and its destination written once, a copy's its bytes read and written.

Layers at 90 % sparsity and batch 8 (--batch): the 3x3 layers of VGG-16 / FCN-8s conv1_2 to conv3_2 on a 500 x 500 image
(FCN pads the first layer by 100: 698, 349 and 175 columns -- the last is no wide layer and is listed as not served) and one
U-Net 3x3 layer at 568 columns without padding.  --only keeps the layers whose name contains one of the given substrings;
--tiny runs 4 -> 4 channels on 6 rows of the same widths.  Prints one JSON line (progress on stderr); --markdown FILE also
writes the tables of profiles/w2b_mi355x.md.

    python tools/wide_bench.py [--batch 8] [--only a,b] [--regions 5] [--reps 20] [--tiny] [--markdown FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import __graft_entry__ as ge  # noqa: E402
from dilated_bench import alternating, summary  # noqa: E402

ROUTES = ("w2b", "w2b128", "auto", "generic", "dense")


def layers(synth, n, tiny=False):
    sh = synth.shape
    full = [("fcn_conv1_2", 64, 698, 698, 64, 1), ("fcn_conv2_1", 64, 349, 349, 128, 1), ("fcn_conv2_2", 128, 349, 349, 128, 1),
            ("fcn_conv3_2", 256, 175, 175, 256, 1), ("unet_568", 64, 568, 568, 64, 0)]
    return [sh(("tiny_" if tiny else "") + name, n, 4 if tiny else c, 6 if tiny else h, w, 4 if tiny else m, 3, pad=pad, bias=False,
               sparsity=0.5 if tiny else 0.9) for name, c, h, w, m, pad in full]


def bench_layer(pkg, synth, s, regions, reps):
    import torch
    dev = torch.device("cuda:0")
    w = synth.pruned_weights(s, 11)
    x = torch.from_numpy(synth.activations(s, 12)).to(dev)
    oh, ow = synth.out_hw(s)
    td = torch.from_numpy(np.random.RandomState(21).uniform(-1, 1, (s.N, s.M, oh, ow)).astype(np.float32)).to(dev)
    top, bd = torch.empty_like(td), torch.empty_like(x)
    narrow = (128 - (s.KW - 1)) // 4 * 4
    routes = dict(w2b=dict(w2b=1), w2b128=dict(w2b=1, w2b_strip=narrow), auto=dict(),
                  generic=dict(kernel=pkg.KERNEL_GENERIC, backward_kernel=pkg.KERNEL_GENERIC),
                  dense=dict(kernel=pkg.KERNEL_DENSE, backward_kernel=pkg.BWD_MFMA, wgrad_kernel=pkg.WGRAD_MFMA))
    plans = {}
    for name in ROUTES:
        plans[name] = pkg.Plan(pkg.ConvDesc.from_shape(s), **routes[name])
        plans[name].weight_align(w)
    p = plans["w2b"]
    row = dict(layer=s.name, N=s.N, sparsity=s.sparsity, nnz=p.nnz(), W=s.W, OW=ow, served=p.stat("w2b"))
    if not row["served"]:
        for k in ("w2b", "w2b128"):
            plans.pop(k).close()
    vd = torch.zeros(row["nnz"], device=dev)
    ops = dict(forward=lambda q: q.forward(x, None, top), data_gradient=lambda q: q.backward(td, bottom_diff=bd),
               weight_gradient=lambda q: q.backward(td, bottom=x, bottom_diff=None, values_diff=vd))
    for what, op in ops.items():
        ts = alternating({k: (lambda q=q: op(q)) for k, q in plans.items()}, regions, reps)
        row[what] = {k: summary(v) for k, v in ts.items()}
    row["kernels"] = {k: dict(forward=q.kernel_name, data=q.stat("bwd_data_kernel"), wgrad=q.stat("wgrad_kernel"), strips=q.stat("w2b_strips"),
                              strip=q.stat("w2b_strip"), workspace_bytes=q.workspace_bytes) for k, q in plans.items()}
    if row["served"]:
        S, SW = p.stat("w2b_strips"), p.stat("w2b_strip")
        xs = torch.empty(s.N * S * s.C * s.H * (SW + s.KW - 1), device=dev)
        ts_ = torch.empty(s.N * S * s.M * oh * SW, device=dev)
        assert p.stat("w2b_scratch_bytes") == 4 * (2 * xs.numel() + ts_.numel())
        xs2, top2, bd2 = torch.empty_like(xs), torch.empty_like(top), torch.empty_like(bd)
        rr = alternating(dict(pack=lambda: p.w2b_pack(x, xs), pack_copy=lambda: xs2.copy_(xs), unpack=lambda: p.w2b_unpack(ts_, top),
                              unpack_copy=lambda: top2.copy_(top), unpack_sum=lambda: p.w2b_unpack_sum(xs, bd),
                              unpack_sum_copy=lambda: bd2.copy_(bd)), regions, reps)
        for k, src, dst in (("pack", x, xs), ("unpack", ts_, top), ("unpack_sum", xs, bd)):
            med, cmed = float(np.median(rr[k])), float(np.median(rr[k + "_copy"]))
            row[k] = dict(summary(rr[k]), src_bytes=src.numel() * 4, dst_bytes=dst.numel() * 4, gbps=round((src.numel() + dst.numel()) * 4 / med * 1e-3, 1),
                          copy_us=round(cmed, 1), copy_gbps=round(2 * dst.numel() * 4 / cmed * 1e-3, 1))
    for q in plans.values():
        q.close()
    return row


def markdown(rows, dev_name, regions, reps):
    out = ["Box: %s.  Median of %d regions of %d back-to-back calls per route, routes alternating (min .. max in brackets), us." % (dev_name, regions, reps), ""]
    for what in ("forward", "data_gradient", "weight_gradient"):
        out += ["### %s" % what.replace("_", " ").capitalize(), "", "| layer | batch | W | " + " | ".join(ROUTES) + " | best without / w2b |",
                "|---|---|---|" + "---|" * (len(ROUTES) + 1)]
        for r in rows:
            c = r[what]
            cell = lambda k: "%.0f (%.0f .. %.0f)" % (c[k]["median_us"], c[k]["min_us"], c[k]["max_us"]) if k in c else "not served"  # noqa: E731
            best = min(c[k]["median_us"] for k in ("auto", "generic", "dense"))
            out.append("| %s | %d | %d | %s | %s |" % (r["layer"], r["N"], r["W"], " | ".join(cell(k) for k in ROUTES),
                                                      "%.2fx" % (best / c["w2b"]["median_us"]) if "w2b" in c else "-"))
        out.append("")
    out += ["### Kernels per route (forward; bwd_data_kernel / wgrad_kernel; strips x strip width)", "", "| layer | route | kernels |", "|---|---|---|"]
    for r in rows:
        for k, v in r["kernels"].items():
            out.append("| %s | %s | `%s`; %d / %d; %d x %d |" % (r["layer"], k, v["forward"], v["data"], v["wgrad"], v["strips"], v["strip"]))
    out += ["", "### The rearrangements alone, beside a device-to-device copy of the bytes each writes", "",
            "| layer | kernel | source MB | destination MB | us | GB/s | copy us | copy GB/s | rate / copy rate |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        for k in ("pack", "unpack", "unpack_sum"):
            if k in r:
                v = r[k]
                out.append("| %s | %s | %.1f | %.1f | %.0f | %.0f | %.0f | %.0f | %.2f |" % (
                    r["layer"], k, v["src_bytes"] / 1e6, v["dst_bytes"] / 1e6, v["median_us"], v["gbps"], v["copy_us"], v["copy_gbps"], v["gbps"] / v["copy_gbps"]))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--only", default="")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--markdown", default="")
    args = ap.parse_args()
    import torch
    pkg = ge.load_package()
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        raise SystemExit("wide_bench needs a HIP device")
    keep = [k for k in args.only.split(",") if k]
    rows = []
    for s in layers(pkg.synth, args.batch, args.tiny):
        if keep and not any(k in s.name for k in keep):
            continue
        print("[wide_bench] %s batch %d" % (s.name, args.batch), file=sys.stderr, flush=True)
        rows.append(bench_layer(pkg, pkg.synth, s, max(args.regions, 5), args.reps))
    dev_name = torch.cuda.get_device_name(0)
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write(markdown(rows, dev_name, max(args.regions, 5), args.reps))
    print(json.dumps(dict(tool="wide_bench", device=dev_name, batch=args.batch, regions=max(args.regions, 5), reps=args.reps, layers=rows)))


if __name__ == "__main__":
    main()
