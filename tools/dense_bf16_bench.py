#!/usr/bin/env python3
"""The dense forward kernel with plan option "dense_math" at 0 (fp32 products, escoin_dense_mfma_kernel: the baseline), at 1
(escoin_dense_bf16_kernel) and with option "dense_split" at 1 (escoin_dense_bf16x3_kernel: route `split`), in the same call on
the MI355X: ONE plan under KERNEL_DENSE and one pair of blobs per layer, the options flipped between regions -- they hold no
state, so nothing is re-aligned.

Layers: the five shapes of profiles/r06_dense_stamps.md (tools/dense_stamps.py SHAPES) and the distinct dense 1x1 layers of
`tools/caffe_test.py --model resnet50_chain`, at one batch.  The three settings alternate region by region, each region being
`--reps` back-to-back forwards between device events after a warm-up; the median of `--regions` regions per setting is
reported in milliseconds with its spread, and as TFLOP/s (2 * N * OH * OW * M * K / time: the layer's dense operations).
Accuracy: the first two images of the bf16 result against the float64 convolution of the operands rounded to bf16, as the worst
ratio to the fp32 accumulation bound B = gamma(K + 4) * sum |w| |x| + (K + 4) * 2^-149 (tools/error_bound.py forward_bound); of
the split result against the float64 convolution of the UNROUNDED operands, as the worst ratio to 2^-16 * sum |w| |x| + 3 B
(include/escoin.h option "dense_split"); and, for scale, the largest |result - fp32 result| relative to the largest output of
either.  Prints one JSON line (progress on stderr); --markdown FILE also writes the table of profiles/dense_split_mi355x.md.

    python tools/dense_bf16_bench.py [--batch 256] [--only a,b] [--regions 7] [--reps 5] [--markdown FILE]
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
from caffe_test import resnet50_chain  # noqa: E402
from dense_stamps import SHAPES  # noqa: E402
from depthwise_bench import alternating, summary  # noqa: E402
from error_bound import TINY, U32, gamma  # noqa: E402


def layers(synth, batch):
    out = [synth.shape(name, batch, c, hw, hw, m, 1, stride=stride, bias=False, sparsity=0.0) for name, c, hw, m, stride in SHAPES]
    seen = {(s.C, s.H, s.M, s.stride_h) for s in out}
    for name, kind, s, _, _ in resnet50_chain(synth, batch, 0.9):
        key = (s.C, s.H, s.M, s.stride_h)
        if kind == "dense" and key not in seen:
            seen.add(key)
            out.append(s)
    return out


def bench(pkg, synth, s, regions, reps):
    import torch
    import torch.nn.functional as F
    dev = torch.device("cuda:0")
    w = synth.pruned_weights(s, 11)
    x = torch.from_numpy(synth.activations(s, 12)).to(dev)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s), kernel=pkg.KERNEL_DENSE)
    plan.weight_align(w)
    top = plan.forward(x)

    def run(math, split=0):
        plan.set_option("dense_math", math)
        plan.set_option("dense_split", split)
        plan.forward(x, None, top)
    t = alternating({"fp32": lambda: run(0), "bf16": lambda: run(1), "split": lambda: run(0, 1)}, regions, reps)
    run(0)
    v32, ref = plan.stat("dense_variant"), top[:2].clone()
    run(0, 1)
    torch.cuda.synchronize()
    assert plan.stat("dense_split") == 1 and plan.stat("dense_variant") == (v32 & ~16) + 128, (v32, plan.stat("dense_variant"))   # (16: stream-K, fp32 only)
    top3 = top[:2].clone()
    run(1)
    torch.cuda.synchronize()
    assert plan.stat("dense_math") == 1 and plan.stat("dense_split") == 0 and plan.stat("dense_variant") >= 32 and v32 < 32
    rnd = lambda a: a.to(torch.bfloat16).to(torch.float64)  # noqa: E731
    conv = lambda a, b: F.conv2d(a, b, stride=(s.stride_h, s.stride_w), padding=(s.pad_h, s.pad_w), groups=s.group)  # noqa: E731
    wr, xr = rnd(torch.from_numpy(w).to(dev)), rnd(x[:2])
    k = float(s.C // s.group * s.KH * s.KW + 4)
    bound = float(gamma(k, U32)) * conv(xr.abs(), wr.abs()) + k * TINY
    ratio = float(((top[:2].double() - conv(xr, wr)).abs() / bound).max())
    rel32 = float((top[:2] - ref).abs().max() / ref.abs().max())
    w64, x64 = torch.from_numpy(w).to(dev).double(), x[:2].double()
    mag = conv(x64.abs(), w64.abs())
    ratio3 = float(((top3.double() - conv(x64, w64)).abs() / (2.0 ** -16 * mag + 3.0 * (float(gamma(k, U32)) * mag + k * TINY))).max())
    rel3 = float((top3 - ref).abs().max() / ref.abs().max())
    oh, ow = synth.out_hw(s)
    flop = 2.0 * s.N * oh * ow * s.M * (s.C // s.group) * s.KH * s.KW
    row = dict(layer=s.name, C=s.C, HW=s.H, M=s.M, stride=s.stride_h, K=s.C // s.group * s.KH * s.KW, variant_fp32=v32,
               variant_bf16=plan.stat("dense_variant"), ms={m: summary(v) for m, v in t.items()},
               tflops={m: round(flop / (float(np.median(v)) * 1e-3) / 1e12, 1) for m, v in t.items()},
               worst_err_over_bound=ratio, max_rel_to_fp32=rel32, split_worst_err_over_bound=ratio3, split_max_rel_to_fp32=rel3)
    plan.close()
    return row


def markdown(rows, dev_name, batch, regions, reps):
    out = ["Box: %s, batch %d.  Median of %d regions of %d back-to-back forwards per setting, settings alternating (min .. max in "
           "brackets), ms." % (dev_name, batch, regions, reps), "",
           "| layer | C @ HxW -> M, stride | K | variant fp32 | fp32 ms | bf16 ms | split ms | TFLOP/s fp32 / bf16 / split | fp32 / bf16 | fp32 / split | "
           "bf16 / split | err / bound bf16, split | max rel. to fp32 bf16, split |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        cell = lambda m: "%.3f (%.3f .. %.3f)" % (r["ms"][m]["median_ms"], r["ms"][m]["min_ms"], r["ms"][m]["max_ms"])  # noqa: E731
        med = {m: r["ms"][m]["median_ms"] for m in ("fp32", "bf16", "split")}
        out.append("| %s | %d @ %dx%d -> %d, s%d | %d | %d | %s | %s | %s | %.1f / %.1f / %.1f | %.2fx | %.2fx | %.2fx | %.3f, %.3f | %.1e, %.1e |" % (
            r["layer"], r["C"], r["HW"], r["HW"], r["M"], r["stride"], r["K"], r["variant_fp32"], cell("fp32"), cell("bf16"), cell("split"),
            r["tflops"]["fp32"], r["tflops"]["bf16"], r["tflops"]["split"], med["fp32"] / med["bf16"], med["fp32"] / med["split"],
            med["bf16"] / med["split"], r["worst_err_over_bound"], r["split_worst_err_over_bound"], r["max_rel_to_fp32"], r["split_max_rel_to_fp32"]))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--only", default="")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--markdown", default=None)
    args = ap.parse_args()
    pkg = ge.load_package()
    import torch
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        sys.exit("dense_bf16_bench: no HIP device visible (a measurement needs the MI355X)")
    synth = pkg.synth
    only = set(filter(None, args.only.split(",")))
    rows = []
    for s in layers(synth, args.batch):
        if only and s.name not in only:
            continue
        rows.append(bench(pkg, synth, s, args.regions, args.reps))
        print("[dense_bf16_bench] %s" % json.dumps(rows[-1]), file=sys.stderr)
    dev_name = torch.cuda.get_device_name(0)
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write(markdown(rows, dev_name, args.batch, args.regions, args.reps))
    print(json.dumps(dict(tool="dense_bf16_bench", device=dev_name, batch=args.batch, regions=args.regions, reps=args.reps, rows=rows)))


if __name__ == "__main__":
    main()
