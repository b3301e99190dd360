#!/usr/bin/env python3
"""Plan option "sp24" (escoin_dense_sp24_kernel, v_smfmac_f32_32x32x32_bf16) against the other routes a 2:4-pruned layer can
take, in the same call on the MI355X.  Weights: synth.pattern_2of4 of dense weights (50 % zeros, 2 of every 4 along a row).

Routes per layer: KERNEL_DENSE with fp32 products ("fp32"), with "dense_math" = 1 ("bf16") and with "sp24" = 1 ("sp24") -- ONE
plan, aligned with the option so that the index table exists, the options flipped between regions -- and a second plan under
KERNEL_AUTO ("auto": the sparse route the library picks for these weights by itself; its kernel is reported).

Layers: the pointwise (stride-1 1x1) layers of `tools/caffe_test.py --model resnet50_chain` and the four 3x3 shapes of
synth.resnet50_3x3, at one batch.  The routes alternate region by region, each region being `--reps` back-to-back forwards
between device events after a warm-up; the median of `--regions` regions per route is reported in milliseconds with its
spread, and as TFLOP/s of the DENSE problem (2 * N * OH * OW * M * K / time).  Prints one JSON line (progress on stderr);
--markdown FILE also writes the table of profiles/sp24_mi355x.md.

    python tools/sp24_bench.py [--batch 256] [--only a,b] [--regions 7] [--reps 5] [--markdown FILE]
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
from depthwise_bench import alternating, summary  # noqa: E402

ROUTES = ("fp32", "bf16", "sp24", "auto")


def layers(synth, batch):
    out, seen = [], set()
    for name, kind, s, _, _ in resnet50_chain(synth, batch, 0.5):
        key = (s.C, s.H, s.M)
        if s.KH == 1 and s.stride_h == 1 and key not in seen:
            seen.add(key)
            out.append(s._replace(name="pw%d_%d_to%d" % key, sparsity=0.5))
    return out + [s._replace(sparsity=0.5) for s in synth.resnet50_3x3(batch)]


def bench(pkg, synth, s, regions, reps):
    import torch
    dev = torch.device("cuda:0")
    w = synth.pattern_2of4(synth.pruned_weights(s._replace(sparsity=0.0), 11))
    x = torch.from_numpy(synth.activations(s, 12)).to(dev)
    desc = pkg.ConvDesc.from_shape(s)
    plan, auto = pkg.Plan(desc, kernel=pkg.KERNEL_DENSE, sp24=1), pkg.Plan(desc)
    plan.weight_align(w)
    auto.weight_align(w)
    assert plan.stat("sp24_pattern") == 1
    top = plan.forward(x)

    def run(math, sp):
        plan.set_option("dense_math", math)
        plan.set_option("sp24", sp)
        plan.forward(x, None, top)
    t = alternating({"fp32": lambda: run(0, 0), "bf16": lambda: run(1, 0), "sp24": lambda: run(0, 1),
                     "auto": lambda: auto.forward(x, None, top)}, regions, reps)
    run(0, 0)
    ref = top[:2].clone()
    run(0, 1)
    torch.cuda.synchronize()
    assert plan.stat("dense_sp24") == 1 and plan.stat("dense_variant") >= 64
    rel32 = float((top[:2] - ref).abs().max() / ref.abs().max())
    oh, ow = synth.out_hw(s)
    k = s.C // s.group * s.KH * s.KW
    flop = 2.0 * s.N * oh * ow * s.M * k
    row = dict(layer=s.name, C=s.C, HW=s.H, M=s.M, KH=s.KH, K=k, variant_sp24=plan.stat("dense_variant"), auto_kernel=auto.kernel_name,
               ms={m: summary(v) for m, v in t.items()},
               tflops={m: round(flop / (float(np.median(v)) * 1e-3) / 1e12, 1) for m, v in t.items()}, max_rel_to_fp32=rel32)
    plan.close()
    auto.close()
    return row


def markdown(rows, dev_name, batch, regions, reps):
    out = ["Box: %s, batch %d, 2:4 weights.  Median of %d regions of %d back-to-back forwards per route, routes alternating (min .. "
           "max in brackets), ms; TFLOP/s of the dense problem." % (dev_name, batch, regions, reps), "",
           "| layer | C @ HxW -> M, kernel | K | fp32 ms | bf16 ms | sp24 ms | auto ms | TFLOP/s fp32 / bf16 / sp24 / auto | bf16 / sp24 | "
           "best other / sp24 | KERNEL_AUTO ran | max rel. to fp32 |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        med = {m: r["ms"][m]["median_ms"] for m in ROUTES}
        cell = lambda m: "%.3f (%.3f .. %.3f)" % (med[m], r["ms"][m]["min_ms"], r["ms"][m]["max_ms"])  # noqa: E731
        out.append("| %s | %d @ %dx%d -> %d, %dx%d | %d | %s | %s | %s | %s | %s | %.2fx | %.2fx | %s | %.1e |" % (
            r["layer"], r["C"], r["HW"], r["HW"], r["M"], r["KH"], r["KH"], r["K"], cell("fp32"), cell("bf16"), cell("sp24"), cell("auto"),
            " / ".join("%.1f" % r["tflops"][m] for m in ROUTES), med["bf16"] / med["sp24"],
            min(med["fp32"], med["bf16"], med["auto"]) / med["sp24"], r["auto_kernel"], r["max_rel_to_fp32"]))
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
        sys.exit("sp24_bench: no HIP device visible (a measurement needs the MI355X)")
    synth = pkg.synth
    only = set(filter(None, args.only.split(",")))
    rows = []
    for s in layers(synth, args.batch):
        if only and s.name not in only:
            continue
        rows.append(bench(pkg, synth, s, args.regions, args.reps))
        print("[sp24_bench] %s" % json.dumps(rows[-1]), file=sys.stderr)
    dev_name = torch.cuda.get_device_name(0)
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write(markdown(rows, dev_name, args.batch, args.regions, args.reps))
    print(json.dumps(dict(tool="sp24_bench", device=dev_name, batch=args.batch, regions=args.regions, reps=args.reps, rows=rows)))


if __name__ == "__main__":
    main()
