#!/usr/bin/env python3
"""The depthwise layers of MobileNet-v1 on the MI355X with and without plan option "depthwise", in the same call: the 13
layers of synth.mobilenet_dw (9 distinct shapes) at one batch, unpruned and with half the taps pruned, forward and data
gradient, four routes each:

  on       option "depthwise" = 1 under AUTO: escoin_depthwise_kernel / escoin_depthwise_dgrad_kernel (the stats are asserted)
  auto     the option off, "kernel" / "backward_kernel" at AUTO  -- the code the option does not touch: the baseline
  generic  the option off, "kernel" / "backward_kernel" forced to KERNEL_GENERIC
  torch    torch.nn.functional.conv2d(groups=C) on the dense weights, and its input gradient

The routes alternate region by region, each region being `--reps` back-to-back calls between device events after a warm-up;
the median of `--regions` regions per route is reported in milliseconds with its spread, and for "on" the fraction of the HBM
roofline: synth.algorithmic_bytes over HBM_PEAK over the time.  The outputs of "on" and "generic" are compared bit for bit
at the timed size.  Prints one JSON line (progress on stderr); --markdown FILE also writes the tables of
profiles/depthwise_mi355x.md.

--sets wgrad times the weight + bias gradient instead (plan option "wgrad_depthwise"; the tables of
profiles/depthwise_wgrad_mi355x.md), by the same method, three routes:

  on       option "wgrad_depthwise" = 1: escoin_depthwise_wgrad_kernel, then the tree sum (stat "wgrad_kernel" asserted to read 5)
  off      the same plan on the same build with the option off: the kernel AUTO picks (named per layer) -- the baseline
  torch    aten.convolution_backward's weight and bias gradient of conv2d(groups=C)

"on" and "off" sum in different orders: their largest difference, relative to the largest gradient, is reported.

    python tools/depthwise_bench.py [--sets forward,wgrad] [--batch 64] [--only a,b] [--regions 7] [--reps 5] [--markdown FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402

HBM_PEAK = 8.0e12     # bytes / s, the MI355X's HBM3E


def region(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def alternating(fns, regions, reps):
    """{name: sorted per-call times (ms)}: `regions` rounds, each timing one region of every route in turn."""
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
    return dict(median_ms=round(float(np.median(ts)), 4), min_ms=round(ts[0], 4), max_ms=round(ts[-1], 4))


def bench_layer(pkg, synth, s, regions, reps):
    import torch
    dev = torch.device("cuda:0")
    w = synth.pruned_weights(s, 11)
    x = torch.from_numpy(synth.activations(s, 12)).to(dev)
    oh, ow = synth.out_hw(s)
    td = torch.from_numpy(synth.uniform(21, s.N * s.M * oh * ow).reshape(s.N, s.M, oh, ow)).to(dev)
    b = torch.from_numpy(synth.bias_vector(s, 13)).to(dev)
    wd = torch.from_numpy(w).to(dev)
    desc = pkg.ConvDesc.from_shape(s)
    plans = dict(on=pkg.Plan(desc, depthwise=1), auto=pkg.Plan(desc),
                 generic=pkg.Plan(desc, kernel=pkg.KERNEL_GENERIC, backward_kernel=pkg.KERNEL_GENERIC))
    for p in plans.values():
        p.weight_align(w)
    tops = {k: torch.empty_like(td) for k in plans}
    bds = {k: torch.empty_like(x) for k in plans}
    F = torch.nn.functional
    fwd = {k: (lambda p=p, k=k: p.forward(x, b, tops[k])) for k, p in plans.items()}
    fwd["torch"] = lambda: F.conv2d(x, wd, b, stride=(s.stride_h, s.stride_w), padding=(s.pad_h, s.pad_w), groups=s.group)
    tf = alternating(fwd, regions, reps)
    bwd = {k: (lambda p=p, k=k: p.backward(td, bottom_diff=bds[k])) for k, p in plans.items()}
    bwd["torch"] = lambda: torch.ops.aten.convolution_backward(td, x, wd, None, (s.stride_h, s.stride_w), (s.pad_h, s.pad_w), (1, 1), False,
                                                               (0, 0), s.group, (True, False, False))
    tb = alternating(bwd, regions, reps)
    torch.cuda.synchronize()
    on = plans["on"]
    assert on.stat("depthwise") == 1 and on.stat("bwd_data_kernel") == pkg.BWD_DEPTHWISE
    same = bool(torch.equal(tops["on"], tops["generic"]) and torch.equal(bds["on"], bds["generic"]))
    floor_ms = synth.algorithmic_bytes(s) / HBM_PEAK * 1e3
    row = dict(layer=s.name, count=s.count, N=s.N, C=s.C, HW=s.H, stride=s.stride_h, nnz=on.nnz(), alg_mbytes=round(synth.algorithmic_bytes(s) / 1e6, 1),
               band_rows=on.stat("depthwise_band_rows"), lds_bytes=on.stat("depthwise_lds_bytes"), dgrad_lds_bytes=on.stat("dgrad_lds_bytes"),
               kernels=dict(auto=plans["auto"].kernel_name, auto_bwd=plans["auto"].stat("bwd_data_kernel")),
               forward={k: summary(v) for k, v in tf.items()}, backward={k: summary(v) for k, v in tb.items()},
               roofline=dict(forward=round(floor_ms / float(np.median(tf["on"])), 3), backward=round(floor_ms / float(np.median(tb["on"])), 3)),
               bits_equal_generic=same)
    for p in plans.values():
        p.close()
    return row


WGRAD_NAMES = {1: "entry", 2: "staged", 3: "mfma", 4: "pointwise", 5: "depthwise"}


def bench_wgrad(pkg, synth, s, regions, reps):
    import torch
    dev = torch.device("cuda:0")
    w = synth.pruned_weights(s, 11)
    x = torch.from_numpy(synth.activations(s, 12)).to(dev)
    oh, ow = synth.out_hw(s)
    td = torch.from_numpy(synth.uniform(21, s.N * s.M * oh * ow).reshape(s.N, s.M, oh, ow)).to(dev)
    wd = torch.from_numpy(w).to(dev)
    desc = pkg.ConvDesc.from_shape(s)
    plans = dict(on=pkg.Plan(desc, wgrad_depthwise=1), off=pkg.Plan(desc))
    for p in plans.values():
        p.weight_align(w)
    # (the gradients accumulate: the blobs are zeroed once, and compared after one call each on fresh ones)
    gw = {k: torch.zeros_like(wd) for k in plans}
    gb = {k: torch.zeros(s.M, device=dev) for k in plans}
    fns = {k: (lambda p=p, k=k: p.backward(td, bottom=x, bottom_diff=None, weight_diff=gw[k], bias_diff=gb[k])) for k, p in plans.items()}
    fns["torch"] = lambda: torch.ops.aten.convolution_backward(td, x, wd, [s.M], (s.stride_h, s.stride_w), (s.pad_h, s.pad_w), (1, 1), False,
                                                               (0, 0), s.group, (False, True, True))
    t = alternating(fns, regions, reps)
    torch.cuda.synchronize()
    on, off = plans["on"], plans["off"]
    assert on.stat("wgrad_kernel") == pkg.WGRAD_DEPTHWISE == 5 and off.stat("wgrad_kernel") != 5
    one = {k: p.backward(td, bottom=x, bottom_diff=None, weight_diff=True, bias_diff=True)[1:] for k, p in plans.items()}
    diff = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(one["on"], one["off"]))
    floor_ms = synth.algorithmic_bytes(s) / HBM_PEAK * 1e3
    row = dict(layer=s.name, count=s.count, N=s.N, C=s.C, HW=s.H, stride=s.stride_h, nnz=on.nnz(), alg_mbytes=round(synth.algorithmic_bytes(s) / 1e6, 1),
               slices=on.stat("wgrad_depthwise_slices"), lds_bytes=on.stat("wgrad_lds_bytes"), off_kernel=WGRAD_NAMES[off.stat("wgrad_kernel")],
               off_chunks=off.stat("bwd_chunks"), wgrad={k: summary(v) for k, v in t.items()},
               roofline=round(floor_ms / float(np.median(t["on"])), 3), max_rel_diff=diff)
    for p in plans.values():
        p.close()
    return row


def markdown_wgrad(results, dev_name, regions, reps):
    out = ["Box: %s.  Median of %d regions of %d back-to-back calls per route, routes alternating (min .. max in brackets), ms."
           % (dev_name, regions, reps), ""]
    for sparsity, rows in results:
        out += ["### Weight + bias gradient, %d %% of the taps pruned" % round(sparsity * 100), "",
                "| layer | x | alg. MB | slices | on | off | off: AUTO's kernel (chunks) | torch | off / on | torch / on | on: of the HBM roofline | max rel. on - off |",
                "|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            c = r["wgrad"]
            cell = lambda k: "%.3f (%.3f .. %.3f)" % (c[k]["median_ms"], c[k]["min_ms"], c[k]["max_ms"])  # noqa: E731
            m = lambda k: c[k]["median_ms"] / c["on"]["median_ms"]  # noqa: E731
            out.append("| %s | %d | %.1f | %d | %s | %s | %s (%d) | %s | %.2fx | %.2fx | %.0f %% | %.1e |" % (
                r["layer"], r["count"], r["alg_mbytes"], r["slices"], cell("on"), cell("off"), r["off_kernel"], r["off_chunks"], cell("torch"),
                m("off"), m("torch"), 100 * r["roofline"], r["max_rel_diff"]))
        out.append("")
    return "\n".join(out)


def markdown(results, dev_name, regions, reps):
    out = ["Box: %s.  Median of %d regions of %d back-to-back calls per route, routes alternating (min .. max in brackets), ms."
           % (dev_name, regions, reps), ""]
    for sparsity, rows in results:
        for what, title in (("forward", "Forward"), ("backward", "Data gradient")):
            out += ["### %s, %d %% of the taps pruned" % (title, round(sparsity * 100)), "",
                    "| layer | x | alg. MB | band | on | off, AUTO | off, GENERIC | torch | AUTO / on | GENERIC / on | torch / on | on: of the HBM roofline | bits = GENERIC |",
                    "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
            for r in rows:
                c = r[what]
                cell = lambda k: "%.3f (%.3f .. %.3f)" % (c[k]["median_ms"], c[k]["min_ms"], c[k]["max_ms"])  # noqa: E731
                m = lambda k: c[k]["median_ms"] / c["on"]["median_ms"]  # noqa: E731
                out.append("| %s | %d | %.1f | %d | %s | %s | %s | %s | %.2fx | %.2fx | %.2fx | %.0f %% | %s |" % (
                    r["layer"], r["count"], r["alg_mbytes"], r["band_rows"], cell("on"), cell("auto"), cell("generic"), cell("torch"),
                    m("auto"), m("generic"), m("torch"), 100 * r["roofline"][what], "yes" if r["bits_equal_generic"] else "NO"))
            out.append("")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--only", default="")
    ap.add_argument("--sets", default="forward", help="forward (and data gradient), wgrad, or both: forward,wgrad")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--markdown", default="")
    args = ap.parse_args()
    import torch
    pkg = ge.load_package()
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        raise SystemExit("depthwise_bench needs a HIP device")
    synth = pkg.synth
    keep = [k for k in args.only.split(",") if k]
    regions = max(args.regions, 5)
    sets = [k for k in args.sets.split(",") if k]
    results, wresults = [], []
    for sparsity in (0.0, 0.5) if "wgrad" in sets else ():
        rows = []
        for s in synth.mobilenet_dw(args.batch, sparsity):
            if keep and not any(k in s.name for k in keep):
                continue
            print("[depthwise_bench] wgrad %s @ %.1f" % (s.name, sparsity), file=sys.stderr, flush=True)
            rows.append(bench_wgrad(pkg, synth, s, regions, args.reps))
        wresults.append((sparsity, rows))
    for sparsity in (0.0, 0.5) if "forward" in sets else ():
        rows = []
        for s in synth.mobilenet_dw(args.batch, sparsity):
            if keep and not any(k in s.name for k in keep):
                continue
            print("[depthwise_bench] %s @ %.1f" % (s.name, sparsity), file=sys.stderr, flush=True)
            rows.append(bench_layer(pkg, synth, s, regions, args.reps))
        results.append((sparsity, rows))
    dev_name = torch.cuda.get_device_name(0)
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write("\n".join(([markdown(results, dev_name, regions, args.reps)] if results else []) +
                              ([markdown_wgrad(wresults, dev_name, regions, args.reps)] if wresults else [])))
    print(json.dumps(dict(tool="depthwise_bench", device=dev_name, batch=args.batch, regions=regions, reps=args.reps, hbm_peak=HBM_PEAK,
                          results=[dict(sparsity=sp, layers=rows) for sp, rows in results],
                          wgrad=[dict(sparsity=sp, layers=rows) for sp, rows in wresults])))


if __name__ == "__main__":
    main()
