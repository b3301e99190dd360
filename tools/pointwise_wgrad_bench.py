#!/usr/bin/env python3
"""The weight gradient of pointwise layers on the MI355X with and without plan option "wgrad_pointwise", in the same call.

Routes, alternating region by region within one process:
  off      the option at 0: "wgrad_kernel" AUTO picks the entry or the staged kernel -- the baseline, code the option does
           not touch
  on       the option at 1: escoin_sconv_wgrad_pointwise_kernel (stat "wgrad_kernel" == 4 is asserted)
  entry    "wgrad_kernel" forced to ENTRY
  staged   "wgrad_kernel" forced to STAGED, where it serves the layer (stride 1)

Sets (--sets): "googlenet" the 39 GoogLeNet 1x1 layers @95 %, "resnet" the eight distinct ResNet-50 bottleneck 1x1 layers
@90 % (batch 256), "fc" AlexNet fc6 / fc7 / fc8 and LeNet ip1 / ip2 at Deep Compression's densities through "b2s" at batch
256 and 32, "deconv" unet_256_128_k2s2 through "deconv" at batch 64 and density 0.3.

Columns, per layer and route: the compact weight gradient (escoin_backward_values, no data gradient, no bias), the bias
gradient alone, and once per layer the same plan's forward; each the median of `--regions` regions of `--reps` back-to-back
calls between device events after a warm-up, with its spread.  "GB/s" is the bytes of G and of the bottom the weight
gradient has to read once, over the route's time.  Before anything is timed the "on" route's gradient is compared with the
"off" route's (relative error of the largest element).

The tool fails without a GPU and never falls back.  --only keeps the layers whose name contains one of the given
substrings.  Prints one JSON line (progress on stderr); --markdown FILE also writes the tables of
profiles/wgrad_pointwise_mi355x.md.

    python tools/pointwise_wgrad_bench.py [--sets googlenet,resnet,fc,deconv] [--only a,b] [--regions 7] [--reps 5] [--markdown FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402

# ResNet-50's bottleneck 1x1 layers, one per distinct shape: (name, C, H = W, M)
RESNET_1X1 = [("res2_reduce", 256, 56, 64), ("res2_expand", 64, 56, 256), ("res3_reduce", 512, 28, 128), ("res3_expand", 128, 28, 512),
              ("res4_reduce", 1024, 14, 256), ("res4_expand", 256, 14, 1024), ("res5_reduce", 2048, 7, 512), ("res5_expand", 512, 7, 2048)]
# (name, K, M, density): Han, Mao, Dally, "Deep Compression", ICLR 2016, tables 1 and 4
FC = [("alexnet_fc6", 9216, 4096, 0.09), ("alexnet_fc7", 4096, 4096, 0.09), ("alexnet_fc8", 4096, 1000, 0.25),
      ("lenet_ip1", 800, 500, 0.08), ("lenet_ip2", 500, 10, 0.19)]
UNET = ("unet_256_128_k2s2", 64, 256, 128, 28, 2, 0.3)       # name, N, C, M, H = W, K = stride, density


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


def cases(pkg, synth, sets):
    """(name, descriptor, plan options, weights, bottom shape, top_diff shape, bytes of G and the bottom)"""
    out = []
    convs = []
    if "googlenet" in sets:
        convs += synth.googlenet_1x1(N=256, sparsity=0.95)
    if "resnet" in sets:
        convs += [synth.shape(n, 256, c, hw, hw, m, 1, sparsity=0.9) for n, c, hw, m in RESNET_1X1]
    for s in convs:
        oh, ow = synth.out_hw(s)
        out.append((s.name, pkg.ConvDesc.from_shape(s), {}, synth.pruned_weights(s, 11), (s.N, s.C, s.H, s.W), (s.N, s.M, oh, ow)))
    if "fc" in sets:
        for batch in (256, 32):
            for name, k, m, density in FC:
                s = synth.shape("%s_b%d" % (name, batch), batch, k, 1, 1, m, 1, sparsity=1.0 - density)
                out.append((s.name, pkg.ConvDesc.from_shape(s), dict(b2s=1), synth.pruned_weights(s, 11, dist="channel"), (batch, k, 1, 1),
                            (batch, m, 1, 1)))
    if "deconv" in sets:
        name, n, c, m, hw, k, density = UNET
        rs = np.random.RandomState(5)
        w = rs.uniform(-1, 1, (c, m, k, k)).astype(np.float32)
        w[w == 0] = 0.5
        w *= rs.uniform(0, 1, w.shape) < density
        out.append((name, pkg.ConvDesc.deconvolution(n, c, hw, hw, m, k, k, 0), dict(deconv=1), w, (n, c, hw, hw), (n, m, k * hw, k * hw)))
    return out


def bench_case(pkg, case, regions, reps):
    import torch
    dev = torch.device("cuda:0")
    name, desc, opts, w, xshape, tshape = case
    x = torch.from_numpy(np.random.RandomState(12).uniform(-1, 1, xshape).astype(np.float32)).to(dev)
    td = torch.from_numpy(np.random.RandomState(21).uniform(-1, 1, tshape).astype(np.float32)).to(dev)
    routes = dict(off=dict(), on=dict(wgrad_pointwise=1), entry=dict(wgrad_kernel=pkg.WGRAD_ENTRY), staged=dict(wgrad_kernel=pkg.WGRAD_STAGED))
    plans, ran, vds = {}, {}, {}
    for r, o in routes.items():
        plan = pkg.Plan(desc, **dict(opts, **o))
        plan.weight_align(w)
        vd = torch.zeros(plan.nnz(), device=dev)
        try:
            plan.backward(td, bottom=x, bottom_diff=None, values_diff=vd)
        except pkg.EscoinError:
            if r != "staged":
                raise
            plan.close()          # the staged kernel does not serve the layer (a stride above 1)
            continue
        torch.cuda.synchronize()
        plans[r], ran[r], vds[r] = plan, plan.stat("wgrad_kernel"), vd
    assert ran["on"] == pkg.WGRAD_POINTWISE, (name, ran)
    want = vds["off"].cpu().numpy().astype(np.float64)
    err = float(np.abs(vds["on"].cpu().numpy() - want).max() / max(np.abs(want).max(), 1e-30))
    assert err <= 1e-4, (name, err)
    bsd = torch.zeros(tshape[1], device=dev)
    wg = alternating({r: (lambda p=p, v=vds[r]: p.backward(td, bottom=x, bottom_diff=None, values_diff=v)) for r, p in plans.items()},
                     regions, reps)
    bias = alternating({r: (lambda p=p: p.backward(td, bottom_diff=None, bias_diff=bsd)) for r, p in plans.items() if r in ("off", "on")},
                       regions, reps)
    top = torch.empty(tshape, device=dev)
    fwd = alternating(dict(forward=lambda: plans["on"].forward(x, None, top)), regions, reps)
    nbytes = 4 * (int(np.prod(xshape)) + int(np.prod(tshape)))
    row = dict(layer=name, nnz=plans["on"].nnz(), chunks=plans["on"].stat("bwd_chunks"), lds_bytes=plans["on"].stat("wgrad_lds_bytes"),
               kernel={r: int(k) for r, k in ran.items()}, rel_err_on_vs_off=err, operand_bytes=nbytes,
               wgrad={r: summary(t) for r, t in wg.items()}, bias={r: summary(t) for r, t in bias.items()},
               forward=summary(fwd["forward"]))
    row["gbps"] = {r: round(nbytes / (row["wgrad"][r]["median_us"] * 1e3), 1) for r in wg}
    for p in plans.values():
        p.close()
    return row


def markdown(rows):
    out = ["| layer | nnz | AUTO ran | off us | on us | entry us | staged us | on / off | on GB/s | bias off us | bias on us | forward us |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    names = {1: "entry", 2: "staged", 3: "mfma", 4: "pointwise"}

    def cell(d, r):
        return "%.0f (%.0f .. %.0f)" % (d[r]["median_us"], d[r]["min_us"], d[r]["max_us"]) if r in d else "-"
    for r in rows:
        w = r["wgrad"]
        out.append("| %s | %d | %s | %s | %s | %s | %s | %.2fx | %.0f | %s | %s | %.0f |" % (
            r["layer"], r["nnz"], names[r["kernel"]["off"]], cell(w, "off"), cell(w, "on"), cell(w, "entry"), cell(w, "staged"),
            w["off"]["median_us"] / w["on"]["median_us"], r["gbps"]["on"], cell(r["bias"], "off"), cell(r["bias"], "on"),
            r["forward"]["median_us"]))
    tot = {k: sum(r["wgrad"][k]["median_us"] for r in rows) for k in ("off", "on")}
    out.append("")
    out.append("sum of medians: off %.0f us, on %.0f us (%.2fx)" % (tot["off"], tot["on"], tot["off"] / tot["on"]))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="googlenet,resnet,fc,deconv")
    ap.add_argument("--only", default="")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--markdown", default="")
    args = ap.parse_args()
    pkg = ge.load_package()
    import torch
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        raise SystemExit("pointwise_wgrad_bench: no HIP device visible")
    from importlib import import_module
    synth = import_module(pkg.__name__ + ".synth")
    only = [t for t in args.only.split(",") if t]
    rows = []
    for case in cases(pkg, synth, set(args.sets.split(","))):
        if only and not any(t in case[0] for t in only):
            continue
        row = bench_case(pkg, case, args.regions, args.reps)
        print("%-28s off %7.1f on %7.1f us" % (row["layer"], row["wgrad"]["off"]["median_us"], row["wgrad"]["on"]["median_us"]),
              file=sys.stderr, flush=True)
        rows.append(row)
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write(markdown(rows))
    print(json.dumps(dict(tool="pointwise_wgrad_bench", regions=args.regions, reps=args.reps, rows=rows)))


if __name__ == "__main__":
    main()
