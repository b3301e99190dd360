#!/usr/bin/env python3
"""Dilated sparse layers on the MI355X with and without plan option "s2b", four routes per layer in the same call:

  s2b      option "s2b" = 1, KERNEL_AUTO: escoin_s2b_pack_kernel + the inner undilated plan of N * P images +
           escoin_s2b_unpack_kernel, forward and data gradient each
  generic  "s2b" = 0, kernel = backward_kernel = GENERIC: the generic forward kernel; the data gradient as the generic
           forward of the (dilated) transposed plan, or the gather kernel where none exists
  dense    "s2b" = 0, kernel = DENSE, backward_kernel = BWD_MFMA: the dense MFMA forward and the MFMA data gradient
  auto     "s2b" = 0, everything automatic: what a dilated layer gets today

The routes alternate region by region (s2b, generic, dense, auto, s2b, ...), each region being `--reps` back-to-back
calls between device events after a warm-up; the median of `--regions` regions per route is reported with its spread
(min .. max), forward and data gradient each.  The forward's two rearrangements alone (escoin_plan_s2b_pack: the bottom
into X'; escoin_plan_s2b_unpack: T' into the top) are timed the same way, each beside a device-to-device copy of as many
bytes as the rearrangement WRITES, in the same process; a rearrangement's GB/s counts its source read once and its
destination written once, a copy's its bytes read and written.

Layers at 90 % sparsity, at batch 8 and at batch 32 (--batch: a comma-separated list): DeepLab-style res4 (256 -> 256, 3x3,
dilation 2, pad 2, 65x65), res5 (512 -> 512, 3x3, dilation 4, pad 4, 65x65), fc6 (512 -> 1024, 3x3, dilation 12, pad 12,
41x41) and an ASPP-like branch (512 -> 256, 3x3, dilation 6, pad 6, 65x65).  --only keeps the layers whose name contains
one of the given substrings; --tiny runs the same four dilations on 8 -> 8 channels and a 9x9 image (tests).  Prints one
JSON line (progress on stderr); --markdown FILE also writes the tables of profiles/s2b_mi355x.md.

    python tools/dilated_bench.py [--batch 8,32] [--only a,b] [--regions 7] [--reps 3] [--tiny] [--markdown FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402


def layers(synth, n, tiny=False):
    sh = synth.shape
    if tiny:
        return [sh("tiny_%s_d%d" % (name, d), n, 8, 9, 9, 8, 3, pad=d, dil=d, bias=False, sparsity=0.5)
                for name, d in (("res4", 2), ("res5", 4), ("fc6", 12), ("aspp", 6))]
    return [
        sh("deeplab_res4_d2", n, 256, 65, 65, 256, 3, pad=2, dil=2, bias=False, sparsity=0.9),
        sh("deeplab_res5_d4", n, 512, 65, 65, 512, 3, pad=4, dil=4, bias=False, sparsity=0.9),
        sh("deeplab_fc6_d12", n, 512, 41, 41, 1024, 3, pad=12, dil=12, bias=False, sparsity=0.9),
        sh("aspp_d6", n, 512, 65, 65, 256, 3, pad=6, dil=6, bias=False, sparsity=0.9),
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
    routes = dict(s2b=dict(s2b=1), generic=dict(kernel=pkg.KERNEL_GENERIC, backward_kernel=pkg.KERNEL_GENERIC),
                  dense=dict(kernel=pkg.KERNEL_DENSE, backward_kernel=pkg.BWD_MFMA), auto=dict())
    plans = {}
    for name, opts in routes.items():
        plans[name] = pkg.Plan(pkg.ConvDesc.from_shape(s), **opts)
        plans[name].weight_align(w)
    fwd = alternating({k: (lambda p=p: p.forward(x, None, top)) for k, p in plans.items()}, regions, reps)
    bwd = alternating({k: (lambda p=p: p.backward(td, bottom_diff=bd)) for k, p in plans.items()}, regions, reps)
    p = plans["s2b"]
    assert p.stat("s2b") == 1
    eh, ew = s.dil_h, s.dil_w
    hi, wi = -(-(s.H + 2 * s.pad_h) // eh), -(-(s.W + 2 * s.pad_w) // ew)
    x_bytes = 4 * s.N * eh * ew * s.C * hi * wi
    t_bytes = 4 * s.N * eh * ew * s.M * (hi - s.KH + 1) * (wi - s.KW + 1)
    assert p.stat("s2b_scratch_bytes") == x_bytes + t_bytes
    a, b = torch.empty(x_bytes // 4, device=dev), torch.empty(x_bytes // 4, device=dev)
    c, d = torch.empty_like(top), torch.empty_like(top)
    rr = alternating(dict(pack=lambda: p.s2b_pack(x), pack_copy=lambda: b.copy_(a), unpack=lambda: p.s2b_unpack(top),
                          unpack_copy=lambda: d.copy_(c)), regions, reps)
    med = {k: float(np.median(v)) for k, v in rr.items()}
    top_bytes = top.numel() * 4
    row = dict(layer=s.name, N=s.N, sparsity=s.sparsity, nnz=p.nnz(), inner_images=s.N * eh * ew, inner_hw=[hi, wi],
               forward={k: dict(summary(v), kernel=plans[k].kernel_name) for k, v in fwd.items()},
               backward={k: dict(summary(v), kernel=plans[k].stat("bwd_data_kernel")) for k, v in bwd.items()},
               pack=dict(summary(rr["pack"]), src_bytes=x.numel() * 4, dst_bytes=x_bytes,
                         gbps=round((x.numel() * 4 + x_bytes) / med["pack"] * 1e-3, 1)),
               pack_copy=dict(summary(rr["pack_copy"]), gbps=round(2 * x_bytes / med["pack_copy"] * 1e-3, 1)),
               unpack=dict(summary(rr["unpack"]), src_bytes=t_bytes, dst_bytes=top_bytes,
                           gbps=round((t_bytes + top_bytes) / med["unpack"] * 1e-3, 1)),
               unpack_copy=dict(summary(rr["unpack_copy"]), gbps=round(2 * top_bytes / med["unpack_copy"] * 1e-3, 1)),
               s2b_workspace_bytes=p.workspace_bytes, auto_workspace_bytes=plans["auto"].workspace_bytes)
    for q in plans.values():
        q.close()
    return row


def markdown(rows, dev_name, regions, reps):
    out = ["Box: %s.  Median of %d regions of %d back-to-back calls per route, routes alternating (min .. max in brackets), us." % (dev_name, regions, reps), ""]
    for what in ("forward", "backward"):
        out += ["### %s" % ("Forward" if what == "forward" else "Data gradient"), "",
                "| layer | batch | s2b | generic | dense | auto (s2b = 0) | s2b vs auto |", "|---|---|---|---|---|---|---|"]
        for r in rows:
            c = r[what]
            cell = lambda k: "%.0f (%.0f .. %.0f)" % (c[k]["median_us"], c[k]["min_us"], c[k]["max_us"])  # noqa: E731
            out.append("| %s | %d | %s | %s | %s | %s | %.2fx |" % (r["layer"], r["N"], cell("s2b"), cell("generic"), cell("dense"), cell("auto"),
                                                                   c["auto"]["median_us"] / c["s2b"]["median_us"]))
        out.append("")
    out += ["### Kernels per route", "", "| layer | batch | s2b forward | auto forward | s2b / auto bwd_data_kernel |", "|---|---|---|---|---|"]
    for r in rows:
        out.append("| %s | %d | `%s` | `%s` | %s / %s |" % (r["layer"], r["N"], r["forward"]["s2b"]["kernel"], r["forward"]["auto"]["kernel"],
                                                          r["backward"]["s2b"]["kernel"], r["backward"]["auto"]["kernel"]))
    out.append("")
    for what, title in (("pack", "The pack kernel (bottom -> X') beside a device-to-device copy of X''s bytes"),
                        ("unpack", "The unpack kernel (T' -> top) beside a device-to-device copy of the top's bytes")):
        out += ["### %s" % title, "",
                "| layer | batch | source MB | destination MB | %s us | %s GB/s | copy us | copy GB/s | %s / copy rate |" % (what, what, what),
                "|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            k, c = r[what], r[what + "_copy"]
            out.append("| %s | %d | %.1f | %.1f | %.0f | %.0f | %.0f | %.0f | %.2f |" % (
                r["layer"], r["N"], k["src_bytes"] / 1e6, k["dst_bytes"] / 1e6, k["median_us"], k["gbps"], c["median_us"], c["gbps"],
                k["gbps"] / c["gbps"]))
        out.append("")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="8,32")
    ap.add_argument("--only", default="")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--markdown", default="")
    args = ap.parse_args()
    import torch
    pkg = ge.load_package()
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        raise SystemExit("dilated_bench needs a HIP device")
    keep = [k for k in args.only.split(",") if k]
    batches = [int(b) for b in args.batch.split(",") if b]
    rows = []
    for n in batches:
        for s in layers(pkg.synth, n, args.tiny):
            if keep and not any(k in s.name for k in keep):
                continue
            print("[dilated_bench] %s batch %d" % (s.name, n), file=sys.stderr, flush=True)
            rows.append(bench_layer(pkg, pkg.synth, s, max(args.regions, 5), args.reps))
    dev_name = torch.cuda.get_device_name(0)
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write(markdown(rows, dev_name, max(args.regions, 5), args.reps))
    print(json.dumps(dict(tool="dilated_bench", device=dev_name, batches=batches, regions=max(args.regions, 5), reps=args.reps, layers=rows)))


if __name__ == "__main__":
    main()
