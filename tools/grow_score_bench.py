#!/usr/bin/env python3
"""The grow score of a rewire on the MI355X, two routes per layer in the same call:

  A  plan.dense_wgrad on the sparse plan itself (escoin_dense_wgrad_mfma_kernel + escoin_dense_wgrad_sum_kernel);
  B  a shadow plan aligned by set_csr on the FULL pattern with wgrad_kernel = WGRAD_MFMA, backward(weight_diff=...)
     (escoin_sconv_wgrad_mfma_kernel per 1024-pixel chunk + the tree sum) -- the only route before dense_wgrad existed.

The routes alternate region by region (A, B, A, B, ...; with --prev-pkg also B on another checkout's build of the library,
e.g. the parent commit's, as a third member of every round), each region being `--reps` back-to-back calls between device
events after a warm-up; the median of `--regions` (at least 5) regions per route is reported with its spread.  The memory
comparison is exact: the shadow plan's workspace_bytes (a dense plan, its backward state and reduction slab) against stat
"dwg_device_bytes".  The two results are compared element by element (they sum in different orders: a relative difference
of a few ulp x sqrt(pixels) is expected).

Sets: the four ResNet-50 3x3 shapes @90 % (batch 256), AlexNet conv2-5 @80 % (batch 128), the GoogLeNet 1x1 layers @95 %
(batch 256).  --only keeps the layers whose name contains one of the given substrings.  Prints one JSON line (progress on
stderr); --markdown FILE also writes the table of profiles/grow_score_mi355x.md.

    python tools/grow_score_bench.py [--sets resnet,alexnet,googlenet] [--only a,b] [--regions 7] [--reps 3]
                                     [--prev-pkg DIR] [--splits N] [--markdown FILE]
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402


def load_other_package(pkg_dir):
    """Another checkout's caffe-escoin_amd/ (its Python binding and the libescoin_hip.so beside it) as a second module."""
    name = "caffe_escoin_amd_prev"
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def full_csr(s):
    """set_csr's arguments for the full pattern of a layer, values 1."""
    mg, kdim = s.M // s.group, (s.C // s.group) * s.KH * s.KW
    rowptr = np.tile(np.arange(mg + 1, dtype=np.int32) * kdim, s.group)
    colidx = np.tile(np.arange(kdim, dtype=np.int32), s.M)
    return rowptr, colidx, np.ones(s.M * kdim, np.float32), np.full(s.group, mg * kdim, np.int32)


def shadow_plan(pkg, s):
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s), wgrad_kernel=pkg.WGRAD_MFMA)
    plan.set_csr(*full_csr(s))
    return plan


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="resnet,alexnet,googlenet")
    ap.add_argument("--only", default="", help="comma-separated substrings: keep the layers whose name contains one")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--prev-pkg", default="", help="another checkout's caffe-escoin_amd directory (built): route B on its library too")
    ap.add_argument("--splits", type=int, default=0, help="option dense_wgrad_splits of route A's plan (0: the rule)")
    ap.add_argument("--markdown", default="")
    a = ap.parse_args()
    if a.regions < 5:
        ap.error("--regions must be at least 5")
    import torch
    pkg = ge.load_package()
    prev = load_other_package(os.path.abspath(a.prev_pkg)) if a.prev_pkg else None
    synth = pkg.synth
    dev = torch.device("cuda:0")
    layers = []
    sets = a.sets.split(",")
    if "resnet" in sets:
        layers += synth.resnet50_3x3(N=256, sparsity=0.9)
    if "alexnet" in sets:
        layers += synth.alexnet(N=128, sparsity=0.8)
    if "googlenet" in sets:
        layers += synth.googlenet_1x1(N=256, sparsity=0.95)
    if a.only:
        layers = [s for s in layers if any(k in s.name for k in a.only.split(","))]
    rows = []
    for i, s in enumerate(layers):
        w = synth.pruned_weights(s, 1000 + i)
        x = torch.from_numpy(synth.activations(s, 3000 + i)).to(dev)
        oh, ow = synth.out_hw(s)
        td = torch.empty((s.N, s.M, oh, ow), device=dev).uniform_(-1, 1)
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s), dense_wgrad_splits=a.splits)
        plan.weight_align(w)
        shadow = shadow_plan(pkg, s)
        score = torch.zeros((s.M, s.C // s.group, s.KH, s.KW), device=dev)
        wd = torch.zeros_like(score)
        ws_before = plan.workspace_bytes
        plan.dense_wgrad(td, x, out=score)
        shadow.backward(td, bottom=x, bottom_diff=None, weight_diff=wd)      # builds the backward state; wd = the gradient
        torch.cuda.synchronize()
        assert shadow.stat("wgrad_kernel") == pkg.WGRAD_MFMA
        diff = float((score - wd).abs().max() / wd.abs().max().clamp_min(1e-30))
        fns = {"A": lambda: plan.dense_wgrad(td, x, out=score),
               "B": lambda: shadow.backward(td, bottom=x, bottom_diff=None, weight_diff=wd)}
        shadow_prev = None
        if prev is not None:
            shadow_prev = shadow_plan(prev, s)
            wd_prev = torch.zeros_like(score)
            shadow_prev.backward(td, bottom=x, bottom_diff=None, weight_diff=wd_prev)
            fns["B_prev"] = lambda: shadow_prev.backward(td, bottom=x, bottom_diff=None, weight_diff=wd_prev)
        t = alternating(fns, a.regions, a.reps)
        med = {k: v[len(v) // 2] for k, v in t.items()}
        mg, kdim = s.M // s.group, (s.C // s.group) * s.KH * s.KW
        r = dict(layer=s.name, N=s.N, positions=s.M * kdim, tiles=s.group * -(-mg // 64) * -(-kdim // 64),
                 chunks=shadow.stat("bwd_chunks"), splits=plan.stat("dwg_splits"),
                 a_us=med["A"], a_spread_us=[t["A"][0], t["A"][-1]], b_us=med["B"], b_spread_us=[t["B"][0], t["B"][-1]],
                 a_over_b=round(med["A"] / med["B"], 3),
                 a_dense_tflops=round(2.0 * s.N * oh * ow * s.M * kdim / (med["A"] * 1e-6) / 1e12, 2),
                 dwg_device_bytes=plan.stat("dwg_device_bytes"), shadow_workspace_bytes=shadow.workspace_bytes,
                 plan_workspace_growth=plan.workspace_bytes - ws_before, max_rel_diff=diff)
        if shadow_prev is not None:
            r.update(b_prev_us=med["B_prev"], b_prev_spread_us=[t["B_prev"][0], t["B_prev"][-1]],
                     a_over_b_prev=round(med["A"] / med["B_prev"], 3), b_over_b_prev=round(med["B"] / med["B_prev"], 3))
            shadow_prev.close()
        plan.close()
        shadow.close()
        rows.append(r)
        print("%-26s tiles %4d chunks %4d splits %3d  A %8.1f us (%.1f .. %.1f)  B %8.1f us (%.1f .. %.1f)%s  A/B %.3f  state %.2f MB vs shadow %.2f MB  diff %.2g" % (
            s.name, r["tiles"], r["chunks"], r["splits"], r["a_us"], t["A"][0], t["A"][-1], r["b_us"], t["B"][0], t["B"][-1],
            "" if shadow_prev is None else "  B_prev %8.1f us" % r["b_prev_us"], r["a_over_b"], r["dwg_device_bytes"] / 1e6,
            r["shadow_workspace_bytes"] / 1e6, diff), file=sys.stderr, flush=True)
    out = dict(tool="grow_score_bench", device=torch.cuda.get_device_name(0), cus=torch.cuda.get_device_properties(0).multi_processor_count,
               regions=a.regions, reps=a.reps, splits_option=a.splits, layers=rows)
    print(json.dumps(out))
    if a.markdown:
        with open(a.markdown, "w") as f:
            f.write("| layer | tiles | chunks | splits | A us (min .. max) | B us (min .. max) |%s A / B | A TFLOP/s (dense) | A state MB | B shadow plan MB |\n" % (
                " B parent us |" if prev is not None else ""))
            f.write("|---|---|---|---|---|---|%s---|---|---|---|\n" % ("---|" if prev is not None else ""))
            for r in rows:
                f.write("| %s | %d | %d | %d | %.1f (%.1f .. %.1f) | %.1f (%.1f .. %.1f) |%s %.3f | %.2f | %.3f | %.2f |\n" % (
                    r["layer"], r["tiles"], r["chunks"], r["splits"], r["a_us"], r["a_spread_us"][0], r["a_spread_us"][1], r["b_us"],
                    r["b_spread_us"][0], r["b_spread_us"][1], " %.1f |" % r["b_prev_us"] if prev is not None else "", r["a_over_b"],
                    r["a_dense_tflops"], r["dwg_device_bytes"] / 1e6, r["shadow_workspace_bytes"] / 1e6))


if __name__ == "__main__":
    main()
