#!/usr/bin/env python3
"""Backward on the MI355X: per layer, forward / data-gradient / weight-gradient / bias-gradient time of the
pattern-preserving backward (escoin_backward), the kernels that ran, and the same shapes through torch's dense conv
backward (MIOpen, dense weights) as a comparison point.  The weight gradient is timed three ways in the same call, on
separate plans: option wgrad_kernel = ENTRY, = STAGED (skipped where the staged kernel does not serve the plan), = MFMA
and the default AUTO; the compact entry point (escoin_backward_values) on the AUTO plan.  Where AUTO ran the gather kernel
for the data gradient (stride > 1, pad > dil x (K - 1)), the data gradient is timed a second time on a plan forced to
backward_kernel = BWD_MFMA (escoin_sconv_dgrad_mfma_kernel), with the regions of both, so that "the MFMA kernel's slowest
region is shorter than the gather kernel's fastest" can be read off one call ("dgrad_mfma_faster").

Sets: the four ResNet-50 3x3 shapes @90 % (batch 256), the GoogLeNet 1x1 layers @95 % (batch 256), AlexNet conv2-5
@80 % (batch 128); "chain": the layers the forward keeps dense -- the distinct 1x1 shapes and the four 3x3 shapes of the
ResNet-50 chain at batch 256 and density 1.0, conv1 of AlexNet (11x11 stride 4) and of ResNet-50 (7x7 stride 2); "sweep":
res2_branch2b, res5_branch2b and the chain's res4_branch2c at densities 1.0 / 0.5 / 0.3 / 0.2 / 0.1; "strided": the 3x3
stride-2 pad-1 shapes 128 @ 56, 256 @ 28 and 512 @ 14 (ResNet-50 v1.5) @90 % (batch 256).  --only keeps the layers whose
name contains one of the given substrings.  Times are device
events around `--reps` back-to-back calls after a warm-up, the median of `--regions` regions, per call.  Prints one JSON line (and progress on stderr).

    python tools/backward_bench.py [--sets resnet,googlenet,alexnet,chain,sweep,strided] [--only a,b] [--regions 7] [--reps 5] [--no-torch]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402

FAMILY = {0: "auto", 1: "gather (escoin_sconv_bwd_data_kernel)", 2: "tiled (transposed plan)",
          3: "dense MFMA (transposed plan)", 4: "generated code (transposed plan)", 5: "MFMA (escoin_sconv_dgrad_mfma_kernel)"}


WGRAD = {1: "entry", 2: "staged", 3: "mfma"}
SWEEP = (1.0, 0.5, 0.3, 0.2, 0.1)


def chain_layers(synth, N=256):
    """The layers of the ResNet-50 chain (tools/caffe_test.py --model resnet50_chain) at density 1.0, one per distinct
    shape, then the two conv1 layers."""
    out, seen = [], set()
    cin, hw = 64, 56
    for si, (mid, cout, blocks, stride) in enumerate([(64, 256, 3, 1), (128, 512, 4, 2), (256, 1024, 6, 2), (512, 2048, 3, 2)]):
        for b in range(blocks):
            st = stride if b == 0 else 1
            tag = "res%d%s" % (si + 2, "abcdef"[b])
            ohw = hw // st
            cand = [(tag + "_branch2a", cin, hw, mid, 1, dict(stride=st)), (tag + "_branch2b", mid, ohw, mid, 3, dict(pad=1)),
                    (tag + "_branch2c", mid, ohw, cout, 1, {})]
            if b == 0:
                cand.insert(0, (tag + "_branch1", cin, hw, cout, 1, dict(stride=st)))
            for name, c, h, m, k, kw in cand:
                key = (c, h, m, k, tuple(sorted(kw.items())))
                if key not in seen:
                    seen.add(key)
                    out.append(synth.shape(name, N, c, h, h, m, k, bias=False, sparsity=0.0, **kw))
            cin, hw = cout, ohw
    out.append(synth.shape("alex_conv1", 128, 3, 227, 227, 96, 11, stride=4, sparsity=0.0))
    out.append(synth.shape("resnet_conv1", N, 3, 224, 224, 64, 7, pad=3, stride=2, sparsity=0.0))
    return out


def sweep_layers(synth, N=256):
    base = [("res2_branch2b", 64, 56, 64, 3, dict(pad=1)), ("res5_branch2b", 512, 7, 512, 3, dict(pad=1)),
            ("res4_branch2c", 256, 14, 1024, 1, {})]
    return [synth.shape("%s@%.1f" % (name, d), N, c, h, h, m, k, bias=False, sparsity=1.0 - d, **kw)
            for name, c, h, m, k, kw in base for d in SWEEP]


def strided_layers(synth, N=256):
    return [synth.shape("s2_3x3_%d@%d" % (c, hw), N, c, hw, hw, c, 3, pad=1, stride=2, bias=False, sparsity=0.9)
            for c, hw in ((128, 56), (256, 28), (512, 14))]


def timed(fn, regions, reps):
    out = timed_regions(fn, regions, reps)
    return out[len(out) // 2]


def timed_regions(fn, regions, reps):
    """Sorted per-call times (us) of `regions` regions of `reps` back-to-back calls."""
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(regions):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / reps)
    out.sort()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="resnet,googlenet,alexnet")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--only", default="", help="comma-separated substrings: keep the layers whose name contains one")
    a = ap.parse_args()
    import torch
    pkg = ge.load_package()
    synth = pkg.synth
    dev = torch.device("cuda:0")
    layers = []
    sets = a.sets.split(",")
    if "resnet" in sets:
        layers += synth.resnet50_3x3(N=256, sparsity=0.9)
    if "googlenet" in sets:
        layers += synth.googlenet_1x1(N=256, sparsity=0.95)
    if "alexnet" in sets:
        layers += synth.alexnet(N=128, sparsity=0.8)
    if "chain" in sets:
        layers += chain_layers(synth)
    if "sweep" in sets:
        layers += sweep_layers(synth)
    if "strided" in sets:
        layers += strided_layers(synth)
    if a.only:
        layers = [s for s in layers if any(k in s.name for k in a.only.split(","))]
    rows = []
    for i, s in enumerate(layers):
        w = synth.pruned_weights(s, 1000 + i)
        b = synth.bias_vector(s, 2000 + i)
        x = torch.from_numpy(synth.activations(s, 3000 + i)).to(dev)
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
        plan.weight_align(w)
        bt = torch.from_numpy(b).to(dev) if b is not None else None
        top = plan.forward(x, bt)
        td = torch.empty_like(top).uniform_(-1, 1)
        bd = torch.empty_like(x)
        wd = torch.zeros((s.M, s.C // s.group, s.KH, s.KW), device=dev)
        bsd = torch.zeros((s.M,), device=dev)
        plan.backward(td, bottom=x, bottom_diff=bd, weight_diff=wd, bias_diff=bsd)   # builds the backward state
        r = dict(layer=s.name, N=s.N, density=round(float((w != 0).mean()), 4), fwd_kernel=plan.kernel_name,
                 bwd_data_kernel=FAMILY[plan.stat("bwd_data_kernel")], bwd_chunks=plan.stat("bwd_chunks"),
                 bwd_align_ms=plan.stat("bwd_align_us") * 1e-3, bwd_device_mb=plan.stat("bwd_device_bytes") / 1e6)
        r["fwd_us"] = timed(lambda: plan.forward(x, bt, top), a.regions, a.reps)
        regions = timed_regions(lambda: plan.backward(td, bottom_diff=bd), a.regions, a.reps)
        r["bwd_data_us"] = regions[len(regions) // 2]
        r["bwd_data_spread_us"] = [regions[0], regions[-1]]
        if plan.stat("bwd_data_kernel") == pkg.KERNEL_GENERIC:
            # the gather kernel ran: the same data gradient on the fp32 matrix cores, in the same call
            forced = pkg.Plan(pkg.ConvDesc.from_shape(s), backward_kernel=pkg.BWD_MFMA)
            forced.weight_align(w)
            forced.backward(td, bottom_diff=bd)
            assert forced.stat("bwd_data_kernel") == pkg.BWD_MFMA
            mregions = timed_regions(lambda: forced.backward(td, bottom_diff=bd), a.regions, a.reps)
            r["bwd_data_mfma_us"] = mregions[len(mregions) // 2]
            r["bwd_data_mfma_spread_us"] = [mregions[0], mregions[-1]]
            r["dgrad_mfma_faster"] = bool(mregions[-1] < regions[0])       # its slowest region against the gather's fastest
            r["dgrad_lds_bytes"] = forced.stat("dgrad_lds_bytes")
            r["dgrad_mfma_over_fwd"] = round(r["bwd_data_mfma_us"] / r["fwd_us"], 3)
            # the kernel multiplies every live 64 x 32 weight block whatever its density: its rate on the dense problem
            r["dgrad_dense_tflops"] = round(2.0 * s.N * plan.out_hw[0] * plan.out_hw[1] * s.M * (s.C // s.group) * s.KH * s.KW /
                                            (r["bwd_data_mfma_us"] * 1e-6) / 1e12, 2)
            forced.close()
        r["bwd_weight_us"] = timed(lambda: plan.backward(td, bottom=x, bottom_diff=None, weight_diff=wd), a.regions, a.reps)
        r["bwd_bias_us"] = timed(lambda: plan.backward(td, bottom_diff=None, bias_diff=bsd), a.regions, a.reps)
        r["wgrad_kernel"] = WGRAD[plan.stat("wgrad_kernel")]
        r["wgrad_lds_bytes"] = plan.stat("wgrad_lds_bytes")
        vd = torch.zeros((plan.nnz(),), device=dev)
        r["bwd_values_us"] = timed(lambda: plan.backward(td, bottom=x, bottom_diff=None, values_diff=vd), a.regions, a.reps)
        for kid in (pkg.WGRAD_ENTRY, pkg.WGRAD_STAGED, pkg.WGRAD_MFMA):
            forced = pkg.Plan(pkg.ConvDesc.from_shape(s), wgrad_kernel=kid)
            forced.weight_align(w)
            key = "bwd_weight_%s" % WGRAD[kid]
            try:
                forced.backward(td, bottom=x, bottom_diff=None, weight_diff=wd)
            except pkg.EscoinError:
                r[key + "_us"] = None          # the forced kernel does not serve this plan
                forced.close()
                continue
            regions = timed_regions(lambda: forced.backward(td, bottom=x, bottom_diff=None, weight_diff=wd), a.regions, a.reps)
            r[key + "_us"] = regions[len(regions) // 2]
            r[key + "_spread_us"] = [regions[0], regions[-1]]
            r["bwd_bias_%s_us" % WGRAD[kid]] = timed(lambda: forced.backward(td, bottom_diff=None, bias_diff=bsd), a.regions, a.reps)
            forced.close()
        r["mfma_over_fwd"] = round(r["bwd_weight_mfma_us"] / r["fwd_us"], 3)
        # the MFMA kernel multiplies the whole M x Kd tile grid whatever the density: its rate on the dense problem
        r["mfma_dense_tflops"] = round(2.0 * s.N * plan.out_hw[0] * plan.out_hw[1] * s.M * (s.C // s.group) * s.KH * s.KW /
                                       (r["bwd_weight_mfma_us"] * 1e-6) / 1e12, 2)
        r["data_over_fwd"] = round(r["bwd_data_us"] / r["fwd_us"], 3)
        r["weight_over_fwd"] = round(r["bwd_weight_us"] / r["fwd_us"], 3)
        if not a.no_torch:
            wdense = torch.from_numpy(w).to(dev)
            args = ([s.stride_h, s.stride_w], [s.pad_h, s.pad_w], [s.dil_h, s.dil_w], False, [0, 0], s.group)
            conv_bwd = torch.ops.aten.convolution_backward
            r["torch_data_us"] = timed(lambda: conv_bwd(td, x, wdense, None, *args, [True, False, False]), a.regions, a.reps)
            r["torch_weight_us"] = timed(lambda: conv_bwd(td, x, wdense, None, *args, [False, True, False]), a.regions, a.reps)
        plan.close()
        rows.append(r)
        print("%-28s fwd %8.1f  data %8.1f  weight %8.1f (%s; entry %s staged %s mfma %.1f; compact %.1f)  bias %7.1f us  [%s]%s" % (
            s.name, r["fwd_us"], r["bwd_data_us"], r["bwd_weight_us"], r["wgrad_kernel"],
            "%.1f" % r["bwd_weight_entry_us"], "-" if r["bwd_weight_staged_us"] is None else "%.1f" % r["bwd_weight_staged_us"], r["bwd_weight_mfma_us"],
            r["bwd_values_us"], r["bwd_bias_us"], r["bwd_data_kernel"],
            "" if a.no_torch else "  torch data %8.1f weight %8.1f" % (r["torch_data_us"], r["torch_weight_us"])),
            file=sys.stderr, flush=True)
        if "bwd_data_mfma_us" in r:
            print("%-28s data gradient: gather %.1f .. %.1f us, MFMA %.1f .. %.1f us (%.2f x fwd, %.1f TFLOP/s dense)  %s" % (
                s.name, r["bwd_data_spread_us"][0], r["bwd_data_spread_us"][1], r["bwd_data_mfma_spread_us"][0],
                r["bwd_data_mfma_spread_us"][1], r["dgrad_mfma_over_fwd"], r["dgrad_dense_tflops"],
                "MFMA faster" if r["dgrad_mfma_faster"] else "MFMA NOT faster"), file=sys.stderr, flush=True)
    print(json.dumps(dict(tool="backward_bench", device=torch.cuda.get_device_name(0), layers=rows)))


if __name__ == "__main__":
    main()
