#!/usr/bin/env python3
"""Sparse inner-product layers on the MI355X with and without plan option "b2s", in the same call.

Layers: the fully connected layers of AlexNet and LeNet at Deep Compression's published per-layer densities (Han, Mao,
Dally, "Deep Compression", ICLR 2016, tables 1 and 4): AlexNet fc6 9216 -> 4096 at 9 %, fc7 4096 -> 4096 at 9 %, fc8
4096 -> 1000 at 25 %; LeNet-5 ip1 800 -> 500 at 8 %, ip2 500 -> 10 at 19 %.  The weights are synth.pruned_weights with
dist = "channel": the per-output-channel skew magnitude pruning leaves.  Batches 256 and 32 (--batch: a list).

Per layer and batch, after the outputs of both routes have been compared with a float64 reference (forward, data gradient
and compact weight gradient, each element within gamma(terms + 4) x the sum of its terms' magnitudes):

  forward, data gradient, compact weight gradient   "b2s" = 0 against "b2s" = 1, alternating region by region, each region
                     `--reps` back-to-back calls between device events after a warm-up; the median of `--regions`
                     regions with its spread
  pack, unpack       escoin_plan_b2s_pack of the bottom and escoin_plan_b2s_unpack into the top alone, each beside a
                     device-to-device copy of the bytes it writes; a transpose's GB/s counts its source read once and its
                     destination written once, a copy's its bytes read and written
  blocks             the forward with "b2s_block" forced to 64, 128 and 256
  dense              the forward with the inner plan forced to KERNEL_DENSE: the dense figure of merit
  align_us, code_bytes, kernel   of the "b2s" = 1 plan: whether the layer's generated code fits or the stream / generic
                     kernel takes over is reported, not assumed

The tool fails without a GPU and never falls back.  --only keeps the layers whose name contains one of the given
substrings; --tiny runs the five layers shrunk to a few dozen channels (tests).  Prints one JSON line (progress on stderr);
--markdown FILE also writes the tables of profiles/b2s_mi355x.md.

    python tools/fc_bench.py [--batch 256,32] [--only a,b] [--regions 7] [--reps 3] [--tiny] [--markdown FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402

# name: (K, M, density), and the tiny twin's (K, M)
LAYERS = [("alexnet_fc6", 9216, 4096, 0.09, 72, 48), ("alexnet_fc7", 4096, 4096, 0.09, 48, 48), ("alexnet_fc8", 4096, 1000, 0.25, 48, 20),
          ("lenet_ip1", 800, 500, 0.08, 40, 24), ("lenet_ip2", 500, 10, 0.19, 24, 10)]
BLOCKS = (64, 128, 256)


def layers(synth, n, tiny=False):
    out = []
    for name, k, m, density, tk, tm in LAYERS:
        short = name.split("_")[1]
        out.append(synth.shape("tiny_" + short if tiny else name, n, tk if tiny else k, 1, 1, tm if tiny else m, 1,
                               sparsity=1.0 - density))
    return out


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


def gamma(k):
    u = 2.0 ** -24
    return k * u / (1.0 - k * u)


def reference(s, w, x, b, td):
    """float64 forward, data gradient and weight gradient with the bound of each element."""
    import torch
    W, X, G = (torch.from_numpy(np.ascontiguousarray(a, np.float64)) for a in (w.reshape(s.M, s.C), x.reshape(s.N, s.C), td.reshape(s.N, s.M)))
    tiny = 2.0 ** -149
    row = (W != 0).sum(dim=1).double() + 4
    col = (W != 0).sum(dim=0).double() + 4
    top = X @ W.T + torch.from_numpy(b.astype(np.float64))
    top_b = gamma(row)[None, :] * (X.abs() @ W.abs().T + torch.from_numpy(np.abs(b).astype(np.float64))) + row[None, :] * tiny
    dx = G @ W
    dx_b = gamma(col)[None, :] * (G.abs() @ W.abs()) + col[None, :] * tiny
    dw = G.T @ X
    dw_b = gamma(s.N + 4.0) * (G.abs().T @ X.abs()) + (s.N + 4.0) * tiny
    return [t.numpy() for t in (top, top_b, dx, dx_b, dw, dw_b)]


def worst(got, want, bound):
    got = np.asarray(got, np.float64).reshape(want.shape)
    r = np.where(np.isfinite(got), np.abs(got - want) / bound, np.inf)
    return float(r.max()) if r.size else 0.0


def bench_layer(pkg, synth, s, regions, reps):
    import torch
    dev = torch.device("cuda:0")
    w = synth.pruned_weights(s, 11, dist="channel")
    b = synth.bias_vector(s, 13)
    x_np = synth.activations(s, 12)
    td_np = np.random.RandomState(21).uniform(-1, 1, (s.N, s.M, 1, 1)).astype(np.float32)
    x, td, bias = (torch.from_numpy(a).to(dev) for a in (x_np, td_np, b))
    top, bd = torch.empty_like(td), torch.empty_like(x)
    routes = dict(plain=dict(), b2s=dict(b2s=1), dense=dict(b2s=1, kernel=pkg.KERNEL_DENSE))
    routes.update({"block%d" % blk: dict(b2s=1, b2s_block=blk) for blk in BLOCKS})
    plans = {}
    for name, opts in routes.items():
        plans[name] = pkg.Plan(pkg.ConvDesc.from_shape(s), **opts)
        plans[name].weight_align(w)
    p = plans["b2s"]
    assert p.stat("b2s") == 1 and plans["plain"].stat("b2s") == 0
    vd = torch.zeros(p.nnz(), device=dev)
    # both routes against float64 before anything is timed
    ref = reference(s, w, x_np, b, td_np)
    rp, ci, _, ng = p.get_csr()
    pos = np.concatenate([(np.repeat(np.arange(s.M), np.diff(rp)) * s.C + ci)]) if s.group == 1 else None
    errs = {}
    for name in ("plain", "b2s", "dense"):
        q = plans[name]
        q.forward(x, bias, top)
        q.backward(td, bottom=x, bottom_diff=bd, values_diff=vd.zero_())
        torch.cuda.synchronize()
        errs[name] = dict(forward=worst(top.cpu().numpy(), ref[0], ref[1]), data_gradient=worst(bd.cpu().numpy(), ref[2], ref[3]),
                          compact_wgrad=worst(vd.cpu().numpy(), ref[4].reshape(-1)[pos], ref[5].reshape(-1)[pos]))
        if max(errs[name].values()) > 1.0:
            raise SystemExit("fc_bench: %s route %s is off its float64 bound: %r" % (s.name, name, errs[name]))
    pair = {k: plans[k] for k in ("plain", "b2s")}
    fwd = alternating({k: (lambda q=q: q.forward(x, bias, top)) for k, q in pair.items()}, regions, reps)
    dgr = alternating({k: (lambda q=q: q.backward(td, bottom_diff=bd)) for k, q in pair.items()}, regions, reps)
    wgr = alternating({k: (lambda q=q: q.backward(td, bottom=x, bottom_diff=None, values_diff=vd)) for k, q in pair.items()}, regions, reps)
    sweep = alternating({k: (lambda q=q: q.forward(x, bias, top)) for k, q in plans.items() if k != "plain"}, regions, reps)
    B = p.stat("b2s_block")
    n_inner = -(-s.N // B)
    x_bytes, t_bytes = 4 * n_inner * s.C * B, 4 * n_inner * s.M * B
    assert p.stat("b2s_scratch_bytes") == 2 * x_bytes + t_bytes
    xi, ti = torch.empty(x_bytes // 4, device=dev), torch.zeros(t_bytes // 4, device=dev)
    a, c = torch.empty_like(xi), torch.empty_like(top)
    rr = alternating(dict(pack=lambda: p.b2s_pack(x, xi), pack_copy=lambda: a.copy_(xi), unpack=lambda: p.b2s_unpack(ti, top, top_side=True),
                          unpack_copy=lambda: c.copy_(top)), regions, reps)
    med = {k: float(np.median(v)) for k, v in rr.items()}
    top_bytes = top.numel() * 4
    row = dict(layer=s.name, N=s.N, K=s.C, M=s.M, density=round(1.0 - s.sparsity, 4), nnz=p.nnz(), block=B, inner_images=n_inner,
               flops=2 * s.N * p.nnz(), errors=errs,
               forward={k: dict(summary(v), kernel=pair[k].kernel_name) for k, v in fwd.items()},
               data_gradient={k: dict(summary(v), kernel=pair[k].stat("bwd_data_kernel")) for k, v in dgr.items()},
               compact_wgrad={k: dict(summary(v), kernel=pair[k].stat("wgrad_kernel")) for k, v in wgr.items()},
               blocks={str(blk): dict(summary(sweep["block%d" % blk]), kernel=plans["block%d" % blk].kernel_name,
                                      tiling=plans["block%d" % blk].tiling_info) for blk in BLOCKS},
               dense=dict(summary(sweep["dense"]), kernel=plans["dense"].kernel_name),
               pack=dict(summary(rr["pack"]), src_bytes=x.numel() * 4, dst_bytes=x_bytes, gbps=round((x.numel() * 4 + x_bytes) / med["pack"] * 1e-3, 1)),
               pack_copy=dict(summary(rr["pack_copy"]), gbps=round(2 * x_bytes / med["pack_copy"] * 1e-3, 1)),
               unpack=dict(summary(rr["unpack"]), src_bytes=t_bytes, dst_bytes=top_bytes, gbps=round((t_bytes + top_bytes) / med["unpack"] * 1e-3, 1)),
               unpack_copy=dict(summary(rr["unpack_copy"]), gbps=round(2 * top_bytes / med["unpack_copy"] * 1e-3, 1)),
               align_us=p.stat("align_us"), plain_align_us=plans["plain"].stat("align_us"), code_bytes=p.stat("code_bytes"),
               plain_code_bytes=plans["plain"].stat("code_bytes"), tiling=p.tiling_info, plain_tiling=plans["plain"].tiling_info,
               b2s_workspace_bytes=p.workspace_bytes, plain_workspace_bytes=plans["plain"].workspace_bytes)
    for q in plans.values():
        q.close()
    return row


def markdown(rows, dev_name, regions, reps):
    out = ["Box: %s.  Median of %d regions of %d back-to-back calls per route, routes alternating (min .. max in brackets), us." % (dev_name, regions, reps), ""]
    for what, title in (("forward", "Forward"), ("data_gradient", "Data gradient"), ("compact_wgrad", "Compact weight gradient")):
        out += ["### %s" % title, "", "| layer | batch | b2s = 0 | b2s = 1 | b2s = 0 / b2s = 1 | kernels (0 / 1) |", "|---|---|---|---|---|---|"]
        for r in rows:
            c = r[what]
            cell = lambda k: "%.0f (%.0f .. %.0f)" % (c[k]["median_us"], c[k]["min_us"], c[k]["max_us"])  # noqa: E731
            out.append("| %s | %d | %s | %s | %.2fx | `%s` / `%s` |" % (r["layer"], r["N"], cell("plain"), cell("b2s"),
                                                                      c["plain"]["median_us"] / c["b2s"]["median_us"], c["plain"]["kernel"], c["b2s"]["kernel"]))
        out.append("")
    out += ["### The block sweep and the dense inner kernel (forward, b2s = 1)", "",
            "| layer | batch | B = 64 | B = 128 | B = 256 | inner DENSE | sparse TFLOP/s at the best block | dense TFLOP/s |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        best = min(r["blocks"][str(b)]["median_us"] for b in BLOCKS)
        dense_flops = 2.0 * r["N"] * r["K"] * r["M"]
        out.append("| %s | %d | %s | %.1f | %.1f |" % (r["layer"], r["N"], " | ".join(
            "%.0f (%.0f .. %.0f)" % (r["blocks"][str(b)]["median_us"], r["blocks"][str(b)]["min_us"], r["blocks"][str(b)]["max_us"]) for b in BLOCKS) +
            " | %.0f" % r["dense"]["median_us"], r["flops"] / best * 1e-6, dense_flops / r["dense"]["median_us"] * 1e-6))
    out.append("")
    out += ["### Align time and generated code (b2s = 1 / b2s = 0)", "", "| layer | batch | nnz | align ms | code MB | inner tiling |", "|---|---|---|---|---|---|"]
    for r in rows:
        out.append("| %s | %d | %d | %.1f / %.1f | %.2f / %.2f | `%s` |" % (r["layer"], r["N"], r["nnz"], r["align_us"] / 1e3, r["plain_align_us"] / 1e3,
                                                                         r["code_bytes"] / 1e6, r["plain_code_bytes"] / 1e6, r["tiling"][:90]))
    out.append("")
    for what, title in (("pack", "The pack kernel (bottom -> X') beside a device-to-device copy of X''s bytes"),
                        ("unpack", "The unpack kernel (T' -> top) beside a device-to-device copy of the top's bytes")):
        out += ["### %s" % title, "",
                "| layer | batch | source MB | destination MB | %s us | %s GB/s | copy us | copy GB/s | %s / copy rate |" % (what, what, what),
                "|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            k, c = r[what], r[what + "_copy"]
            out.append("| %s | %d | %.2f | %.2f | %.1f | %.0f | %.1f | %.0f | %.2f |" % (
                r["layer"], r["N"], k["src_bytes"] / 1e6, k["dst_bytes"] / 1e6, k["median_us"], k["gbps"], c["median_us"], c["gbps"],
                k["gbps"] / max(c["gbps"], 1e-9)))
        out.append("")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="256,32")
    ap.add_argument("--only", default="")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--markdown", default="")
    args = ap.parse_args()
    import torch
    pkg = ge.load_package()
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        raise SystemExit("fc_bench needs a HIP device")
    keep = [k for k in args.only.split(",") if k]
    batches = [int(b) for b in args.batch.split(",") if b]
    rows = []
    for n in batches:
        for s in layers(pkg.synth, n, args.tiny):
            if keep and not any(k in s.name for k in keep):
                continue
            print("[fc_bench] %s batch %d" % (s.name, n), file=sys.stderr, flush=True)
            rows.append(bench_layer(pkg, pkg.synth, s, max(args.regions, 5), args.reps))
    dev_name = torch.cuda.get_device_name(0)
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write(markdown(rows, dev_name, max(args.regions, 5), args.reps))
    print(json.dumps(dict(tool="fc_bench", device=dev_name, batches=batches, regions=max(args.regions, 5), reps=args.reps, layers=rows)))


if __name__ == "__main__":
    main()
