#!/usr/bin/env python3
"""In-place weight updates on the MI355X: per layer and per set,
  (a) escoin_update_values from a device blob on a plan in its training state (forward and backward state built: the
      update reaches the backward state's copies too),
  (b) what the same effect costs without it: escoin_weight_align with w_on_device = 1 plus the rebuild the first
      escoin_backward then does (stats align_us + bwd_align_us; median of --realigns rounds),
  (c) the layer's forward, in the same call.

Sets: the four ResNet-50 3x3 shapes @90 % (batch 256, x their count in the net), AlexNet conv2-5 @80 % (batch 128), the
GoogLeNet 1x1 layers @95 % (batch 256).  (a) and (c) are device events around `--reps` back-to-back calls after a warm-up,
the median of `--regions` regions, per call.  Prints one JSON line (progress on stderr); --md writes the table.

    python tools/update_bench.py [--sets resnet,alexnet,googlenet] [--regions 7] [--reps 5] [--realigns 3] [--md out.md]

--solver sgd|nesterov|adam measures the solver step instead, on the same plans in the same training state:
  (a) escoin_solver_step on the compact gradient (the rule and the scatter in one launch),
  (b) what the same effect costs without it: the rule as in-place torch element-wise ops on compact tensors (L2 decay,
      history, update of a compact copy of the values), then escoin_plan_set_values from the device,
  (c) the layer's forward.

    python tools/update_bench.py --solver adam [--sets ...] [--regions 7] [--reps 5] [--md out.md]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402


def timed(fn, regions, reps):
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
    return out[len(out) // 2]


HYPER = dict(rate=1e-3, momentum=0.9, momentum2=0.999, delta=1e-8, decay=5e-4)


def torch_rule(rule, vals, g, h, h2, tmp):
    """The rule of include/escoin.h "Solver step" (L2 decay) as in-place torch ops on compact tensors, as few as it takes."""
    import torch
    rate, mom, mom2, delta, decay = (HYPER[k] for k in ("rate", "momentum", "momentum2", "delta", "decay"))
    torch.add(g, vals, alpha=decay, out=tmp)                       # Regularize
    if rule == "adam":
        h.mul_(mom).add_(tmp, alpha=1 - mom)
        h2.mul_(mom2).addcmul_(tmp, tmp, value=1 - mom2)
        torch.sqrt(h2, out=tmp)
        vals.addcdiv_(h, tmp.add_(delta), value=-rate)
    elif rule == "nesterov":
        vals.add_(h, alpha=mom)                                    # w -= (1 + mom) * h' - mom * h
        h.mul_(mom).add_(tmp, alpha=rate)
        vals.add_(h, alpha=-(1 + mom))
    else:
        h.mul_(mom).add_(tmp, alpha=rate)
        vals.sub_(h)


def solver_main(a):
    import torch
    pkg = ge.load_package()
    synth = pkg.synth
    dev = torch.device("cuda:0")
    rows, totals = [], []
    k = 0
    for set_name, layers in make_sets(synth, a.sets):
        tot = dict(set=set_name, layers=0, fused_us=0.0, torch_us=0.0, fwd_us=0.0)
        for s in layers:
            k += 1
            w = synth.pruned_weights(s, 1000 + k)
            b = synth.bias_vector(s, 2000 + k)
            x = torch.from_numpy(synth.activations(s, 3000 + k)).to(dev)
            W = torch.from_numpy(w).to(dev)
            bt = torch.from_numpy(b).to(dev) if b is not None else None
            plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
            plan.weight_align(W)
            top = plan.forward(x, bt)
            td = torch.empty_like(top).uniform_(-1, 1)
            bd = torch.empty_like(x)
            plan.backward(td, bottom_diff=bd)       # the training state: the step reaches the backward state's copies too
            n = plan.nnz()
            vals = torch.from_numpy(plan.get_csr()[2].copy()).to(dev)
            g = torch.empty(n, device=dev).uniform_(-1e-3, 1e-3)
            h, h2, tmp = torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.empty(n, device=dev)
            desc = pkg.SolverDesc.make(type=a.solver, regularization="L2", **HYPER)   # built once: the timed call is the C call
            plan.solver_step(g, h, h2, desc=desc)   # builds the update state and its entry-major view
            torch.cuda.synchronize()
            assert plan.stat("update_fast") == 1, s.name
            r = dict(set=set_name, layer=s.name, count=s.count, N=s.N, nnz=n, kernel=plan.kernel_name,
                     destinations=plan.stat("update_destinations"), upd_device_mb=round(plan.stat("upd_device_bytes") / 1e6, 3))
            r["fused_us"] = timed(lambda: plan.solver_step(g, h, h2, desc=desc), a.regions, a.reps)
            # (b) starts where (a) left the layer: the plan's values, copies of the histories
            vals.copy_(torch.from_numpy(plan.get_csr()[2]))
            hb, h2b = h.clone(), h2.clone()

            def unfused():
                torch_rule(a.solver, vals, g, hb, h2b, tmp)
                plan.set_values(vals)

            r["torch_us"] = timed(unfused, a.regions, a.reps)
            r["fwd_us"] = timed(lambda: plan.forward(x, bt, top), a.regions, a.reps)
            r["fused_over_torch"] = r["fused_us"] / r["torch_us"]
            r["fused_over_fwd"] = r["fused_us"] / r["fwd_us"]
            rows.append(r)
            for key in ("fused_us", "torch_us", "fwd_us"):
                tot[key] += r[key] * s.count
            tot["layers"] += s.count
            print("%-22s %-34s nnz %8d dst %9d  fused %7.1f us  torch + set_values %7.1f us  fwd %7.1f us" %
                  (s.name, r["kernel"], n, r["destinations"], r["fused_us"], r["torch_us"], r["fwd_us"]), file=sys.stderr)
            plan.close()
            del x, W, top, td, bd, vals, g, h, h2, hb, h2b, tmp
            torch.cuda.empty_cache()
        tot["fused_over_torch"] = tot["fused_us"] / tot["torch_us"]
        tot["fused_over_fwd"] = tot["fused_us"] / tot["fwd_us"]
        totals.append(tot)
    result = dict(tool="update_bench", solver=a.solver, regions=a.regions, reps=a.reps, totals=totals, layers=rows)
    line = json.dumps(result)
    print(line)
    if a.md:
        with open(a.md, "w") as f:
            f.write("| set | layers | (a) solver_step (%s), us | (b) torch rule + set_values, us | (c) forward, us | (a)/(b) | (a)/(c) |\n" % a.solver)
            f.write("|---|---:|---:|---:|---:|---:|---:|\n")
            for t in totals:
                f.write("| %s | %d | %.1f | %.1f | %.1f | %.3f | %.3f |\n" % (t["set"], t["layers"], t["fused_us"], t["torch_us"], t["fwd_us"],
                                                                          t["fused_over_torch"], t["fused_over_fwd"]))
            f.write("\n| layer | x | kernel | nnz | destinations | (a) us | (b) us | (c) us | (a)/(b) | (a)/(c) |\n")
            f.write("|---|---:|---|---:|---:|---:|---:|---:|---:|---:|\n")
            for r in rows:
                f.write("| %s | %d | %s | %d | %d | %.1f | %.1f | %.1f | %.3f | %.3f |\n" %
                        (r["layer"], r["count"], r["kernel"], r["nnz"], r["destinations"], r["fused_us"], r["torch_us"], r["fwd_us"],
                         r["fused_over_torch"], r["fused_over_fwd"]))
            f.write("\n```\n" + line + "\n```\n")


def make_sets(synth, names):
    sets = []
    for name in names.split(","):
        if name == "resnet":
            sets.append(("resnet50_3x3@90%", synth.resnet50_3x3(N=256, sparsity=0.9)))
        elif name == "alexnet":
            sets.append(("alexnet@80%", synth.alexnet(N=128, sparsity=0.8)))
        elif name == "googlenet":
            sets.append(("googlenet_1x1@95%", synth.googlenet_1x1(N=256, sparsity=0.95)))
    return sets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="resnet,alexnet,googlenet")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--realigns", type=int, default=3)
    ap.add_argument("--md", default=None)
    ap.add_argument("--solver", default=None, choices=["sgd", "nesterov", "adam"])
    a = ap.parse_args()
    if a.solver:
        return solver_main(a)
    import torch
    pkg = ge.load_package()
    synth = pkg.synth
    dev = torch.device("cuda:0")
    sets = make_sets(synth, a.sets)
    rows, totals = [], []
    k = 0
    for set_name, layers in sets:
        tot = dict(set=set_name, layers=0, update_us=0.0, realign_us=0.0, fwd_us=0.0)
        for s in layers:
            k += 1
            w = synth.pruned_weights(s, 1000 + k)
            b = synth.bias_vector(s, 2000 + k)
            x = torch.from_numpy(synth.activations(s, 3000 + k)).to(dev)
            W = torch.from_numpy(w).to(dev)
            bt = torch.from_numpy(b).to(dev) if b is not None else None
            plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
            plan.weight_align(W)
            top = plan.forward(x, bt)
            td = torch.empty_like(top).uniform_(-1, 1)
            bd = torch.empty_like(x)
            # (b) first: align from the device blob + the backward state's rebuild, as the parent needs after every step
            re = []
            for _ in range(a.realigns):
                plan.weight_align(W)
                plan.backward(td, bottom_diff=bd)
                torch.cuda.synchronize()
                re.append(plan.stat("align_us") + plan.stat("bwd_align_us"))
            re.sort()
            plan.update_values(W)            # builds the update state (the backward state exists: covered)
            torch.cuda.synchronize()
            assert plan.stat("update_fast") == 1, s.name
            r = dict(set=set_name, layer=s.name, count=s.count, N=s.N, nnz=plan.nnz(), kernel=plan.kernel_name,
                     destinations=plan.stat("update_destinations"), upd_device_mb=round(plan.stat("upd_device_bytes") / 1e6, 3),
                     realign_us=float(re[len(re) // 2]))
            r["update_us"] = timed(lambda: plan.update_values(W), a.regions, a.reps)
            r["fwd_us"] = timed(lambda: plan.forward(x, bt, top), a.regions, a.reps)
            r["update_over_realign"] = r["update_us"] / r["realign_us"]
            r["update_over_fwd"] = r["update_us"] / r["fwd_us"]
            rows.append(r)
            for key in ("update_us", "realign_us", "fwd_us"):
                tot[key] += r[key] * s.count
            tot["layers"] += s.count
            print("%-22s %-34s nnz %8d dst %9d  update %7.1f us  realign %9.0f us  fwd %7.1f us" %
                  (s.name, r["kernel"], r["nnz"], r["destinations"], r["update_us"], r["realign_us"], r["fwd_us"]), file=sys.stderr)
            plan.close()
            del x, W, top, td, bd
            torch.cuda.empty_cache()
        tot["update_over_realign"] = tot["update_us"] / tot["realign_us"]
        tot["update_over_fwd"] = tot["update_us"] / tot["fwd_us"]
        totals.append(tot)
    result = dict(tool="update_bench", regions=a.regions, reps=a.reps, realigns=a.realigns, totals=totals, layers=rows)
    line = json.dumps(result)
    print(line)
    if a.md:
        with open(a.md, "w") as f:
            f.write("| set | layers | (a) update_values, us | (b) weight_align + backward rebuild, us | (c) forward, us | (a)/(b) | (a)/(c) |\n")
            f.write("|---|---:|---:|---:|---:|---:|---:|\n")
            for t in totals:
                f.write("| %s | %d | %.1f | %.0f | %.1f | %.5f | %.3f |\n" % (t["set"], t["layers"], t["update_us"], t["realign_us"],
                                                                          t["fwd_us"], t["update_over_realign"], t["update_over_fwd"]))
            f.write("\n| layer | x | kernel | nnz | destinations | (a) us | (b) us | (c) us | (a)/(b) | (a)/(c) |\n")
            f.write("|---|---:|---|---:|---:|---:|---:|---:|---:|---:|\n")
            for r in rows:
                f.write("| %s | %d | %s | %d | %d | %.1f | %.0f | %.1f | %.5f | %.3f |\n" %
                        (r["layer"], r["count"], r["kernel"], r["nnz"], r["destinations"], r["update_us"], r["realign_us"], r["fwd_us"],
                         r["update_over_realign"], r["update_over_fwd"]))
            f.write("\n```\n" + line + "\n```\n")


if __name__ == "__main__":
    main()
