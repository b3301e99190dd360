#!/usr/bin/env python3
"""One pruning step from 80 % to 90 % sparsity on the MI355X, per layer and per set, two routes in the same run:
  (a) escoin_plan_prune on a plan in its training state (forward, backward and one device-source solver step done: the
      device holds the values), then escoin_compact_entries over two histories.  Phases: the selection / scan / map
      launches (device events, stat "prune_kernels_us"), the wall time until the host holds the map ("prune_map_us":
      launches + read-back), the re-align ("prune_realign_us"), the two compact launches (device events);
  (b) what a user does without it, on an identical plan in the same state: get_csr (reads the values back and waits),
      the same rule ranked with numpy (a stable argsort on the integer keys) and the kept CSR built on the host, set_csr,
      and the two histories re-indexed with torch.  Wall time each, the device idle before every phase.
Both routes end in the same re-align; the two maps are compared before anything is reported.

Sets: the four ResNet-50 3x3 shapes (batch 256, x their count in the net), AlexNet conv2-5 (batch 128), the GoogLeNet
1x1 layers (batch 256), all at 80 % sparsity.  Every figure is the median of --rounds rounds, each on freshly aligned
plans; the route that goes first alternates from round to round.  Prints one JSON line (progress on stderr); --md writes the table.

    python tools/prune_bench.py [--sets resnet,alexnet,googlenet] [--rounds 4] [--md out.md]

--rewire measures one drop-and-grow step instead, same protocol: per layer 10 % of the entries are dropped by magnitude
and as many grown where a dense random score is largest.
  (a) escoin_plan_rewire (stats "rewire_kernels_us", "rewire_map_us", "rewire_realign_us"), then escoin_compact_entries
      over two histories into zeroed arrays;
  (b) what the library offered before: escoin_plan_prune (one re-align), get_csr, the dense score copied to the host,
      masked and ranked with numpy and the merged CSR built there, set_csr (a second re-align), and the two histories
      re-indexed with torch.
Both routes must give the same maps, the same CSR bits and the same kernel before anything is reported.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402
from tools.update_bench import make_sets  # noqa: E402

HYPER = dict(type="sgd", regularization="L2", rate=1e-3, momentum=0.9, decay=5e-4)


def keys(v):
    u = np.ascontiguousarray(v).view(np.uint32)
    return u & np.uint32(0x7fffffff)


def numpy_map(values, keep):
    """The rule of include/escoin.h "Pruning" with numpy: a stable sort by descending key."""
    k = keys(values)
    order = np.argsort(np.uint32(0x7fffffff) - k, kind="stable")
    kept = np.zeros(k.size, bool)
    kept[order[:keep]] = True
    m = np.full(k.size, -1, np.int32)
    m[kept] = np.arange(keep, dtype=np.int32)
    return m, kept


def kept_csr(desc, rp, ng, kept):
    mg = desc.M // desc.group
    out_rp, out_ng = np.zeros_like(rp), np.zeros_like(ng)
    base = 0
    for grp in range(desc.group):
        r = rp[grp * (mg + 1):(grp + 1) * (mg + 1)]
        n = int(ng[grp])
        rows = np.repeat(np.arange(mg), np.diff(r))
        cnt = np.bincount(rows[kept[base:base + n]], minlength=mg)
        out_rp[grp * (mg + 1) + 1:(grp + 1) * (mg + 1)] = np.cumsum(cnt)
        out_ng[grp] = cnt.sum()
        base += n
    return out_rp, out_ng


def wall_us(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, out


def event_us(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3, out


def training_state(pkg, s, W, x, bt, dev):
    """A plan aligned on W after a forward, a backward and one device-source solver step, with its two histories."""
    import torch
    torch.manual_seed(4321)          # the two routes' plans see the same gradient
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
    plan.weight_align(W)
    top = plan.forward(x, bt)
    td = torch.empty_like(top).uniform_(-1, 1)
    n = plan.nnz()
    _, vd, _ = plan.backward(td, bottom=x, bottom_diff=torch.empty_like(x), values_diff=True)
    h, h2 = torch.zeros(n, device=dev), torch.ones(n, device=dev)
    plan.solver_step(vd, h, None, **HYPER)
    torch.cuda.synchronize()
    return plan, h, h2


def one_round(pkg, s, k, dev, a_first):
    import torch
    synth = pkg.synth
    W = torch.from_numpy(synth.pruned_weights(s, 1000 + k)).to(dev)
    b = synth.bias_vector(s, 2000 + k)
    bt = torch.from_numpy(b).to(dev) if b is not None else None
    x = torch.from_numpy(synth.activations(s, 3000 + k)).to(dev)
    total = s.M * (s.C // s.group) * s.KH * s.KW
    keep = int(round(0.1 * total))
    r = {}
    def route_a():
        plan, h, h2 = training_state(pkg, s, W, x, bt, dev)
        r["nnz_before"] = plan.nnz()
        r["kernel_before"] = plan.kernel_name
        r["a_total_us"], entry_map = wall_us(lambda: plan.prune(keep=keep))
        r["a_kernels_us"] = plan.stat("prune_kernels_us")
        r["a_map_us"] = plan.stat("prune_map_us")
        r["a_realign_us"] = plan.stat("prune_realign_us")
        out1, out2 = torch.empty(keep, device=dev), torch.empty(keep, device=dev)
        r["a_compact_us"], _ = event_us(lambda: (pkg.compact_entries(entry_map, h, out=out1), pkg.compact_entries(entry_map, h2, out=out2)))
        r["a_total_us"] += r["a_compact_us"]
        r["nnz_after"] = plan.nnz()
        r["kernel_after"] = plan.kernel_name
        res = entry_map.cpu().numpy(), plan.get_csr()[2]
        plan.close()
        return res

    def route_b():
        plan, h, h2 = training_state(pkg, s, W, x, bt, dev)
        r["b_get_csr_us"], (rp, ci, va, ng) = wall_us(plan.get_csr)

        def rank():
            m, kept = numpy_map(va, keep)
            new_rp, new_ng = kept_csr(plan.desc, rp, ng, kept)
            return m, kept, new_rp, ci[kept], va[kept], new_ng

        r["b_rank_us"], (m, kept, new_rp, new_ci, new_va, new_ng) = wall_us(rank)
        r["b_set_csr_us"], _ = wall_us(lambda: plan.set_csr(new_rp, new_ci, new_va, new_ng))

        def reindex():
            idx = torch.from_numpy(np.flatnonzero(kept)).to(dev)
            return h[idx], h2[idx]

        r["b_reindex_us"], _ = wall_us(reindex)
        r["b_total_us"] = r["b_get_csr_us"] + r["b_rank_us"] + r["b_set_csr_us"] + r["b_reindex_us"]
        res = m, plan.get_csr()[2], plan.kernel_name
        plan.close()
        return res

    # the route that runs first also pays for whatever the process meets first on this layer: the rounds alternate
    if a_first:
        (map_a, vals_a), (map_b, vals_b, kernel_b) = route_a(), route_b()
    else:
        (map_b, vals_b, kernel_b), (map_a, vals_a) = route_b(), route_a()
    assert np.array_equal(map_a, map_b), s.name
    assert vals_a.tobytes() == vals_b.tobytes() and kernel_b == r["kernel_after"], s.name
    del W, x
    torch.cuda.empty_cache()
    return r


def positions_of(desc, rp, ng, ci):
    mg, kdim = desc.M // desc.group, (desc.C // desc.group) * desc.KH * desc.KW
    out, base = [], 0
    for grp in range(desc.group):
        r = rp[grp * (mg + 1):(grp + 1) * (mg + 1)]
        n = int(ng[grp])
        rows = np.repeat(np.arange(mg, dtype=np.int64), np.diff(r)) + grp * mg
        out.append(rows * kdim + ci[base:base + n])
        base += n
    return np.concatenate(out)


def csr_of(desc, pos):
    mg, kdim = desc.M // desc.group, (desc.C // desc.group) * desc.KH * desc.KW
    cnt = np.bincount(pos // kdim, minlength=desc.M).reshape(desc.group, mg)
    rp = np.zeros((desc.group, mg + 1), np.int32)
    rp[:, 1:] = np.cumsum(cnt, axis=1)
    return rp.ravel(), (pos % kdim).astype(np.int32), cnt.sum(axis=1).astype(np.int32)


def one_round_rewire(pkg, s, k, dev, a_first):
    import torch
    synth = pkg.synth
    W = torch.from_numpy(synth.pruned_weights(s, 1000 + k)).to(dev)
    b = synth.bias_vector(s, 2000 + k)
    bt = torch.from_numpy(b).to(dev) if b is not None else None
    x = torch.from_numpy(synth.activations(s, 3000 + k)).to(dev)
    D = s.M * (s.C // s.group) * s.KH * s.KW
    score = torch.empty(D, device=dev).uniform_(-1, 1, generator=torch.Generator(device=dev).manual_seed(5000 + k))
    r = {}

    def route_a():
        plan, h, h2 = training_state(pkg, s, W, x, bt, dev)
        n = plan.nnz()
        k10 = n // 10
        r["nnz_before"], r["kernel_before"] = n, plan.kernel_name
        r["a_total_us"], (entry_map, grown) = wall_us(lambda: plan.rewire(k10, score, drop_keep=n - k10))
        r["a_kernels_us"] = plan.stat("rewire_kernels_us")
        r["a_map_us"] = plan.stat("rewire_map_us")
        r["a_realign_us"] = plan.stat("rewire_realign_us")
        new_nnz = plan.nnz()

        def carry():
            out1, out2 = torch.zeros(new_nnz, device=dev), torch.zeros(new_nnz, device=dev)
            return pkg.compact_entries(entry_map, h, out=out1), pkg.compact_entries(entry_map, h2, out=out2)

        r["a_compact_us"], (h_new, _) = event_us(carry)
        r["a_total_us"] += r["a_compact_us"]
        r["nnz_after"], r["kernel_after"] = new_nnz, plan.kernel_name
        res = entry_map.cpu().numpy(), grown.cpu().numpy(), plan.get_csr(), h_new.cpu().numpy()
        plan.close()
        return res

    def route_b():
        plan, h, h2 = training_state(pkg, s, W, x, bt, dev)
        n = plan.nnz()
        k10 = n // 10
        rp0, ci0, _, ng0 = plan.get_csr()          # (the pattern before the step: a training loop has it already)
        old_pos = positions_of(plan.desc, rp0, ng0, ci0)
        r["b_prune_us"], drop_map = wall_us(lambda: plan.prune(keep=n - k10))
        r["b_get_csr_us"], ((rp, ci, va, ng), drop_np) = wall_us(lambda: (plan.get_csr(), drop_map.cpu().numpy()))

        def rank():
            sc = score.cpu().numpy()
            free = np.ones(D, bool)
            free[old_pos] = False
            cand = np.flatnonzero(free)
            kk = keys(sc[cand])
            order = np.argsort(np.uint32(0x7fffffff) - kk, kind="stable")
            grown_pos = np.sort(cand[order[:k10]])
            kept_pos = old_pos[drop_np >= 0]
            new_pos = np.sort(np.concatenate([kept_pos, grown_pos]))
            final_map = np.full(n, -1, np.int32)
            final_map[drop_np >= 0] = np.searchsorted(new_pos, kept_pos).astype(np.int32)
            grown = np.searchsorted(new_pos, grown_pos).astype(np.int32)
            vals = np.zeros(new_pos.size, np.float32)
            vals[final_map[drop_np >= 0]] = va
            new_rp, new_ci, new_ng = csr_of(plan.desc, new_pos)
            return final_map, grown, new_rp, new_ci, vals, new_ng

        r["b_rank_us"], (final_map, grown, new_rp, new_ci, vals, new_ng) = wall_us(rank)
        r["b_set_csr_us"], _ = wall_us(lambda: plan.set_csr(new_rp, new_ci, vals, new_ng))

        def reindex():
            kept = torch.from_numpy(np.flatnonzero(final_map >= 0)).to(dev)
            to = torch.from_numpy(final_map[final_map >= 0].astype(np.int64)).to(dev)
            out1, out2 = torch.zeros(vals.size, device=dev), torch.zeros(vals.size, device=dev)
            out1[to], out2[to] = h[kept], h2[kept]
            return out1, out2

        r["b_reindex_us"], (h_new, _) = wall_us(reindex)
        r["b_total_us"] = r["b_prune_us"] + r["b_get_csr_us"] + r["b_rank_us"] + r["b_set_csr_us"] + r["b_reindex_us"]
        res = final_map, grown, plan.get_csr(), h_new.cpu().numpy(), plan.kernel_name
        plan.close()
        return res

    if a_first:
        (map_a, grown_a, csr_a, h_a), (map_b, grown_b, csr_b, h_b, kernel_b) = route_a(), route_b()
    else:
        (map_b, grown_b, csr_b, h_b, kernel_b), (map_a, grown_a, csr_a, h_a) = route_b(), route_a()
    assert np.array_equal(map_a, map_b) and np.array_equal(grown_a, grown_b), s.name
    assert all(p.tobytes() == q.tobytes() for p, q in zip(csr_a, csr_b)) and h_a.tobytes() == h_b.tobytes(), s.name
    assert kernel_b == r["kernel_after"], s.name
    del W, x, score
    torch.cuda.empty_cache()
    return r


NUM_REWIRE = ("a_kernels_us", "a_map_us", "a_realign_us", "a_compact_us", "a_total_us", "b_prune_us", "b_get_csr_us", "b_rank_us", "b_set_csr_us", "b_reindex_us", "b_total_us")


def main_rewire(a):
    import torch
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    rows, totals = [], []
    k = 0
    for set_name, layers in make_sets(pkg.synth, a.sets):
        set_name = set_name.split("@")[0] + "@80%, 10% rewired"
        tot = dict(set=set_name, layers=0, **{key: 0.0 for key in NUM_REWIRE})
        for s in layers:
            k += 1
            s = s._replace(sparsity=0.8)
            rounds = [one_round_rewire(pkg, s, k, dev, (i % 2 == 0) != (a.first == "b")) for i in range(a.rounds)]
            r = dict(set=set_name, layer=s.name, count=s.count, N=s.N, **{key: rounds[0][key] for key in ("nnz_before", "nnz_after", "kernel_before", "kernel_after")})
            for key in NUM_REWIRE:
                r[key] = float(np.median([q[key] for q in rounds]))
                tot[key] += r[key] * s.count
            tot["layers"] += s.count
            rows.append(r)
            print("%-22s nnz %8d  (a) kernels %6.0f  map %7.0f  realign %8.0f  compact %5.0f  total %8.0f us | (b) prune %8.0f  get_csr %7.0f  rank %8.0f  set_csr %8.0f  reindex %6.0f  total %8.0f us" %
                  ((s.name, r["nnz_before"]) + tuple(r[key] for key in NUM_REWIRE)), file=sys.stderr)
        tot["a_over_b"] = tot["a_total_us"] / tot["b_total_us"]
        totals.append(tot)
    line = json.dumps(dict(tool="prune_bench --rewire", rounds=a.rounds, totals=totals, layers=rows))
    print(line)
    if a.md:
        with open(a.md, "w") as f:
            head = "| %s | x | nnz | (a) all launches | (a) until the host has the map | (a) re-align | (a) 2 compact launches | (a) total | (b) prune | (b) get_csr + map | (b) numpy rank + merge | (b) set_csr | (b) 2 re-indexes | (b) total | (a)/(b) |\n"
            f.write("All times in microseconds, median of %d rounds; (a) escoin_plan_rewire + escoin_compact_entries, (b) escoin_plan_prune, get_csr, numpy, set_csr.\n\n" % a.rounds)
            f.write(head % "set")
            f.write("|---|" + "---:|" * 14 + "\n")
            for t in totals:
                f.write(("| %s | %d | |" + " %.0f |" * 11 + " %.3f |\n") % ((t["set"], t["layers"]) + tuple(t[key] for key in NUM_REWIRE) + (t["a_over_b"],)))
            f.write("\n" + head % "layer")
            f.write("|---|" + "---:|" * 14 + "\n")
            for r in rows:
                f.write(("| %s | %d | %d |" + " %.0f |" * 11 + " %.3f |\n") % ((r["layer"], r["count"], r["nnz_before"]) + tuple(r[key] for key in NUM_REWIRE) + (r["a_total_us"] / r["b_total_us"],)))
            f.write("\n```\n" + line + "\n```\n")


NUM = ("a_kernels_us", "a_map_us", "a_realign_us", "a_compact_us", "a_total_us", "b_get_csr_us", "b_rank_us", "b_set_csr_us", "b_reindex_us", "b_total_us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="resnet,alexnet,googlenet")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--first", default="a", choices=["a", "b"], help="the route that goes first in even rounds (they alternate)")
    ap.add_argument("--md", default=None)
    ap.add_argument("--rewire", action="store_true", help="measure one drop-and-grow step (escoin_plan_rewire) instead of a pruning step")
    a = ap.parse_args()
    if a.rewire:
        return main_rewire(a)
    import torch
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    rows, totals = [], []
    k = 0
    for set_name, layers in make_sets(pkg.synth, a.sets):
        set_name = set_name.split("@")[0] + "@80%->90%"
        tot = dict(set=set_name, layers=0, **{key: 0.0 for key in NUM})
        for s in layers:
            k += 1
            s = s._replace(sparsity=0.8)
            rounds = [one_round(pkg, s, k, dev, (i % 2 == 0) != (a.first == "b")) for i in range(a.rounds)]
            r = dict(set=set_name, layer=s.name, count=s.count, N=s.N, **{key: rounds[0][key] for key in ("nnz_before", "nnz_after", "kernel_before", "kernel_after")})
            for key in NUM:
                r[key] = float(np.median([q[key] for q in rounds]))
                tot[key] += r[key] * s.count
            tot["layers"] += s.count
            rows.append(r)
            print("%-22s nnz %8d -> %8d  (a) kernels %6.0f  map %7.0f  realign %8.0f  compact %5.0f  total %8.0f us | (b) get_csr %7.0f  rank %8.0f  set_csr %8.0f  reindex %6.0f  total %8.0f us" %
                  (s.name, r["nnz_before"], r["nnz_after"], r["a_kernels_us"], r["a_map_us"], r["a_realign_us"], r["a_compact_us"], r["a_total_us"],
                   r["b_get_csr_us"], r["b_rank_us"], r["b_set_csr_us"], r["b_reindex_us"], r["b_total_us"]), file=sys.stderr)
        tot["a_over_b"] = tot["a_total_us"] / tot["b_total_us"]
        totals.append(tot)
    result = dict(tool="prune_bench", rounds=a.rounds, totals=totals, layers=rows)
    line = json.dumps(result)
    print(line)
    if a.md:
        with open(a.md, "w") as f:
            head = "| %s | x | nnz before | nnz after | (a) select + scan + map launches | (a) until the host has the map | (a) re-align | (a) 2 compact launches | (a) total | (b) get_csr | (b) numpy rank + CSR | (b) set_csr | (b) 2 re-indexes | (b) total | (a)/(b) |\n"
            f.write("All times in microseconds, median of %d rounds; (a) escoin_plan_prune + escoin_compact_entries, (b) get_csr, numpy, set_csr.\n\n" % a.rounds)
            f.write(head % "set")
            f.write("|---|" + "---:|" * 14 + "\n")
            for t in totals:
                f.write("| %s | %d | | | %.0f | %.0f | %.0f | %.0f | %.0f | %.0f | %.0f | %.0f | %.0f | %.0f | %.3f |\n" %
                        (t["set"], t["layers"], t["a_kernels_us"], t["a_map_us"], t["a_realign_us"], t["a_compact_us"], t["a_total_us"],
                         t["b_get_csr_us"], t["b_rank_us"], t["b_set_csr_us"], t["b_reindex_us"], t["b_total_us"], t["a_over_b"]))
            f.write("\n" + head % "layer")
            f.write("|---|" + "---:|" * 14 + "\n")
            for r in rows:
                f.write("| %s | %d | %d | %d | %.0f | %.0f | %.0f | %.0f | %.0f | %.0f | %.0f | %.0f | %.0f | %.0f | %.3f |\n" %
                        (r["layer"], r["count"], r["nnz_before"], r["nnz_after"], r["a_kernels_us"], r["a_map_us"], r["a_realign_us"], r["a_compact_us"],
                         r["a_total_us"], r["b_get_csr_us"], r["b_rank_us"], r["b_set_csr_us"], r["b_reindex_us"], r["b_total_us"], r["a_total_us"] / r["b_total_us"]))
            f.write("\n```\n" + line + "\n```\n")


if __name__ == "__main__":
    main()
