#!/usr/bin/env python3
"""GPU box: which kernel and layout WeightAlign gives every case of tests/golden/align_cases.json, as integers, strings
and hashes -- the record a change that only MOVES WeightAlign's rules must reproduce exactly.

    ESCOIN_LIB=<library of the commit to record> python tools/align_fingerprint.py --write tests/golden/align_decisions_mi355x.json
    python tools/align_fingerprint.py --check tests/golden/align_decisions_mi355x.json

Per case: kernel_choice, kernel_name, tiling_info, the layout stats, the sha256 of the exported aligned form (tiling,
channel deal, unit table and every code word) and, after one backward of one image, the backward's kernels.  Only the
public binding and synth are used, so the same script runs against any build of the library (ESCOIN_LIB).

case_shape / case_options / case_weights are also what the tests of the host-only rules (tests/test_align_rules*.py)
build their inputs with."""
import argparse
import hashlib
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "golden", "align_cases.json")

STATS = ("small_launch_rule", "lds_bytes", "workgroup_columns", "code_bytes", "jit_rows", "jit_records",
         "deal_slowest_over_mean_x1000", "deal_worst_block_x1000", "device_bytes")
BWD_STATS = ("bwd_data_kernel", "wgrad_kernel", "wgrad_lds_bytes", "bwd_device_bytes")
SHAPE_FIELDS = ("N", "C", "H", "W", "M", "KH", "KW", "pad_h", "pad_w", "stride_h", "stride_w", "dil_h", "dil_w", "group", "bias")


def load_cases(only=None):
    with open(CASES) as f:
        cases = json.load(f)["cases"]
    return [c for c in cases if only is None or c["set"] == only]


def case_shape(synth, c):
    """The case as a synth.ConvShape (sparsity: the first group's)."""
    sp = c["sparsity"]
    return synth.ConvShape(c["name"], *[c["shape"][k] for k in SHAPE_FIELDS], sparsity=sp[0] if isinstance(sp, list) else sp)


def case_options(c):
    return dict(c.get("options", {}))


def case_weights(synth, c):
    """blobs_[0] of the case: synth's pruned weights for its seed; "sparsity" as a list prunes every conv group to its
    own figure (group g of the weights synth makes for the whole layer at sparsity[g]); "f64" cases in double."""
    s = case_shape(synth, c)
    sp = c["sparsity"]
    if isinstance(sp, list):
        mg = s.M // s.group
        w = np.concatenate([synth.pruned_weights(s._replace(sparsity=sp[g]), c["seed"], c["dist"])[g * mg:(g + 1) * mg]
                            for g in range(s.group)])
    else:
        w = synth.pruned_weights(s, c["seed"], c["dist"])
    return w.astype(np.float64) if c.get("f64") else w


def fingerprint(pkg, torch, c):
    synth = pkg.synth
    s = case_shape(synth, c)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s), **case_options(c))
    plan.weight_align(case_weights(synth, c))
    rec = {"kernel_choice": plan.stat("kernel_choice"), "kernel_name": plan.kernel_name, "tiling_info": plan.tiling_info}
    for k in STATS:
        rec[k] = plan.stat(k)
    # (a double plan has no aligned form beyond its CSR: that is what its hash covers)
    blobs = plan.get_csr() if c.get("f64") else (plan.export_aligned(),)
    rec["aligned_sha256"] = hashlib.sha256(b"".join(np.ascontiguousarray(b).tobytes() for b in blobs)).hexdigest()
    # the backward's decisions depend on desc.N, not on the images of the call: one image keeps the run short
    dt = torch.float64 if c.get("f64") else torch.float32
    oh, ow = plan.out_hw
    x = torch.zeros((1, s.C, s.H, s.W), device="cuda:0", dtype=dt)
    g = torch.zeros((1, s.M, oh, ow), device="cuda:0", dtype=dt)
    plan.backward(g, bottom=x, weight_diff=True, bias_diff=True)
    torch.cuda.synchronize()
    for k in BWD_STATS:
        rec[k] = plan.stat(k)
    plan.close()
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", metavar="JSON", help="record every case into this file")
    ap.add_argument("--check", metavar="JSON", help="compare every field of every case with this record")
    ap.add_argument("--set", help="only the cases of this set (layer sets by name, \"branch\")")
    args = ap.parse_args()
    if bool(args.write) == bool(args.check):
        ap.error("one of --write / --check")
    import torch
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("caffe-escoin_amd")
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    got = {}
    for c in load_cases(args.set):
        got[c["name"]] = dict(fingerprint(pkg, torch, c), n_cu=n_cu)
        print("%-34s %s  %s" % (c["name"], got[c["name"]]["kernel_name"], got[c["name"]]["tiling_info"]), flush=True)
    if args.write:
        with open(args.write, "w") as f:
            f.write('{"device": %s, "n_cu": %d, "cases": {\n' % (json.dumps(torch.cuda.get_device_name(0)), n_cu))
            f.write(",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in got.items()))
            f.write("\n}}\n")
        print("align_fingerprint: recorded %d cases on %d CUs into %s" % (len(got), n_cu, args.write))
        return 0
    with open(args.check) as f:
        want = json.load(f)["cases"]
    bad = 0
    for name, rec in got.items():
        diff = sorted(k for k in set(rec) | set(want.get(name, {})) if rec.get(k) != want.get(name, {}).get(k))
        for k in diff:
            print("MISMATCH %s.%s: got %r, recorded %r" % (name, k, rec.get(k), want.get(name, {}).get(k)))
        bad += bool(diff)
    fields = sum(len(r) for r in got.values())
    print("align_fingerprint: %d of %d cases match the record in every field (%d fields, %d CUs)%s"
          % (len(got) - bad, len(got), fields, n_cu, "" if not bad else " -- FAILED"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
