#!/usr/bin/env python3
"""Generates tests/golden/aligned_form_*.bin and aligned_form.json -- run on an MI355X.

The persisted aligned form (escoin_plan_export_aligned) of two small generated-code plans, as the library at commit
`--commit` writes it: the blobs pin the format byte for byte (tests/test_aligned_form.py parses and rewrites them on the
host, tests/test_tools_gpu.py exports them again and imports them on the device).  Weights are synth.pruned_weights of
the shape and seed the sidecar records, so nothing but the blobs and the recipe needs to be kept.

    python tests/golden/make_aligned_form_golden.py --commit <id of the commit the library was built from> [--out DIR]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

TILING_BATCH = 4
W_SEED = 3100

# name, N, C, H, W, M, K, pad, group
CASES = [
    ("k3p1", 4, 32, 14, 14, 32, 3, 1, 1),
    ("k1g2", 4, 64, 28, 28, 32, 1, 0, 2),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    pkg = ge.load_package()
    synth = pkg.synth
    os.makedirs(args.out, exist_ok=True)
    side = {"commit": args.commit, "kernel": "KERNEL_JIT", "tiling_batch": TILING_BATCH, "cases": []}
    for k, (name, N, C, H, W, M, K, pad, group) in enumerate(CASES):
        s = synth.shape(name, N, C, H, W, M, K, pad=pad, group=group, bias=False, sparsity=0.9)
        seed = W_SEED + k
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s), kernel=pkg.KERNEL_JIT, tiling_batch=TILING_BATCH)
        plan.weight_align(synth.pruned_weights(s, seed))
        assert plan.stat("code_bytes") > 0, name
        blob = plan.export_aligned()
        fname = "aligned_form_%s.bin" % name
        blob.tofile(os.path.join(args.out, fname))
        side["cases"].append({"file": fname, "weights_seed": seed, "bytes": int(blob.size),
                              "code_bytes": plan.stat("code_bytes"), "kernel_name": plan.kernel_name,
                              "shape": {"N": N, "C": C, "H": H, "W": W, "M": M, "K": K, "pad": pad, "group": group,
                                        "sparsity": 0.9}})
        print("%-24s %7d bytes (code %d)  %s  %s" % (fname, blob.size, plan.stat("code_bytes"), plan.kernel_name,
                                                    plan.tiling_info))
        plan.close()
    with open(os.path.join(args.out, "aligned_form.json"), "w") as f:
        json.dump(side, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
