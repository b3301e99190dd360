#!/usr/bin/env python3
"""Generates tests/golden/ref_results.json -- run where oracle/_ref is built (it needs the reference tree at build time).

Records what the reference's own CPU kernel (oracle/_ref) computes for the live cases of tests/test_oracle.py: the
SHA-256 of every whole-batch case's top blob (float32 bytes; the test asserts bit-exact equality, so equal digests
are the same check) and the two single-image outputs as plain numbers.  Data only.

    python tests/golden/make_ref_results.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import __graft_entry__ as ge  # noqa: E402
import test_oracle as t  # noqa: E402


def main():
    oracle = ge.load_oracle()
    synth = ge.load_package().synth
    if not oracle.have_ref():
        oracle.build()
    if not oracle.have_ref():
        raise SystemExit("oracle/_ref is not built (needs the reference tree)")
    live = {}
    for k, s in enumerate(t._live_cases(synth)):
        g, x, w, b = t._live_inputs(oracle, synth, k, s)
        live[s.name] = t._digest(oracle.ref_conv_forward(g, x, w, b, threads=2))
    s, g, padded, rp, ci, va, bias = t._single_image_inputs(oracle, synth)
    plain = oracle.ref_sconv(g, padded, s.C, rp, ci, va, s.M)
    fused = oracle.ref_sconv(g, padded, s.C, rp, ci, va, s.M, bias=bias, relu=True)
    out = {"live": live,
           "single_image": {"shape": list(plain.shape), "plain": [float(v) for v in plain.ravel()],
                            "fused": [float(v) for v in fused.ravel()]}}
    with open(os.path.join(HERE, "ref_results.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
