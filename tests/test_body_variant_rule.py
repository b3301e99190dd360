"""Which compiled body a generated-code plan's launches run (csrc/align_rules.h body_variant) without a GPU:
tests/cpp/body_variant_check.cpp, compiled with plain g++ and no ROCm include path, gives the chained body to the 16
benched ResNet-50 3x3 layers of tests/golden/align_cases.json (four shapes, benched 3 + 4 + 6 + 3 times) and the
generic body to a stream-layout plan and to generated code that is not chained."""
import json
import os
import subprocess

import numpy as np

from test_align_rules import OPTIONS, fingerprint_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "align_decisions_mi355x.json")


def test_rule_picks_the_chained_body_for_the_benched_layers(tmp_path, synth):
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    exe = str(tmp_path / "body_variant_check")
    srcs = [os.path.join(ROOT, "tests", "cpp", "body_variant_check.cpp")] + [os.path.join(csrc, f) for f in
                                                                           ("align_rules.cpp", "stream_builder.cpp", "jit_codegen.cpp")]
    flags = ["g++", "-O2", "-std=c++17", "-I" + csrc, "-I" + os.path.join(ROOT, "include")]
    procs = [subprocess.Popen(flags + ["-c", s, "-o", str(tmp_path / (os.path.basename(s) + ".o"))]) for s in srcs]
    assert all(p.wait() == 0 for p in procs)
    subprocess.check_call(flags + ["-o", exe] + [str(tmp_path / (os.path.basename(s) + ".o")) for s in srcs] + ["-lpthread"])

    tool = fingerprint_tool()
    with open(GOLDEN) as f:
        golden = json.load(f)
    resnet = [c for c in tool.load_cases() if c["set"] == "resnet50_3x3"]
    # (the cases are the benched set's shapes: the benchmark runs each `count` times)
    bench = {s.name: s for s in synth.resnet50_3x3()}
    assert sum(s.count for s in bench.values()) == 16 and len(resnet) == len(bench)
    for c in resnet:
        assert tool.case_shape(synth, c)[1:15] == bench[c["name"]][1:15] and c["sparsity"] == bench[c["name"]].sparsity
    others = [c for c in tool.load_cases() if c["name"] in ("stream_layout", "lenet_conv2")]
    assert len(others) == 2
    cases = resnet + others
    lines = []
    for i, c in enumerate(cases):
        path = str(tmp_path / ("w%d.f32" % i))
        tool.case_weights(synth, c).astype(np.float32).tofile(path)
        opts = tool.case_options(c)
        row = [c["shape"][k] for k in tool.SHAPE_FIELDS[:-1]] + [opts.get(k, d) for k, d in OPTIONS] + [0, golden["n_cu"]]
        lines.append(" ".join(str(int(v)) for v in row) + " " + path)
    manifest = str(tmp_path / "manifest.txt")
    with open(manifest, "w") as f:
        f.write("\n".join(lines) + "\n")
    out = subprocess.run([exe, manifest], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = out.stdout.decode()
    assert out.returncode == 0, text
    got = {c["name"]: json.loads(l) for c, l in zip(cases, text.splitlines())}
    assert len(got) == len(cases), text
    for c in cases:     # the layouts are the recorded ones
        assert got[c["name"]]["tiling_info"] == golden["cases"][c["name"]]["tiling_info"], c["name"]
    for c in resnet:
        assert "chained=1" in got[c["name"]]["tiling_info"] and got[c["name"]]["body_variant"] == 1, got[c["name"]]
    assert got["stream_layout"]["tiling_info"].startswith("stream ") and got["stream_layout"]["body_variant"] == 0
    assert "generated-code" in got["lenet_conv2"]["tiling_info"] and "chained=0" in got["lenet_conv2"]["tiling_info"]
    assert got["lenet_conv2"]["body_variant"] == 0
