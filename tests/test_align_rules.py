"""WeightAlign's rules without a GPU (csrc/align_rules.{h,cpp} through tests/cpp/align_rules_check.cpp): compiled with
plain g++ and no ROCm include path -- that compile is the proof that the rules are host-only -- they give every case
of tests/golden/align_cases.json (the benched layer sets and one case per branch of the rules) the kernel and the layout
the library gave it on an MI355X (tests/golden/align_decisions_mi355x.json, recorded by tools/align_fingerprint.py
with the library of the commit BEFORE the rules moved)."""
import importlib.util
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "align_decisions_mi355x.json")
FIELDS = ("kernel_choice", "tiling_info", "small_launch_rule", "lds_bytes", "workgroup_columns", "code_bytes", "jit_rows",
          "jit_records", "wgrad_kernel", "wgrad_lds_bytes")
OPTIONS = (("kernel", 0), ("conv_mode", 3), ("dense_gate", 0), ("dense_threshold_pct", -1), ("tiling_batch", 0), ("wgrad_kernel", 0))


def fingerprint_tool():
    spec = importlib.util.spec_from_file_location("align_fingerprint", os.path.join(ROOT, "tools", "align_fingerprint.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_host_rules(tmp_path):
    """tests/cpp/align_rules_check.cpp against the rules and the two builders: g++, -Icsrc -Iinclude, nothing of ROCm."""
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    exe = str(tmp_path / "align_rules_check")
    srcs = [os.path.join(ROOT, "tests", "cpp", "align_rules_check.cpp")] + [os.path.join(csrc, f) for f in
                                                                          ("align_rules.cpp", "stream_builder.cpp", "jit_codegen.cpp")]
    flags = ["g++", "-O2", "-std=c++17", "-I" + csrc, "-I" + os.path.join(ROOT, "include")]
    # (one compiler per source, four at a time)
    procs = [subprocess.Popen(flags + ["-c", s, "-o", str(tmp_path / (os.path.basename(s) + ".o"))]) for s in srcs]
    assert all(p.wait() == 0 for p in procs)
    subprocess.check_call(flags + ["-o", exe] + [str(tmp_path / (os.path.basename(s) + ".o")) for s in srcs] + ["-lpthread"])
    return exe


def host_rules(exe, tmp_path, synth, cases, n_cu):
    """What the rules decide for `cases` on a device of n_cu compute units: one dict per case."""
    tool = fingerprint_tool()
    lines = []
    for i, c in enumerate(cases):
        path = str(tmp_path / ("w%d.f32" % i))
        tool.case_weights(synth, c).astype(np.float32).tofile(path)
        opts = tool.case_options(c)
        assert set(opts) <= {k for k, _ in OPTIONS}, opts
        row = [c["shape"][k] for k in tool.SHAPE_FIELDS[:-1]] + [opts.get(k, d) for k, d in OPTIONS] + [int(bool(c.get("f64"))), n_cu]
        lines.append(" ".join(str(int(v)) for v in row) + " " + path)
    manifest = str(tmp_path / "manifest.txt")
    with open(manifest, "w") as f:
        f.write("\n".join(lines) + "\n")
    out = subprocess.run([exe, manifest], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = out.stdout.decode()
    assert out.returncode == 0, text
    got = [json.loads(l) for l in text.splitlines()]
    assert len(got) == len(cases) and all(r["error"] == "" for r in got), text
    return got


def test_host_rules_reproduce_the_recorded_decisions(tmp_path, synth):
    tool = fingerprint_tool()
    cases = tool.load_cases()
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert set(golden["cases"]) == {c["name"] for c in cases} and len(cases) == len(golden["cases"])
    got = host_rules(build_host_rules(tmp_path), tmp_path, synth, cases, golden["n_cu"])
    bad = ["%s.%s: rules %r, recorded %r" % (c["name"], k, r[k], golden["cases"][c["name"]][k])
           for c, r in zip(cases, got) for k in FIELDS if r[k] != golden["cases"][c["name"]][k]]
    assert not bad, "\n".join(bad)
    # the record covers the branches it is there for
    rec = golden["cases"]
    assert "nbuf=3" in rec["three_buffers"]["tiling_info"] and "oc_waves=4" in rec["half_workgroups"]["tiling_info"]
    assert rec["small_launch_generic"]["small_launch_rule"] == 2 and rec["small_launch_code"]["small_launch_rule"] == 1
    assert rec["stream_layout"]["tiling_info"].startswith("stream ") and rec["stream_layout"]["kernel_choice"] == 2
    assert rec["dense_by_model"]["kernel_choice"] == 3 and rec["sparse_above_cut"]["kernel_choice"] == 4
    assert rec["dilated_dense"]["kernel_choice"] == 3 and rec["dilated_generic"]["kernel_choice"] == 1
    assert rec["mixed_groups"]["kernel_name"].endswith("+ escoin_dense_mfma_kernel")
    assert rec["wgrad_entry"]["wgrad_kernel"] == 1 and rec["wgrad_staged"]["wgrad_kernel"] == 2
