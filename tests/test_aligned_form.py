"""The persisted aligned form without a GPU (csrc/aligned_form.{h,cpp} through tests/cpp/aligned_form_check.cpp): compiled
with plain g++ and no ROCm include path -- that compile is the proof that the unit is host-only -- under the address and
undefined-behaviour sanitizers, and run as a stand-alone program.  The golden blobs (tests/golden/aligned_form_*.bin, an
MI355X's exports at the commit their sidecar names) parse and are written again byte for byte; programs generated on the
host round-trip; every mismatch of device or plan is "does not fit"; a damaged container is refused with its code and
message; and the code section, parsed directly, survives truncation at every boundary and every header field and tiling
int set to 0, 1, -1 and INT32_MAX without a sanitizer report."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PROGRAMS = ("k3p1", "k1", "k5p2g2")


def expected_lines(goldens):
    lines = []
    for name in goldens:
        lines += ["OK golden %s parse" % name, "OK golden %s rewrite" % name]
    for p in PROGRAMS:
        lines += ["OK host %s fields" % p, "OK host %s rewrite" % p]
    lines += ["OK nofit %s" % m for m in ("n_cu", "isa", "tiling_batch", "n_dense_groups", "dense_mask")]
    lines += ["OK outer %s" % c for c in ("flip_values", "flip_code", "splice", "magic", "total_bytes", "other_M", "nnz", "sizes")]
    for p in PROGRAMS:
        lines += ["OK code %s %s" % (p, c) for c in ("truncation", "header_fields", "tiling_ints", "unit_off", "chan")]
    return lines


def test_parsers_and_writers_on_the_host_under_sanitizers(tmp_path):
    with open(os.path.join(GOLDEN, "aligned_form.json")) as f:
        goldens = [c["file"] for c in json.load(f)["cases"]]
    assert len(goldens) == 2
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    exe = str(tmp_path / "aligned_form_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "aligned_form_check.cpp")] +
                          [os.path.join(csrc, s) for s in ("aligned_form.cpp", "align_rules.cpp", "stream_builder.cpp", "jit_codegen.cpp")])
    out = subprocess.run([exe] + [os.path.join(GOLDEN, g) for g in goldens], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode()
    assert out.returncode == 0, text
    assert text.splitlines() == expected_lines(goldens), text
