"""The host-only half of pruning without a GPU (csrc/prune_rules.{h,cpp} through tests/cpp/prune_rules_san.cpp): compiled
with plain g++ and no ROCm include path -- that compile is the proof that the unit is host-only -- under the address and
undefined-behaviour sanitizers, and run as a stand-alone program over the score cases and sizes of the pruning tests."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def expected_lines():
    with open(os.path.join(ROOT, "caffe-escoin_amd", "csrc", "prune_rules.h")) as f:
        text = f.read()
    tile = int(re.search(r"kThreads = (\d+);", text).group(1)) * int(re.search(r"kItems = (\d+);", text).group(1))
    sizes = [1, 2, 63, 64, 65, tile - 1, tile, tile + 1, 3 * tile + 1, 0]
    lines = []
    for t in ("float", "double"):
        lines += ["OK %s selection n=%d" % (t, n) for n in sizes]
    lines += ["OK float apply_entry_map", "OK double apply_entry_map", "OK launch_plan"]
    return lines


def test_prune_rules_on_the_host_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    exe = str(tmp_path / "prune_rules_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + csrc, "-o", exe, os.path.join(ROOT, "tests", "cpp", "prune_rules_san.cpp"),
                           os.path.join(csrc, "prune_rules.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode()
    assert out.returncode == 0, text
    assert text.splitlines() == expected_lines(), text
