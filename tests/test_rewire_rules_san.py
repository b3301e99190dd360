"""The host-only half of rewiring without a GPU (csrc/rewire_rules.{h,cpp} on prune_rules, through
tests/cpp/rewire_rules_san.cpp): compiled with plain g++ and no ROCm include path -- that compile is the proof that the
unit is host-only -- under the address and undefined-behaviour sanitizers, and run as a stand-alone program over the
dense sizes of the rewiring tests."""
import os
import subprocess

import rewire_common as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def expected_lines():
    tile, scan_width, max_grid = rc.tile_positions()
    sizes = [63, 64, 65, tile + 1, tile + 128, tile * scan_width + 512, tile * max_grid + 257536]
    lines = []
    for t in ("float", "double"):
        lines += ["OK %s grow D=%d" % (t, n) for n in sizes] + ["OK %s grow without candidates" % t]
    lines += ["OK float merge", "OK double merge", "OK launch_plan"]
    return lines


def test_rewire_rules_on_the_host_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    exe = str(tmp_path / "rewire_rules_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + csrc, "-o", exe, os.path.join(ROOT, "tests", "cpp", "rewire_rules_san.cpp"),
                           os.path.join(csrc, "rewire_rules.cpp"), os.path.join(csrc, "prune_rules.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode()
    assert out.returncode == 0, text
    assert text.splitlines() == expected_lines(), text
