"""The value maps behind escoin_update_values, without a GPU (tests/cpp/value_map_check.cpp): for the generated-code
geometries of emulate_tiled.cpp and the same set through the stream builder, the map has one distinct in-range word per
CSR entry, that word holds the entry's bits, code generated from other values at the same pattern differs ONLY at mapped
words, and the old code patched through the map equals the new code word for word."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pattern_alone_shapes_code_and_stream(tmp_path):
    exe = str(tmp_path / "value_map_check")
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "value_map_check.cpp"),
                           os.path.join(csrc, "align_rules.cpp"), os.path.join(csrc, "stream_builder.cpp"), os.path.join(csrc, "jit_codegen.cpp"), "-lpthread"])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    text = out.stdout.decode()
    assert out.returncode == 0, text
    assert "all cases OK" in text and "FAILED" not in text
    jit = [l for l in text.splitlines() if l.startswith("jit ")]
    stream = [l for l in text.splitlines() if l.startswith("stream ")]
    assert len(jit) == 46 and len(stream) == 46
    forms = [(int(re.search(r"literals=(\d+)", l).group(1)), int(re.search(r"lines=(\d+)", l).group(1))) for l in jit]
    # both forms of a value in generated code are covered: literals behind a move, slots of a unit's weight lines ...
    assert sum(1 for a, b in forms if a > 0 and b == 0) >= 10 and sum(1 for a, b in forms if b > 0 and a == 0) >= 10
    # ... and both inside ONE program (units of more than 30 000 nonzeros keep their literals)
    assert any(a > 0 and b > 0 for a, b in forms)
    # four-wave workgroups, conv groups, chained units and chains generated on several threads (>= 20 000 nonzeros)
    assert sum("waves=4" in l for l in jit) >= 5 and sum(" g=2" in l for l in jit) >= 3 and sum("chained" in l for l in jit) >= 15
    assert sum(1 for l in jit if int(re.search(r": (\d+) nonzeros", l).group(1)) >= 20000) >= 2
