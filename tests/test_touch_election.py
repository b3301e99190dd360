"""Which workgroups of a tiled launch touch generated code with whole lines (csrc/align_rules.h touch_election) without a
GPU: tests/cpp/touch_election_check.cpp, compiled with plain g++ and no ROCm include path, enumerates every workgroup id
of every launch -- the BODY rows of tests/layout_cases.py and emulate_tiled.cpp's geometries, at the rows' own batch and at
256 images, on 256, 64 and 8 compute units, in launch order and grouped by XCD -- and checks that every set of
workgroups sharing an XCD and a grid row has a toucher, rank 0 first, that forced strides are honoured, that stride 1
marks every workgroup and that touch_lines() is the enumerated count."""
import os
import re
import subprocess

import layout_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_set_has_its_toucher_and_the_line_count_is_the_enumerated_one(tmp_path, synth):
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    exe = str(tmp_path / "touch_election_check")
    srcs = [os.path.join(ROOT, "tests", "cpp", "touch_election_check.cpp")] + [os.path.join(csrc, f) for f in
                                                                             ("align_rules.cpp", "stream_builder.cpp", "jit_codegen.cpp")]
    flags = ["g++", "-O2", "-std=c++17", "-I" + csrc, "-I" + os.path.join(ROOT, "include")]
    procs = [subprocess.Popen(flags + ["-c", s, "-o", str(tmp_path / (os.path.basename(s) + ".o"))]) for s in srcs]
    assert all(p.wait() == 0 for p in procs)
    subprocess.check_call(flags + ["-o", exe] + [str(tmp_path / (os.path.basename(s) + ".o")) for s in srcs] + ["-lpthread"])

    manifest = str(tmp_path / "rows.txt")
    with open(manifest, "w") as f:
        for row in lc.BODY:
            s = synth.shape(row.name, *row.dims, **row.kw)
            assert s.KH == s.KW and s.pad_h == s.pad_w and s.group == 1, row.name     # what a manifest line can say
            f.write("%s %d %d %d %d %d %d %d %r\n" % (row.name, s.N, s.C, s.H, s.W, s.M, s.KH, s.pad_h, float(s.sparsity)))
    out = subprocess.run([exe, manifest], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = out.stdout.decode()
    assert out.returncode == 0, text
    assert "all cases OK" in text and "FAILED" not in text, text
    m = re.search(r"rows=(\d+) geometries=(\d+) launches=(\d+) sets=(\d+)", text)
    rows, geoms, launches, sets = (int(v) for v in m.groups())
    # every row and geometry, each at 2 batches x 3 CU counts x 2 orders; far more sets than launches: the grids have
    # several rows and the XCDs several sets each
    assert rows == len(lc.BODY) and geoms == 44 and launches == 12 * (rows + geoms)
    assert sets > 8 * launches
