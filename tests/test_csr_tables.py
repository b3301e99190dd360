"""The tables derived from a plan's host CSR without a GPU (csrc/csr_tables.{h,cpp} through tests/cpp/csr_tables_check.cpp):
compiled with plain g++ against csr_tables.cpp alone and no ROCm include path -- that compile is the proof that the unit
is host-only -- every builder's output equals a brute-force restatement (dense scatter and scan, stable sort, the defining
formula) on seven small patterns: grouped with an asymmetric kernel, dilated with a short last channel block, strided,
with empty rows and channels, empty, one entry per row in the last column, fully dense.  The composition of two entry
maps (compose_maps) is checked on every pattern's own two maps, and once more against a result written out by hand."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("grouped", "dilated", "strided", "empty_rows", "empty", "lone", "dense")
BUILDERS = ("for_each_entry", "forward_transpose", "gather_transpose", "dense_positions kdim", "dense_positions padded",
            "generic_tables", "staged_tables", "entry_major", "compose_maps", "stretched_col")


def test_every_builder_equals_its_brute_force_restatement(tmp_path):
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    exe = str(tmp_path / "csr_tables_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "csr_tables_check.cpp"), os.path.join(csrc, "csr_tables.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    text = out.stdout.decode()
    assert out.returncode == 0, text
    lines = text.splitlines()
    assert "FAIL" not in text, text
    for case in CASES:
        for builder in BUILDERS:
            assert lines.count("OK %s %s" % (case, builder)) == 1, (case, builder, text)
    assert lines.count("OK by_hand compose_maps") == 1, text
    assert len(lines) == len(CASES) * len(BUILDERS) + 1, text
