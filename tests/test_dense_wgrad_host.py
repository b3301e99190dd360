"""The dense weight gradient's host side without a GPU: the option, the package's symbols and -- through
tests/cpp/dense_wgrad_plan_check.cpp, compiled with plain g++ and no ROCm include path (that compile is the proof that
the code is host-only) -- align_rules.h dwg_plan against a numpy restatement of its rule at 256 CUs, on the benched layer
geometries (ResNet, AlexNet, GoogLeNet sets) and on every shape of test_dense_wgrad_gpu.py, and csr_tables.h im2col_ktab
against the ktab of wgrad_mfma_tables."""
import os
import subprocess

import pytest

from dense_wgrad_common import LDS, MAX_ROUNDS, RESIDENT_PER_CU, TILE, split_cost
from dense_wgrad_common import rule as _rule
from wgrad_mfma_common import ALL, make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CU = 256


def rule(s, synth, n_cu=N_CU, max_splits=0):
    return _rule(s, synth.out_hw(s), n_cu, max_splits)


def test_option_and_symbols(pkg, synth):
    for name in ("escoin_dense_wgrad", "escoin_dense_wgrad_f64", "escoin_dense_wgrad_cpu", "escoin_dense_wgrad_cpu_f64"):
        assert name in pkg.API_SYMBOLS and hasattr(pkg.lib(), name)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(make(synth, "d_onepx")))
    plan.set_option("dense_wgrad_splits", 0)
    plan.set_option("dense_wgrad_splits", 3)
    with pytest.raises(pkg.EscoinError) as e:
        plan.set_option("dense_wgrad_splits", -1)
    assert "failed (-1)" in str(e.value) and "dense_wgrad_splits" in str(e.value)      # ESCOIN_EINVAL
    # nothing has been built: the stats are zero, and the workspace does not count a state that is not there
    for key in ("dwg_device_bytes", "dwg_splits", "dwg_lds_bytes", "dwg_count"):
        assert plan.stat(key) == 0
    with pytest.raises(pkg.EscoinError):
        plan.stat("dwg_nonsense")
    plan.weight_align_cpu(synth.pruned_weights(make(synth, "d_onepx"), 11))
    plan.close()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """g++, -Icsrc -Iinclude, nothing of ROCm."""
    tmp = tmp_path_factory.mktemp("dwg")
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    out = str(tmp / "dense_wgrad_plan_check")
    srcs = [os.path.join(ROOT, "tests", "cpp", "dense_wgrad_plan_check.cpp")] + [
        os.path.join(csrc, f) for f in ("align_rules.cpp", "csr_tables.cpp", "stream_builder.cpp", "jit_codegen.cpp")]
    flags = ["g++", "-O1", "-std=c++17", "-Wall", "-I" + csrc, "-I" + os.path.join(ROOT, "include")]
    procs = [subprocess.Popen(flags + ["-c", s, "-o", str(tmp / (os.path.basename(s) + ".o"))]) for s in srcs]
    assert all(p.wait() == 0 for p in procs)
    subprocess.check_call(flags + ["-o", out] + [str(tmp / (os.path.basename(s) + ".o")) for s in srcs] + ["-lpthread"])
    return out


def _run(exe, tmp_path, cases):
    """cases: (shape, is_f64, n_cu, max_splits).  Returns one dict of rows per case."""
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        for s, f64, n_cu, ms in cases:
            f.write(" ".join(str(int(v)) for v in (s.N, s.C, s.H, s.W, s.M, s.KH, s.KW, s.pad_h, s.pad_w, s.stride_h, s.stride_w,
                                                  s.dil_h, s.dil_w, s.group, f64, n_cu, ms)) + "\n")
    out = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = out.stdout.decode()
    assert out.returncode == 0, text
    res = []
    for line in text.splitlines():
        parts = line.split()
        if parts[0] == "serves":
            res.append({})
        res[-1][parts[0]] = [int(v) for v in parts[1:]]
    assert len(res) == len(cases), text
    return res


def _layers(synth):
    benched = synth.resnet50_3x3() + synth.alexnet() + synth.googlenet_1x1()
    return benched + [make(synth, name) for name in ALL]


def _check(s, synth, got, n_cu, ms):
    what = (s.name, n_cu, ms)
    assert got["serves"] == [1], what
    mtiles, ktiles, chunks, span, splits, D, slab = rule(s, synth, n_cu, ms)
    assert got["plan"] == [mtiles, ktiles, chunks, span, splits, D, slab, LDS], what
    g_span, g_splits = got["plan"][3], got["plan"][4]
    # every chunk is covered once and no span is empty
    assert got["cover"] == [1, 1] and got["empty"] == [0], what
    assert g_splits * g_span >= chunks and 1 <= g_splits <= chunks, what
    tiles = s.group * mtiles * ktiles
    # a split never asks for more rounds of resident workgroups than the rule allows, and no other admissible span is cheaper
    assert g_splits == 1 or tiles * g_splits <= MAX_ROUNDS * RESIDENT_PER_CU * n_cu, what
    if tiles >= MAX_ROUNDS * RESIDENT_PER_CU * n_cu:
        assert g_splits == 1, what
    mine = split_cost(tiles, chunks, g_span, n_cu)
    for span in range(1, chunks + 1):
        n = -(-chunks // span)
        if n == 1 or ((ms == 0 or n <= ms) and tiles * n <= MAX_ROUNDS * RESIDENT_PER_CU * n_cu):
            assert mine <= split_cost(tiles, chunks, span, n_cu), (what, span)
    if ms > 0:
        assert g_splits <= ms, what
    # the slab is splits x D floats
    assert got["plan"][6] == 4 * g_splits * s.M * (s.C // s.group) * s.KH * s.KW, what
    kpad = ktiles * TILE
    assert got["ktab_equal"] == [1, 4 * kpad], what


def test_split_rule_on_the_benched_layers_and_the_test_shapes(synth, exe, tmp_path):
    layers = _layers(synth)
    cases = [(s, 0, N_CU, ms) for s in layers for ms in (0, 1, 2, 5)]
    got = _run(exe, tmp_path, cases)
    for (s, _, n_cu, ms), g in zip(cases, got):
        _check(s, synth, g, n_cu, ms)
    by_name = {s.name: g for (s, _, _, ms), g in zip(cases, got) if ms == 0}
    # res2 3x3 at batch 256: 9 tiles, 784 chunks -> 112 spans of 7 chunks, 1008 workgroups: one round of the 1024 resident;
    # res5 3x3: 576 tiles, 13 chunks -> 7 spans of 2 chunks, 4032 workgroups: four rounds of two chunks
    assert by_name["res2_branch2b"]["plan"][2:5] == [784, 7, 112]
    assert by_name["res5_branch2b"]["plan"][2:5] == [13, 2, 7]


def test_other_cu_counts_and_refusals(synth, exe, tmp_path):
    s = synth.resnet50_3x3()[0]
    cases = [(s, 0, n_cu, 0) for n_cu in (1, 64, 304, 100000)]
    for (c, g) in zip(cases, _run(exe, tmp_path, cases)):
        _check(c[0], synth, g, c[2], 0)
    # a double plan, and N*OH*OW at 2^31, are refused (wgm_plan's predicate)
    huge = synth.shape("huge", 1 << 20, 1, 64, 32, 1, 1, sparsity=0.0)
    got = _run(exe, tmp_path, [(s, 1, N_CU, 0), (huge, 0, N_CU, 0)])
    assert got[0]["serves"] == [0] and got[1]["serves"] == [0]
