"""The MFMA weight-gradient kernel's host side without a GPU: the option value and the package constant, and -- through
tests/cpp/wgrad_mfma_tables_check.cpp, compiled with plain g++ and no ROCm include path (that compile is the proof that
the code is host-only) -- the serve predicate, the tile plan with the LDS bytes it reports and the tables derived from the
CSR, each against a numpy restatement on every shape of test_wgrad_mfma_gpu.py."""
import os
import subprocess

import numpy as np
import pytest

from wgrad_common import csr_positions
from wgrad_mfma_common import ALL, make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 64             # output channels x columns of a workgroup's tile
STEP = 32             # pixels per LDS step
LDS_BUDGET = 64 * 1024


def test_option_value_and_package_constant(pkg, synth):
    assert pkg.WGRAD_MFMA == 3
    assert (pkg.WGRAD_AUTO, pkg.WGRAD_ENTRY, pkg.WGRAD_STAGED) == (0, 1, 2)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(make(synth, "d_onepx")))
    plan.set_option("wgrad_kernel", 3)
    with pytest.raises(pkg.EscoinError) as e:
        plan.set_option("wgrad_kernel", 4)
    assert "failed (-1)" in str(e.value) and "wgrad_kernel" in str(e.value)      # ESCOIN_EINVAL
    with pytest.raises(pkg.EscoinError):
        plan.set_option("wgrad_kernel", -1)
    plan.set_option("wgrad_kernel", 0)
    plan.close()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """g++, -Icsrc -Iinclude, nothing of ROCm."""
    tmp = tmp_path_factory.mktemp("wgm")
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    out = str(tmp / "wgrad_mfma_tables_check")
    srcs = [os.path.join(ROOT, "tests", "cpp", "wgrad_mfma_tables_check.cpp")] + [
        os.path.join(csrc, f) for f in ("align_rules.cpp", "csr_tables.cpp", "stream_builder.cpp", "jit_codegen.cpp")]
    flags = ["g++", "-O1", "-std=c++17", "-Wall", "-I" + csrc, "-I" + os.path.join(ROOT, "include")]
    procs = [subprocess.Popen(flags + ["-c", s, "-o", str(tmp / (os.path.basename(s) + ".o"))]) for s in srcs]
    assert all(p.wait() == 0 for p in procs)
    subprocess.check_call(flags + ["-o", out] + [str(tmp / (os.path.basename(s) + ".o")) for s in srcs] + ["-lpthread"])
    return out


def _run(exe, tmp_path, s, rp, ci, ng, f64=False):
    mg = s.M // s.group
    words = [s.N, s.C, s.H, s.W, s.M, s.KH, s.KW, s.pad_h, s.pad_w, s.stride_h, s.stride_w, s.dil_h, s.dil_w, s.group, int(f64)]
    base = 0
    for grp in range(s.group):
        words += [int(v) for v in rp[grp * (mg + 1):(grp + 1) * (mg + 1)]]
        words += [int(v) for v in ci[base:base + int(ng[grp])]]
        base += int(ng[grp])
    path = str(tmp_path / "case.txt")
    with open(path, "w") as f:
        f.write(" ".join(str(w) for w in words) + "\n")
    out = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    text = out.stdout.decode()
    assert out.returncode == 0, text
    rows = {}
    for line in text.splitlines():
        parts = line.split()
        rows[parts[0]] = np.array([int(v) for v in parts[1:]], np.int64)
    return rows


@pytest.mark.parametrize("name", list(ALL))
def test_predicate_tile_plan_and_tables_equal_their_numpy_restatement(pkg, synth, exe, tmp_path, name):
    s = make(synth, name)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
    plan.weight_align_cpu(synth.pruned_weights(s, 11))
    rp, ci, _, ng = plan.get_csr()
    pos = csr_positions(plan)
    nnz = plan.nnz()
    plan.close()
    oh, ow = synth.out_hw(s)
    mg, cg = s.M // s.group, s.C // s.group
    kdim = cg * s.KH * s.KW
    got = _run(exe, tmp_path, s, rp, ci, ng)
    # the predicate: every float plan of these sizes; no double plan
    assert got["serves"].tolist() == [1]
    assert _run(exe, tmp_path, s, rp, ci, ng, f64=True)["serves"].tolist() == [0]
    # the tile plan
    mtiles, ktiles = -(-mg // TILE), -(-kdim // TILE)
    tile_m, tile_k, g_mt, g_kt, kpad, chunks, lds, budget = got["plan"].tolist()
    assert (tile_m, tile_k, g_mt, g_kt, kpad) == (TILE, TILE, mtiles, ktiles, ktiles * TILE)
    assert chunks == -(-s.N * oh * ow // 1024)
    # two buffers x (G tile, bottom tile) x 32 pixels x rows padded to 65 floats
    assert lds == 2 * 2 * STEP * (TILE + 1) * 4
    assert budget == LDS_BUDGET and 0 < lds <= budget
    # (row, column) -> entry: the exact inverse of csr_positions on the pattern, "no entry" everywhere else
    ent = got["ent"]
    assert ent.shape == (s.M * kdim,)
    want = np.full(s.M * kdim, -1, np.int64)
    want[pos] = np.arange(nnz)
    assert np.array_equal(ent, want)
    assert np.array_equal(ent[pos], np.arange(nnz)) and (ent >= 0).sum() == nnz
    # entries per tile
    cnt = np.zeros((s.group, mtiles, ktiles), np.int64)
    row, col = pos // kdim, pos % kdim
    np.add.at(cnt, (row // mg, (row % mg) // TILE, col // TILE), 1)
    assert np.array_equal(got["cnt"], cnt.reshape(-1)) and cnt.sum() == nnz
    # the im2col decode of column k = (ic * KH + kr) * KW + kc; the last tile's padding is marked invalid
    k = np.arange(kpad)
    ic, kr, kc = k // (s.KH * s.KW), (k // s.KW) % s.KH, k % s.KW
    valid = k < kdim
    ktab = np.stack([(ic * s.H + kr * s.dil_h) * s.W + kc * s.dil_w, kr * s.dil_h, kc * s.dil_w, np.ones_like(k)], 1)
    ktab[~valid] = 0
    assert np.array_equal(got["ktab"], ktab.reshape(-1))


def test_predicate_refuses_what_the_kernel_cannot_index(pkg, synth, exe, tmp_path):
    """N*OH*OW at 2^31 and beyond does not fit the kernel's pixel arithmetic; an empty pattern is still served (no launch)."""
    s = synth.shape("huge", 1 << 20, 1, 64, 32, 1, 1, sparsity=0.0)          # 2^31 pixels
    rp, ci, ng = np.array([0, 1]), np.array([0]), np.array([1])
    assert _run(exe, tmp_path, s, rp, ci, ng)["serves"].tolist() == [0]
    s = synth.shape("empty", 2, 4, 5, 5, 3, 3, pad=1, sparsity=0.0)
    got = _run(exe, tmp_path, s, np.zeros(4, np.int64), np.zeros(0, np.int64), np.array([0]))
    assert got["serves"].tolist() == [1]
    assert np.all(got["ent"] == -1) and np.all(got["cnt"] == 0)
