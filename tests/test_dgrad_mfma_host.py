"""The MFMA data-gradient kernel's host side without a GPU: the option value and the package constant, and -- through
tests/cpp/dgrad_mfma_tables_check.cpp, compiled with plain g++ and no ROCm include path (that compile is the proof that
the code is host-only) -- the serve predicate, the tile plan with the LDS bytes it reports and the tables derived from the
CSR, each against a numpy restatement on every shape of test_dgrad_mfma_gpu.py.  Then the kernel's GEMM is evaluated in
float64 from the printed tables alone (phases, column decode, matrix places, live steps) and compared with torch's
float64 data gradient: the phase decomposition is pinned before any GPU runs it."""
import os
import subprocess

import numpy as np
import pytest

from dgrad_mfma_common import SHAPES, make, phases, random_shapes, weights
from wgrad_common import seeded, torch_backward

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 64             # input channels x phase pixels of a workgroup's tile
STEP = 32             # columns per LDS step
LDS_BUDGET = 64 * 1024


def test_option_value_and_package_constant(pkg, synth):
    assert pkg.BWD_MFMA == 5
    assert pkg.BWD_MFMA not in (pkg.KERNEL_AUTO, pkg.KERNEL_GENERIC, pkg.KERNEL_TILED, pkg.KERNEL_DENSE, pkg.KERNEL_JIT)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(make(synth, "3x3_s2")))
    plan.set_option("backward_kernel", 5)
    for bad in (6, -1):
        with pytest.raises(pkg.EscoinError) as e:
            plan.set_option("backward_kernel", bad)
        assert "failed (-1)" in str(e.value) and "backward_kernel" in str(e.value)      # ESCOIN_EINVAL
    with pytest.raises(pkg.EscoinError) as e:
        plan.set_option("kernel", 5)
    assert "failed (-1)" in str(e.value)
    plan.set_option("backward_kernel", 0)
    plan.close()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """g++, -Icsrc -Iinclude, nothing of ROCm."""
    tmp = tmp_path_factory.mktemp("dgm")
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    out = str(tmp / "dgrad_mfma_tables_check")
    srcs = [os.path.join(ROOT, "tests", "cpp", "dgrad_mfma_tables_check.cpp")] + [
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


def _entries(s, rp, ci, ng):
    """(grp, ocl, ic, kr, kc) of every CSR entry, in get_csr()'s order."""
    mg = s.M // s.group
    grp, ocl = [], []
    for g in range(s.group):
        r = rp[g * (mg + 1):(g + 1) * (mg + 1)]
        grp += [g] * int(ng[g])
        ocl += np.repeat(np.arange(mg), np.diff(r)).tolist()
    ci = np.asarray(ci, np.int64)
    return (np.array(grp, np.int64), np.array(ocl, np.int64), ci // (s.KH * s.KW), (ci // s.KW) % s.KH, ci % s.KW)


def _check_tables(synth, s, got, rp, ci, ng):
    """The printed plan and tables against their restatement in numpy."""
    oh, ow = synth.out_hw(s)
    mg, cg = s.M // s.group, s.C // s.group
    want = phases(s)
    P = s.stride_h * s.stride_w
    ctiles = -(-cg // TILE)
    ntaps = [len(p["taps"]) for p in want]
    ksteps = [-(-mg * t // STEP) for t in ntaps]
    col0 = np.concatenate([[0], np.cumsum([k * STEP for k in ksteps])])
    tiles = [-(-s.N * p["rows"] * p["cols"] // TILE) for p in want]
    tile_c, tile_p, step_k, ph_h, ph_w, g_ct, tiles_max, cols_total, mat_floats, lds, budget = got["plan"].tolist()
    assert (tile_c, tile_p, step_k, ph_h, ph_w, g_ct) == (TILE, TILE, STEP, s.stride_h, s.stride_w, ctiles)
    assert got["tiles"].tolist() == tiles and tiles_max == max(tiles)
    assert cols_total == col0[-1] and mat_floats == s.group * ctiles * TILE * cols_total
    # two buffers x (weight block, G block) x 32 columns x rows padded to 65 floats
    assert lds == 2 * 2 * STEP * (TILE + 1) * 4 and budget == LDS_BUDGET and 0 < lds <= budget
    # every bottom pixel belongs to exactly one phase, every tap to exactly one phase
    cover = np.zeros((s.H, s.W), np.int64)
    for p in want:
        cover[p["h0"]::s.stride_h, p["w0"]::s.stride_w] += 1
        assert cover[p["h0"]::s.stride_h, p["w0"]::s.stride_w].shape == (p["rows"], p["cols"])
    assert np.all(cover == 1) and sum(ntaps) == s.KH * s.KW
    ph = got["phase"].reshape(P, 8)
    assert ph.tolist() == [[p["h0"], p["w0"], p["rows"], p["cols"], mg * t, k, c, t]
                           for p, t, k, c in zip(want, ntaps, ksteps, col0[:-1])]
    assert got["tap_ptr"].tolist() == np.concatenate([[0], np.cumsum(ntaps)]).tolist()
    assert got["taps"].tolist() == [kr << 8 | kc for p in want for kr, kc, _, _ in p["taps"]]
    # the column decode: k = ocl * ntaps + t; the last step's padding is marked invalid
    col = np.zeros((cols_total, 4), np.int64)
    for p, t, c in zip(want, ntaps, col0[:-1]):
        for ocl in range(mg):
            for ti, (_, _, dh, dw) in enumerate(p["taps"]):
                col[c + ocl * t + ti] = (ocl * oh * ow, dh, dw, 1)
    assert np.array_equal(got["col"].reshape(-1, 4), col)
    # every entry's one place in the phase matrices, and the live steps
    grp, ocl, ic, kr, kc = _entries(s, rp, ci, ng)
    nnz = len(ic)
    phase_of = (kr * s.dil_h % s.stride_h) * s.stride_w + kc * s.dil_w % s.stride_w
    tap_of = np.array([[(a, b) for a, b, _, _ in want[p]["taps"]].index((r, c)) for p, r, c in zip(phase_of, kr, kc)], np.int64)
    k = ocl * np.array(ntaps, np.int64)[phase_of] + tap_of
    ct = ic // TILE
    pos = ((grp * ctiles + ct) * cols_total + col0[phase_of] + k) * TILE + ic % TILE
    assert np.array_equal(got["pos"][:nnz], pos) and len(np.unique(pos)) == nnz and np.all(pos < mat_floats)
    live = [[] for _ in range(s.group * P * ctiles)]
    for li, st in sorted(set(zip(((grp * P + phase_of) * ctiles + ct).tolist(), (k // STEP).tolist()))):
        live[li].append(st)
    assert got["live_ptr"].tolist() == np.concatenate([[0], np.cumsum([len(v) for v in live])]).tolist()
    flat = [st for v in live for st in v]
    assert got["live"].tolist() == (flat if flat else [0])


def _gemm_from_tables(s, synth, got, vals, td):
    """What the kernel computes, in float64, read off the printed tables alone: per (group, phase, channel tile) the live
    steps ascending, per column the weights of its 64 channels from the matrix and G through the column's decode."""
    oh, ow = synth.out_hw(s)
    mg, cg = s.M // s.group, s.C // s.group
    P = s.stride_h * s.stride_w
    _, _, _, _, _, ctiles, _, cols_total, mat_floats, _, _ = got["plan"].tolist()
    mat = np.zeros(mat_floats, np.float64)
    mat[got["pos"][:len(vals)]] = vals
    mat = mat.reshape(s.group * ctiles, cols_total, TILE)
    col = got["col"].reshape(-1, 4)
    G = np.asarray(td, np.float64)
    dx = np.full((td.shape[0], s.C, s.H, s.W), np.nan)
    for grp in range(s.group):
        Gg = G[:, grp * mg:(grp + 1) * mg].reshape(td.shape[0], mg * oh * ow)
        for p in range(P):
            h0, w0, rows, cols, kp, ksteps, col0, _ = got["phase"][8 * p:8 * p + 8].tolist()
            hh, ww = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
            for ct in range(ctiles):
                li = (grp * P + p) * ctiles + ct
                acc = np.zeros((td.shape[0], TILE, rows, cols))
                for st in got["live"][got["live_ptr"][li]:got["live_ptr"][li + 1]].tolist():
                    assert 0 <= st < ksteps
                    for k in range(st * STEP, (st + 1) * STEP):
                        goff, dh, dw, valid = col[col0 + k].tolist()
                        if not valid:
                            assert k >= kp and not mat[grp * ctiles + ct, col0 + k].any()
                            continue
                        y, x = hh + dh, ww + dw
                        ok = (y >= 0) & (y < oh) & (x >= 0) & (x < ow)
                        g = np.where(ok[None], Gg[:, goff + np.where(ok, y * ow + x, 0)], 0.0)
                        acc += mat[grp * ctiles + ct, col0 + k][None, :, None, None] * g[:, None]
                nch = min(TILE, cg - ct * TILE)
                assert not mat[grp * ctiles + ct, :, nch:].any()
                c_lo = grp * cg + ct * TILE
                dx[:, c_lo:c_lo + nch, h0::s.stride_h, w0::s.stride_w] = acc[:, :nch]
    return dx


def _case(pkg, synth, exe, tmp_path, s, w):
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
    plan.weight_align_cpu(w)
    rp, ci, vals, ng = plan.get_csr()
    plan.close()
    got = _run(exe, tmp_path, s, rp, ci, ng)
    # the predicate: every float plan of these sizes; no double plan
    assert got["serves"].tolist() == [1]
    assert _run(exe, tmp_path, s, rp, ci, ng, f64=True)["serves"].tolist() == [0]
    _check_tables(synth, s, got, rp, ci, ng)
    td = seeded((s.N, s.M) + synth.out_hw(s), 21, np.float64)
    x = np.zeros((s.N, s.C, s.H, s.W))
    want = torch_backward(x, w, None, s, td)[0]
    dx = _gemm_from_tables(s, synth, got, vals, td)
    assert not np.isnan(dx).any(), "a bottom pixel no phase wrote"
    err = float(np.abs(dx - want).max() / max(np.abs(want).max(), 1e-300))
    print(s.name, "GEMM from the tables vs torch float64: rel err %.3g" % err)
    assert err <= 1e-12, s.name


@pytest.mark.parametrize("name", list(SHAPES))
def test_plan_and_tables_equal_their_restatement_and_give_the_data_gradient(pkg, synth, exe, tmp_path, name):
    s = make(synth, name)
    _case(pkg, synth, exe, tmp_path, s, weights(synth, s))


def test_random_geometries(pkg, synth, exe, tmp_path):
    for i, s in enumerate(random_shapes(synth)):
        _case(pkg, synth, exe, tmp_path, s, synth.pruned_weights(s, 100 + i))


def test_predicate_refuses_what_the_kernel_cannot_index(pkg, synth, exe, tmp_path):
    """N*H*W at 2^31 does not fit the kernel's pixel arithmetic; an empty pattern is still served (every tile writes zeros)."""
    s = synth.shape("huge", 1 << 20, 1, 64, 32, 1, 1, sparsity=0.0)          # 2^31 pixels
    rp, ci, ng = np.array([0, 1]), np.array([0]), np.array([1])
    assert _run(exe, tmp_path, s, rp, ci, ng)["serves"].tolist() == [0]
    s = synth.shape("empty", 2, 4, 5, 5, 3, 3, pad=1, stride=2, sparsity=0.0)
    got = _run(exe, tmp_path, s, np.zeros(4, np.int64), np.zeros(0, np.int64), np.array([0]))
    assert got["serves"].tolist() == [1]
    assert np.all(got["live_ptr"] == 0) and got["pos"].tolist() == [0]
