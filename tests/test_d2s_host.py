"""Plan option "deconv" without a GPU: the option's values and the refusals with their messages, and -- through
tests/cpp/d2s_tables_check.cpp, compiled with plain g++ and no ROCm include path (that compile is the proof that the code is
host-only) -- d2s_plan (the serve predicate, the top, the inner descriptor, the mirror convolution, the scratch and launch
sizes) and d2s_csr (the inner CSR and the entry map), each against a numpy restatement on every shape of d2s_common.SHAPES
and on 200 seeded random geometries.  Then the inner stride-1 convolution is evaluated in float64 from the printed tables
alone (dense inner weights scattered through the printed map), followed by the unpack rule, and compared with torch's float64
conv_transpose2d; the three gradients likewise through the pack rule, against autograd: the identity is pinned before any
GPU runs it.  Last, d2s_plan's size limits, each at its edge and one past it, with no allocation."""
import os
import subprocess

import numpy as np
import pytest

import d2s_common as dc

torch = pytest.importorskip("torch")
F = torch.nn.functional
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESTATE = "failed (-1)", "failed (-4)"


def _refused(pkg, fn, code, *words):
    with pytest.raises(pkg.EscoinError) as e:
        fn()
    assert code in str(e.value), str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_option_values_and_states(pkg):
    s = dc.make("k4s2p1")
    plan = pkg.Plan(dc.desc(pkg, s))
    plan.set_option("deconv", 1)
    plan.set_option("deconv", 0)
    for bad in (2, -1):
        _refused(pkg, lambda: plan.set_option("deconv", bad), EINVAL, "deconv")
    plan.set_option("deconv", 1)
    assert plan.stat("deconv") == 0 and plan.stat("deconv_scratch_bytes") == 0     # nothing is active before a device align
    plan.weight_align_cpu(dc.weights(s))
    for v in (0, 1):
        _refused(pkg, lambda: plan.set_option("deconv", v), ESTATE, "before")      # after the align
    plan.close()
    plan = pkg.Plan(dc.desc(pkg, s), deconv=1)                                     # the constructor passes options through
    assert plan.out_hw == dc.out_hw(s) == pkg.deconv_out_shape(dc.desc(pkg, s))
    plan.close()


def test_default_is_a_convolution(pkg):
    """Without the option the same descriptor is the convolution it always was: another top, another weight shape."""
    s = dc.make("k4s2p1")
    plan = pkg.Plan(dc.desc(pkg, s))
    assert plan.out_hw == pkg.out_shape(dc.desc(pkg, s)) != dc.out_hw(s)
    plan.weight_align_cpu(np.ones((s.M, s.C, s.KH, s.KW), np.float32))
    assert plan.nnz() == s.M * s.C * s.KH * s.KW and len(plan.get_csr()[0]) == s.M + 1
    plan.close()


def test_refusals_at_the_align_name_their_reason(pkg):
    s = dc.make("k3s2p1")
    w = dc.weights(s)
    # a dilation
    d = dc.desc(pkg, s)
    d.dil_h = 2
    d.pad_h = 2
    plan = pkg.Plan(d, deconv=1)
    _refused(pkg, lambda: plan.weight_align_cpu(w), EINVAL, "deconv", "dilation")
    plan.close()
    # an empty top: H = 1, K = 2, pad 1 crops everything (and is a valid convolution, which plan_create asks for)
    d = pkg.ConvDesc.deconvolution(1, 2, 1, 1, 2, 2, 1, 1)
    _refused(pkg, lambda: pkg.deconv_out_shape(d), EINVAL)
    plan = pkg.Plan(d)
    plan.set_option("deconv", 1)
    _refused(pkg, lambda: plan.weight_align_cpu(np.ones((2, 2, 2, 2), np.float32)), EINVAL, "deconv", "empty top")
    plan.close()
    # a double plan, through the _f64 entry point
    plan = pkg.Plan(dc.desc(pkg, s), deconv=1)
    _refused(pkg, lambda: plan.weight_align_cpu(w.astype(np.float64)), EINVAL, "deconv", "double")
    assert plan.stat("host_aligned") == 0
    plan.close()
    # together with another derived-plan option
    for other in ("s2d", "s2b", "b2s"):
        plan = pkg.Plan(dc.desc(pkg, s), deconv=1, **{other: 1})
        _refused(pkg, lambda: plan.weight_align_cpu(w), EINVAL, "deconv", other)
        plan.close()


def test_entry_points_not_carried_over_are_refused(pkg):
    s = dc.make("k3s2p1")
    plan = pkg.Plan(dc.desc(pkg, s), deconv=1)
    plan.weight_align_cpu(dc.weights(s))
    x, _, td = dc.inputs(s)
    _refused(pkg, lambda: plan.prune_cpu(keep=3), EINVAL, "deconv", "escoin_plan_prune")
    _refused(pkg, lambda: plan.rewire_cpu(1, np.ones(plan._dense_size(), np.float32)), EINVAL, "deconv", "escoin_plan_rewire")
    _refused(pkg, lambda: plan.dense_wgrad_cpu(td, x), EINVAL, "deconv", "escoin_dense_wgrad")
    plan.close()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """g++, -Icsrc -Iinclude, nothing of ROCm."""
    tmp = tmp_path_factory.mktemp("d2s")
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    out = str(tmp / "d2s_tables_check")
    srcs = [os.path.join(ROOT, "tests", "cpp", "d2s_tables_check.cpp")] + [
        os.path.join(csrc, f) for f in ("align_rules.cpp", "csr_tables.cpp", "stream_builder.cpp", "jit_codegen.cpp")]
    flags = ["g++", "-O1", "-std=c++17", "-Wall", "-I" + csrc, "-I" + os.path.join(ROOT, "include")]
    procs = [subprocess.Popen(flags + ["-c", s, "-o", str(tmp / (os.path.basename(s) + ".o"))]) for s in srcs]
    assert all(p.wait() == 0 for p in procs)
    subprocess.check_call(flags + ["-o", out] + [str(tmp / (os.path.basename(s) + ".o")) for s in srcs] + ["-lpthread"])
    return out


def _run(exe, tmp_path, s, csr=None, f64=False, bias=1, relu=0, dil=1):
    words = [s.N, s.C, s.H, s.W, s.M, s.KH, s.KW, s.pad_h, s.pad_w, s.stride_h, s.stride_w, dil, dil, s.group, bias, relu, int(f64),
             int(csr is not None)]
    if csr is not None:
        rp, ci, ng = csr
        cg, base = s.C // s.group, 0
        for grp in range(s.group):
            words += [int(v) for v in rp[grp * (cg + 1):(grp + 1) * (cg + 1)]]
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
        rows[parts[0]] = " ".join(parts[1:]) if parts[0] == "error" else np.array([int(v) for v in parts[1:]], np.int64)
    return rows


def _restate_csr(s, rp, ci, ng):
    """The inner CSR and the entry map restated: every outer entry's (inner row, inner column) by the contract's formula,
    sorted by (group, row, column)."""
    P, kh, kw, _, _ = dc.inner_dims(s)
    cg, mg = s.C // s.group, s.M // s.group
    rows_g = mg * P
    ent, base = [], 0
    for g in range(s.group):
        r = rp[g * (cg + 1):(g + 1) * (cg + 1)]
        for cl in range(cg):
            for j in range(r[cl], r[cl + 1]):
                col = int(ci[base + j])
                ml, kr, kc = col // (s.KH * s.KW), (col // s.KW) % s.KH, col % s.KW
                row, icol = dc.inner_position(s, g * cg + cl, ml, kr, kc)
                ent.append((g, row - g * rows_g, icol, base + j))
        base += int(ng[g])
    ent.sort()
    rowptr = np.zeros(s.group * (rows_g + 1), np.int64)
    for g, row, _, _ in ent:
        rowptr[g * (rows_g + 1) + row + 1:(g + 1) * (rows_g + 1)] += 1
    return rowptr.tolist(), [e[2] for e in ent], [e[3] for e in ent]


def _dense_inner(s, got, vals):
    """The inner layer's dense weights (M * P, Cg, KH', KW') in float64 from the printed CSR and entry map alone."""
    P, kh, kw, _, _ = dc.inner_dims(s)
    cg, rows_g = s.C // s.group, (s.M // s.group) * P
    w = np.zeros((s.M * P, cg * kh * kw), np.float64)
    base = 0
    for g in range(s.group):
        r = got["rowptr"][g * (rows_g + 1):(g + 1) * (rows_g + 1)]
        for m in range(rows_g):
            k = np.arange(r[m], r[m + 1]) + base
            if len(k):
                assert np.all(np.diff(got["colidx"][k]) > 0)                       # ascending inner columns
                w[g * rows_g + m, got["colidx"][k]] = np.asarray(vals, np.float64)[got["src"][k]]
        base += int(got["nnz_g"][g])
    return w.reshape(s.M * P, cg, kh, kw)


def _case(pkg, exe, tmp_path, s, w, seed=7):
    rp, ci, vals, ng = dc.csr_of(s, w)
    got = _run(exe, tmp_path, s, (rp, ci, ng), relu=1)
    assert got["serves"].tolist() == [1], got
    refused = _run(exe, tmp_path, s, f64=True)
    assert refused["serves"].tolist() == [0] and "double" in refused["error"]
    P, kh, kw, hi, wi = dc.inner_dims(s)
    oh, ow = dc.out_hw(s)
    assert got["top"].tolist() == [oh, ow]
    assert got["phases"].tolist() == [s.stride_h, s.stride_w, P]
    assert got["sizes"].tolist() == [s.N * s.M * P * hi * wi, s.N * s.M * oh * ow, s.N * s.M * oh, s.N * s.M * P * hi]
    # N, C, H x W, group and has_bias are the outer plan's; M' = M P; pad K' - 1, stride 1, dilation 1, no ReLU
    assert got["inner"].tolist() == [s.N, s.C, s.H, s.W, s.M * P, kh, kw, kh - 1, kw - 1, 1, 1, 1, 1, s.group, 1, 0]
    assert got["mirror"].tolist() == [s.N, s.M, oh, ow, s.C, s.KH, s.KW, s.pad_h, s.pad_w, s.stride_h, s.stride_w, 1, 1, s.group, 1, 1]
    rowptr, colidx, src = _restate_csr(s, rp, ci, ng)
    assert got["rowptr"].tolist() == rowptr
    assert got.get("colidx", np.zeros(0)).tolist() == colidx and got.get("src", np.zeros(0)).tolist() == src
    assert sorted(src) == list(range(len(ci)))                                     # a permutation of the outer entries
    assert got["nnz_g"].tolist() == [int(v) for v in ng]
    if len(ci):
        assert int(max(colidx)) < (s.C // s.group) * kh * kw
    # forward: the inner convolution of the bottom itself, then the unpack rule, equals conv_transpose2d
    wi64 = _dense_inner(s, got, vals)
    want_w, _ = dc.inner_weights(s, w)
    assert np.array_equal(wi64, want_w.astype(np.float64))
    x, b, td = (a.astype(np.float64) for a in dc.inputs(s, seed))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))  # noqa: E731
    errs = []
    for relu in (False, True):
        want = dc.ref_forward(s, w, x, b, relu)
        inner = F.conv2d(t(x), t(wi64), None, padding=(kh - 1, kw - 1), groups=s.group).numpy()
        assert inner.shape == (s.N, s.M * P, hi, wi)
        top = dc.unpack(s, inner, b, relu)
        errs.append(float(np.abs(top - want).max() / max(np.abs(want).max(), 1e-300)))
        # the three gradients: the inner layer's on G' = pack(top_diff, top), carried back through the map
        want_g = dc.ref_backward(s, w, x, b, td, top if relu else None)
        X, Wt = torch.tensor(x, requires_grad=True), torch.tensor(wi64, requires_grad=True)
        Bi = torch.zeros(s.M * P, dtype=torch.float64, requires_grad=True)
        F.conv2d(X, Wt, Bi, padding=(kh - 1, kw - 1), groups=s.group).backward(t(dc.pack(s, td, top if relu else None)))
        _, at = dc.inner_weights(s, w)
        wd = Wt.grad.numpy().reshape(-1)[at] * (w != 0)
        bd = Bi.grad.numpy().reshape(s.M, P).sum(axis=1)
        for a, c in zip((X.grad.numpy(), wd, bd), want_g):
            errs.append(float(np.abs(a - c).max() / max(np.abs(c).max(), 1e-300)))
    print(s.name, "inner conv from the tables vs torch float64 (forward, three gradients; linear, relu):", " ".join("%.2g" % e for e in errs))
    assert max(errs) <= 1e-12, (s.name, errs)


@pytest.mark.parametrize("name", list(dc.SHAPES))
def test_tables_equal_their_restatement_and_give_the_deconvolution(pkg, exe, tmp_path, name):
    s = dc.make(name)
    _case(pkg, exe, tmp_path, s, dc.weights(s))


def test_random_geometries(pkg, exe, tmp_path):
    shapes = dc.random_shapes()
    assert len(shapes) == 200
    for i, s in enumerate(shapes):
        _case(pkg, exe, tmp_path, s, dc.weights(s, 100 + i, density=0.5), seed=300 + i)


def test_an_empty_pattern_is_served(exe, tmp_path):
    s = dc.make("k3s2p1")
    got = _run(exe, tmp_path, s, (np.zeros(s.C + 1, np.int64), np.zeros(0, np.int64), np.array([0])))
    assert got["serves"].tolist() == [1] and got["nnz_g"].tolist() == [0] and np.all(got["rowptr"] == 0)
    assert len(got["rowptr"]) == s.M * 4 + 1


def test_refusals_of_the_rule(exe, tmp_path):
    s = dc.make("k3s2p1")
    got = _run(exe, tmp_path, s, dil=2)
    assert got["serves"].tolist() == [0] and "dilation" in got["error"]
    got = _run(exe, tmp_path, dc.DShape("empty", 1, 2, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1))
    assert got["serves"].tolist() == [0] and "empty top" in got["error"]
    got = _run(exe, tmp_path, dc.DShape("empty_w", 1, 2, 3, 1, 2, 2, 2, 1, 1, 0, 1, 1))
    assert got["serves"].tolist() == [0] and "empty top" in got["error"]


def test_size_limits_at_their_edges(exe, tmp_path):
    """Each limit at the last size that is served and at the first that is not; nothing is allocated."""
    S = dc.DShape

    def served(s):
        got = _run(exe, tmp_path, s)
        return int(got["serves"][0]), got.get("error", "")

    # the top blob: N * M * OH * OW = 2^31 with P = 1 (T' is the top's size)
    assert served(S("top_fits", (1 << 19) - 1, 1, 64, 64, 1, 1, 1, 1, 1, 0, 0, 1)) == (1, "")
    ok, why = served(S("top_2^31", 1 << 19, 1, 64, 64, 1, 1, 1, 1, 1, 0, 0, 1))
    assert ok == 0 and "top blob" in why
    # T': stride 2 under a 1 x 1 kernel, 2 x 2 bottom: top = 9 N, T' = 16 N
    assert served(S("t_fits", (1 << 27) - 1, 1, 2, 2, 1, 1, 1, 2, 2, 0, 0, 1)) == (1, "")
    ok, why = served(S("t_2^31", 1 << 27, 1, 2, 2, 1, 1, 1, 2, 2, 0, 0, 1))
    assert ok == 0 and "T'" in why
    # the inner weight matrix: M P Cg KH' KW' = 262136 x 8192 < 2^31 <= 262136 x 8193 (two groups of 32767 output channels)
    assert served(S("w_fits", 1, 2 * 8192, 1, 1, 65534, 2, 2, 2, 2, 0, 0, 2)) == (1, "")
    ok, why = served(S("w_2^31", 1, 2 * 8193, 1, 1, 65534, 2, 2, 2, 2, 0, 0, 2))
    assert ok == 0 and "weight matrix" in why
    # M * P: four channels per block of a grid axis of 65535 (three groups, so that a group stays within 32767)
    assert served(S("mp_fits", 1, 3, 2, 2, 65535, 2, 2, 2, 2, 0, 0, 3)) == (1, "")
    ok, why = served(S("mp_over", 1, 3, 2, 2, 65538, 2, 2, 2, 2, 0, 0, 3))
    assert ok == 0 and "channel limit" in why
    # output channels per group: the mirror convolution's input channels
    assert served(S("mg_fits", 1, 1, 2, 2, 32767, 1, 1, 1, 1, 0, 0, 1)) == (1, "")
    ok, why = served(S("mg_over", 1, 1, 2, 2, 32768, 1, 1, 1, 1, 0, 0, 1))
    assert ok == 0 and "32767" in why
    assert served(S("mg_groups", 1, 2, 2, 2, 65534, 1, 1, 1, 1, 0, 0, 2)) == (1, "")
