"""Plan option "s2d" without a GPU: the option's values and refusals, and -- through tests/cpp/s2d_tables_check.cpp,
compiled with plain g++ and no ROCm include path (that compile is the proof that the code is host-only) -- the serve
predicate, the inner descriptor, the inner CSR and the entry map s2d_src, each against a numpy restatement on every shape of
test_s2d_gpu.py.  Then the inner stride-1 convolution is evaluated in float64 from the printed tables alone (dense inner
weights scattered through s2d_src, X' by the pack rule) and compared with torch's float64 conv2d of the OUTER layer, and
the same for the data gradient through the unpack rule: the identity is pinned before any GPU runs it."""
import os
import subprocess

import numpy as np
import pytest

from s2d_common import SHAPES, UNSERVED, inner_dims, make, pack, random_shapes, unpack
from wgrad_common import seeded, torch_backward

torch = pytest.importorskip("torch")
F = torch.nn.functional
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_values_and_refusals(pkg, synth):
    s = make(synth, "3x3_s2")
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
    plan.set_option("s2d", 1)
    plan.set_option("s2d", 0)
    for bad in (2, -1):
        with pytest.raises(pkg.EscoinError) as e:
            plan.set_option("s2d", bad)
        assert "failed (-1)" in str(e.value) and "s2d" in str(e.value)      # ESCOIN_EINVAL
    plan.set_option("s2d", 1)
    assert plan.stat("s2d") == 0 and plan.stat("s2d_scratch_bytes") == 0   # nothing is active before a device align
    plan.weight_align_cpu(synth.pruned_weights(s, 11))
    for v in (0, 1):
        with pytest.raises(pkg.EscoinError) as e:
            plan.set_option("s2d", v)                                       # after the align
        assert "failed (-4)" in str(e.value) and "before" in str(e.value)   # ESCOIN_ESTATE
    plan.close()
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s), s2d=1)                      # the constructor passes options through
    plan.close()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """g++, -Icsrc -Iinclude, nothing of ROCm."""
    tmp = tmp_path_factory.mktemp("s2d")
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    out = str(tmp / "s2d_tables_check")
    srcs = [os.path.join(ROOT, "tests", "cpp", "s2d_tables_check.cpp")] + [
        os.path.join(csrc, f) for f in ("align_rules.cpp", "csr_tables.cpp", "stream_builder.cpp", "jit_codegen.cpp")]
    flags = ["g++", "-O1", "-std=c++17", "-Wall", "-I" + csrc, "-I" + os.path.join(ROOT, "include")]
    procs = [subprocess.Popen(flags + ["-c", s, "-o", str(tmp / (os.path.basename(s) + ".o"))]) for s in srcs]
    assert all(p.wait() == 0 for p in procs)
    subprocess.check_call(flags + ["-o", out] + [str(tmp / (os.path.basename(s) + ".o")) for s in srcs] + ["-lpthread"])
    return out


def _run(exe, tmp_path, s, rp, ci, ng, f64=False, relu=0):
    mg = s.M // s.group
    words = [s.N, s.C, s.H, s.W, s.M, s.KH, s.KW, s.pad_h, s.pad_w, s.stride_h, s.stride_w, s.dil_h, s.dil_w, s.group,
             int(bool(s.bias)), relu, int(f64)]
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


def _restate_csr(s, synth, rp, ci, ng):
    """The inner CSR and s2d_src restated: per row the outer entries by ascending inner column."""
    ph_n, pw_n, _, _, _, kh, kw = inner_dims(s, synth)
    mg = s.M // s.group
    ci = np.asarray(ci, np.int64)
    ic, kr, kc = ci // (s.KH * s.KW), (ci // s.KW) % s.KH, ci % s.KW
    cin = (ic * ph_n + kr % s.stride_h) * pw_n + kc % s.stride_w
    col = (cin * kh + kr // s.stride_h) * kw + kc // s.stride_w
    colidx, src = [], []
    base = 0
    for g in range(s.group):
        r = rp[g * (mg + 1):(g + 1) * (mg + 1)]
        for m in range(mg):
            e = np.arange(r[m], r[m + 1]) + base
            order = np.argsort(col[e], kind="stable")
            assert len(np.unique(col[e])) == len(e), "the map is injective within a row"
            colidx += col[e][order].tolist()
            src += e[order].tolist()
        base += int(ng[g])
    return colidx, src


def _dense_inner(s, synth, got, vals):
    """The inner layer's dense weights (M, Cg', KH', KW') in float64 from the printed CSR and s2d_src alone."""
    _, _, ci_n, _, _, kh, kw = inner_dims(s, synth)
    mg, cgi = s.M // s.group, ci_n // s.group
    w = np.zeros((s.M, cgi * kh * kw), np.float64)
    base = 0
    for g in range(s.group):
        r = got["rowptr"][g * (mg + 1):(g + 1) * (mg + 1)]
        for m in range(mg):
            k = np.arange(r[m], r[m + 1]) + base
            w[g * mg + m, got["colidx"][k]] = np.asarray(vals, np.float64)[got["src"][k]]
        base += int(got["nnz_g"][g])
    return w.reshape(s.M, cgi, kh, kw)


def _case(pkg, synth, exe, tmp_path, s, w):
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
    plan.weight_align_cpu(w)
    rp, ci, vals, ng = plan.get_csr()
    plan.close()
    got = _run(exe, tmp_path, s, rp, ci, ng, relu=1)
    # the predicate: every strided float plan of these sizes; no double plan
    assert got["serves"].tolist() == [1]
    assert _run(exe, tmp_path, s, rp, ci, ng, f64=True)["serves"].tolist() == [0]
    ph_n, pw_n, ci_n, hi, wi, kh, kw = inner_dims(s, synth)
    oh, ow = synth.out_hw(s)
    assert got["phases"].tolist() == [ph_n, pw_n, s.N * ci_n * hi * wi]
    # N, has_bias, fuse_relu and group are the outer plan's; pad 0, stride 1, dilation 1
    assert got["inner"].tolist() == [s.N, ci_n, hi, wi, s.M, kh, kw, 0, 0, 1, 1, 1, 1, s.group, int(bool(s.bias)), 1]
    assert (hi - kh + 1, wi - kw + 1) == (oh, ow)
    colidx, src = _restate_csr(s, synth, rp, ci, ng)
    mg = s.M // s.group
    assert got.get("colidx", np.zeros(0)).tolist() == colidx and got.get("src", np.zeros(0)).tolist() == src
    assert sorted(src) == list(range(len(ci)))                              # a permutation of the outer entries ...
    assert got["nnz_g"].tolist() == [int(v) for v in ng]
    assert got["rowptr"].tolist() == [int(v) for v in rp]                   # ... inside each row
    for g in range(s.group):
        r = got["rowptr"][g * (mg + 1):(g + 1) * (mg + 1)]
        base = int(np.sum(ng[:g]))
        for m in range(mg):
            assert np.all(np.diff(got["colidx"][base + r[m]:base + r[m + 1]]) > 0)     # ascending inner columns
    if len(ci):
        assert int(max(colidx)) < (ci_n // s.group) * kh * kw
    # forward: the inner dense convolution of X' equals the outer layer's convolution
    wi64 = _dense_inner(s, synth, got, vals)
    x = synth.activations(s, 12).astype(np.float64)
    b = synth.bias_vector(s, 13)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float64))  # noqa: E731
    want = F.conv2d(t(x), t(w), t(b), stride=(s.stride_h, s.stride_w), padding=(s.pad_h, s.pad_w), groups=s.group).numpy()
    xi = pack(s, synth, x)
    assert xi.shape == (s.N, ci_n, hi, wi)
    inner = F.conv2d(t(xi), t(wi64), t(b), groups=s.group).numpy()
    scale = max(np.abs(want).max(), 1e-300)
    err = float(np.abs(inner - want).max() / scale)
    # data gradient: the inner layer's, through the unpack rule
    td = seeded((s.N, s.M, oh, ow), 21, np.float64)
    want_dx = torch_backward(x, w, None, s, td)[0]
    Xi = torch.tensor(xi, requires_grad=True)
    F.conv2d(Xi, t(wi64), None, groups=s.group).backward(t(td))
    dx = unpack(s, synth, Xi.grad.numpy())
    assert not np.isnan(dx).any()
    err_dx = float(np.abs(dx - want_dx).max() / max(np.abs(want_dx).max(), 1e-300))
    print(s.name, "inner conv from the tables vs torch float64: forward %.3g, data gradient %.3g" % (err, err_dx))
    assert err <= 1e-12 and err_dx <= 1e-12, s.name


def test_division_by_multiplication_and_lanes_per_row(exe):
    """The kernels' index arithmetic divides by launch constants through s2d_div: exact on [0, 2^31) for every divisor tried."""
    out = subprocess.run([exe, "--div"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = out.stdout.decode()
    assert out.returncode == 0 and text.startswith("div OK"), text
    assert int(text.split()[2]) > 1000000


@pytest.mark.parametrize("name", list(SHAPES))
def test_tables_equal_their_restatement_and_give_the_outer_layer(pkg, synth, exe, tmp_path, name):
    s = make(synth, name)
    _case(pkg, synth, exe, tmp_path, s, synth.pruned_weights(s, 11))


def test_random_geometries(pkg, synth, exe, tmp_path):
    for i, s in enumerate(random_shapes(synth)):
        _case(pkg, synth, exe, tmp_path, s, synth.pruned_weights(s, 100 + i))


def test_predicate_refuses_what_the_option_does_not_serve(pkg, synth, exe, tmp_path):
    """Stride 1 in both axes, a dilation, and the size limits (X' and the bottom at 2^31 elements, more than 32767 inner
    channels per group); an empty pattern is still served."""
    rp, ci, ng = np.array([0, 1]), np.array([0]), np.array([1])
    for name in UNSERVED:
        s = make(synth, name)
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
        plan.weight_align_cpu(synth.pruned_weights(s, 11))
        r, c, _, n = plan.get_csr()
        plan.close()
        assert _run(exe, tmp_path, s, r, c, n)["serves"].tolist() == [0], name
    s = synth.shape("huge_x", 1 << 19, 1, 64, 64, 1, 1, stride=2, sparsity=0.0)           # N*C*H*W = 2^31
    assert _run(exe, tmp_path, s, rp, ci, ng)["serves"].tolist() == [0]
    s = synth.shape("huge_xi", 1 << 25, 1, 2, 2, 1, 2, stride=2, pad=3, sparsity=0.0)      # N*C*H*W = 2^27, N*C'*H'*W' = 2^25 * 4 * 4 * 4 = 2^31
    assert _run(exe, tmp_path, s, rp, ci, ng)["serves"].tolist() == [0]
    s = synth.shape("fits_xi", (1 << 25) - 1, 1, 2, 2, 1, 2, stride=2, pad=3, sparsity=0.0)
    assert _run(exe, tmp_path, s, rp, ci, ng)["serves"].tolist() == [1]
    s = synth.shape("many_ch", 1, 9000, 4, 4, 1, 2, stride=2, sparsity=0.0)               # Cg' = 36000 > 32767
    assert _run(exe, tmp_path, s, rp, ci, ng)["serves"].tolist() == [0]
    s = synth.shape("just_fits", 1, 8191, 4, 4, 1, 2, stride=2, sparsity=0.0)             # Cg' = 32764
    assert _run(exe, tmp_path, s, rp, ci, ng)["serves"].tolist() == [1]
    s = synth.shape("empty", 2, 4, 5, 5, 3, 3, pad=1, stride=2, sparsity=0.0)
    got = _run(exe, tmp_path, s, np.zeros(4, np.int64), np.zeros(0, np.int64), np.array([0]))
    assert got["serves"].tolist() == [1] and got["nnz_g"].tolist() == [0] and np.all(got["rowptr"] == 0)
