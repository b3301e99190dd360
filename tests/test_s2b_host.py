"""Plan option "s2b" without a GPU: the option's values and refusals; through tests/cpp/s2b_plan_check.cpp, compiled with
plain g++ and no ROCm include path (that compile is the proof that the rule is host-only), align_rules.h s2b_plan -- the
serve predicate, the residue classes, the inner descriptor and the scratch sizes -- against a numpy restatement on every
shape of test_s2b_gpu.py and on 200 seeded random geometries; and the composition itself, exactly: on small integer-valued
weights, bottoms and top_diffs, where float arithmetic is exact, pack -> undilated convolution of N * P images -> unpack
equals the dilated convolution, element for element, forward and data gradient, with and without ReLU.  That pins the
mapping of include/escoin.h "Space-to-batch" before any GPU runs it."""
import os
import subprocess

import numpy as np
import pytest

from s2b_common import SHAPES, UNSERVED, inner_dims, make, pack, random_shapes, unpack

torch = pytest.importorskip("torch")
F = torch.nn.functional
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_INNER_IMAGES = 65535      # align_rules.h kS2bMaxInnerImages: the image index is a grid dimension of the inner kernels


def test_option_values_and_refusals(pkg, synth):
    s = make(synth, "3x3_d2")
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
    plan.set_option("s2b", 1)
    plan.set_option("s2b", 0)
    for bad in (2, -1):
        with pytest.raises(pkg.EscoinError) as e:
            plan.set_option("s2b", bad)
        assert "failed (-1)" in str(e.value) and "s2b" in str(e.value)      # ESCOIN_EINVAL
    plan.set_option("s2b", 1)
    plan.set_option("s2d", 1)                                               # both may be set: they serve disjoint geometries
    assert plan.stat("s2b") == 0 and plan.stat("s2b_scratch_bytes") == 0   # nothing is active before a device align
    plan.weight_align_cpu(synth.pruned_weights(s, 11))
    for v in (0, 1):
        with pytest.raises(pkg.EscoinError) as e:
            plan.set_option("s2b", v)                                       # after the align
        assert "failed (-4)" in str(e.value) and "before" in str(e.value)   # ESCOIN_ESTATE
    plan.close()
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s), s2b=1)                      # the constructor passes options through
    plan.close()
    assert "escoin_plan_s2b_pack" in pkg.API_SYMBOLS and "escoin_plan_s2b_unpack" in pkg.API_SYMBOLS
    assert hasattr(pkg.Plan, "s2b_pack") and hasattr(pkg.Plan, "s2b_unpack")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """g++, -Icsrc -Iinclude, nothing of ROCm."""
    tmp = tmp_path_factory.mktemp("s2b")
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    out = str(tmp / "s2b_plan_check")
    srcs = [os.path.join(ROOT, "tests", "cpp", "s2b_plan_check.cpp")] + [
        os.path.join(csrc, f) for f in ("align_rules.cpp", "csr_tables.cpp", "stream_builder.cpp", "jit_codegen.cpp")]
    flags = ["g++", "-O1", "-std=c++17", "-Wall", "-I" + csrc, "-I" + os.path.join(ROOT, "include")]
    procs = [subprocess.Popen(flags + ["-c", s, "-o", str(tmp / (os.path.basename(s) + ".o"))]) for s in srcs]
    assert all(p.wait() == 0 for p in procs)
    subprocess.check_call(flags + ["-o", out] + [str(tmp / (os.path.basename(s) + ".o")) for s in srcs] + ["-lpthread"])
    return out


def _words(s, relu=1, f64=0):
    return [s.N, s.C, s.H, s.W, s.M, s.KH, s.KW, s.pad_h, s.pad_w, s.stride_h, s.stride_w, s.dil_h, s.dil_w, s.group,
            int(bool(s.bias)), relu, int(f64)]


def _run(exe, tmp_path, cases):
    """One line of the program's output per case (a list of 17 ints), as ints."""
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        for c in cases:
            f.write(" ".join(str(int(v)) for v in c) + "\n")
    out = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    text = out.stdout.decode()
    assert out.returncode == 0, text
    rows = [[int(v) for v in line.split()] for line in text.splitlines()]
    assert len(rows) == len(cases), text
    return rows


def _restate(s, synth):
    """s2b_plan's output line for a served shape, from include/escoin.h alone."""
    eh, ew, P, hi, wi, ohi, owi = inner_dims(s, synth)
    x_floats, t_floats = s.N * P * s.C * hi * wi, s.N * P * s.M * ohi * owi
    return [1, eh, ew, x_floats, t_floats,
            s.N * P, s.C, hi, wi, s.M, s.KH, s.KW, 0, 0, 1, 1, 1, 1, s.group, int(bool(s.bias)), 0]


def test_the_rule_equals_its_restatement_on_the_shapes_and_on_random_geometries(synth, exe, tmp_path):
    shapes = [make(synth, n) for n in SHAPES] + random_shapes(synth, count=200)
    assert len(shapes) == len(SHAPES) + 200
    got = _run(exe, tmp_path, [_words(s) for s in shapes])
    for s, row in zip(shapes, got):
        assert row == _restate(s, synth), s
    # the named shapes are what their table says
    assert inner_dims(make(synth, "3x3_d2x3_g2"), synth)[:5] == (2, 3, 6, 8, 4)        # Hp = 15: classes of 8 and 7 rows
    assert inner_dims(make(synth, "d_gt_out"), synth)[:3] == (3, 2, 6) and synth.out_hw(make(synth, "d_gt_out"))[0] == 1
    assert inner_dims(make(synth, "one_tap_axis"), synth)[:3] == (1, 2, 2)
    assert inner_dims(make(synth, "d12_small"), synth)[2:5] == (144, 4, 4)
    # no double plan
    assert all(r == [0] for r in _run(exe, tmp_path, [_words(s, f64=1) for s in shapes[:len(SHAPES)]]))


def test_predicate_refuses_what_the_option_does_not_serve(synth, exe, tmp_path):
    """A stride, P == 1 (dilation 1; a 1x1 kernel; a dilation on one-tap axes only), a double plan, and the size limits:
    each of the four blobs at 2^31 elements, and N * P past the inner kernels' image limit."""
    sh = synth.shape
    cases = [(make(synth, n), 0) for n in UNSERVED]
    cases += [
        (sh("row_dilated_column_kernel", 2, 4, 9, 9, 4, 3, KW=1, dil=1, dil_w=3, sparsity=0.0), 0),  # KW = 1: ew = 1, and dil_h = 1
        (sh("one_axis", 2, 4, 9, 9, 4, 3, KW=1, dil=2, dil_w=3, sparsity=0.0), 1),                   # eh = 2 alone serves
        (sh("stride_w", 1, 4, 9, 9, 4, 3, stride_w=2, dil=2, pad=2, sparsity=0.0), 0),
        # the bottom at 2^31: N*C*H*W = 2^12 * 2^9 * 32 * 32, 1x3 kernel dilated by 2 (P = 2)
        (sh("huge_bottom", 1 << 12, 1 << 9, 32, 32, 1, 1, KW=3, dil=2, sparsity=0.0), 0),
        # X' at 2^31 with the bottom below: pad 16 makes the padded frame 4 x the image
        (sh("huge_x", 1 << 11, 1 << 8, 32, 32, 1, 3, dil=2, pad=16, sparsity=0.0), 0),
        (sh("fits_x", (1 << 11) - 1, 1 << 8, 32, 32, 1, 3, dil=2, pad=16, sparsity=0.0), 1),
        # the top (and T') at 2^31 with the bottom and X' far below: M = 2^13, C = 1
        (sh("huge_top", 1 << 8, 1, 34, 34, 1 << 13, 2, dil=2, sparsity=0.0), 0),
        (sh("fits_top", (1 << 8) - 1, 1, 34, 34, 1 << 13, 2, dil=2, sparsity=0.0), 1),
        # T' alone at 2^31: OH = 1 < eh = 16 rounds each class up to one row: T' = N * 256 * M, the top N * M * 1 * 1
        (sh("huge_t", 1 << 7, 1, 17, 17, 1 << 16, 2, dil=16, sparsity=0.0), 0),
        (sh("fits_t", (1 << 7) - 1, 1, 17, 17, 1 << 16, 2, dil=16, sparsity=0.0), 1),
        # N * P past the image limit: 16384 * 4 = 65536
        (sh("many_images", 16384, 1, 5, 5, 1, 2, dil=2, sparsity=0.0), 0),
        (sh("most_images", 16383, 1, 5, 5, 1, 2, dil=2, sparsity=0.0), 1),
        (sh("d256", 1, 1, 300, 300, 1, 2, dil=256, sparsity=0.0), 0),               # P = 65536
        (sh("d255", 1, 1, 300, 300, 1, 2, dil=255, sparsity=0.0), 1),               # P = 65025
    ]
    got = _run(exe, tmp_path, [_words(s) for s, _ in cases])
    for (s, want), row in zip(cases, got):
        assert row[0] == want, s
        if want:
            assert row == _restate(s, synth), s
            assert row[5] <= MAX_INNER_IMAGES and max(row[3], row[4]) < 2 ** 31


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float64))


def _integers(s, synth, seed):
    """Integer-valued float32 weights (the shape's pattern), bias, bottom and top_diff: every product and partial sum of the
    layer is an integer far below 2^24, so float32 and float64 arithmetic are both exact in any order."""
    rs = np.random.RandomState(seed)
    w = synth.pruned_weights(s, seed)
    w = np.where(w != 0, rs.randint(1, 4, w.shape) * rs.choice([-1, 1], w.shape), 0).astype(np.float32)
    x = rs.randint(-3, 4, (s.N, s.C, s.H, s.W)).astype(np.float32)
    b = rs.randint(-5, 6, (s.M,)).astype(np.float32) if s.bias else None
    td = rs.randint(-3, 4, (s.N, s.M) + tuple(synth.out_hw(s))).astype(np.float32)
    return w, x, b, td


def _composition(s, synth, seed):
    w, x, b, td = _integers(s, synth, seed)
    eh, ew, P, hi, wi, ohi, owi = inner_dims(s, synth)
    oh, ow = synth.out_hw(s)
    X = torch.tensor(x.astype(np.float64), requires_grad=True)
    lin = F.conv2d(X, _t(w), _t(b), padding=(s.pad_h, s.pad_w), dilation=(s.dil_h, s.dil_w), groups=s.group)
    for relu in (False, True):
        # (the library's mask is [top > 0]: integer tops hit 0 exactly, where clamp's gradient would be 1)
        want = torch.where(lin > 0, lin, torch.zeros_like(lin)) if relu else lin
        X.grad = None
        want.backward(_t(td), retain_graph=True)
        want_np, want_dx = want.detach().numpy(), X.grad.numpy().copy()
        # forward: pack -> the undilated convolution of N * P images (no pad, no ReLU) -> unpack -> ReLU
        xi = pack(x, eh, ew, s.pad_h, s.pad_w, hi, wi)
        assert xi.shape == (s.N * P, s.C, hi, wi) and xi.dtype == np.float32
        Xi = torch.tensor(xi.astype(np.float64), requires_grad=True)
        ti = F.conv2d(Xi, _t(w), _t(b), groups=s.group)
        assert tuple(ti.shape) == (s.N * P, s.M, ohi, owi)
        top = unpack(ti.detach().numpy(), eh, ew, 0, 0, oh, ow)
        if relu:
            top = np.where(top > 0, top, 0.0)
        assert not np.isnan(top).any() and np.array_equal(top, want_np), (s.name, relu)
        assert np.array_equal(top.astype(np.float32).astype(np.float64), top)            # exact in float32 too
        # data gradient: pack of top_diff (times [top > 0]) -> the inner data gradient -> unpack at the pad
        g = np.where(top > 0, td, 0.0) if relu else td.astype(np.float64)
        gi = pack(g, eh, ew, 0, 0, ohi, owi)
        ti.backward(_t(gi))
        dx = unpack(Xi.grad.numpy(), eh, ew, s.pad_h, s.pad_w, s.H, s.W)
        assert not np.isnan(dx).any() and np.array_equal(dx, want_dx), (s.name, relu)
    return want_np, want_dx


@pytest.mark.parametrize("name", list(SHAPES))
def test_pack_inner_convolution_unpack_is_the_dilated_convolution_exactly(synth, name):
    s = make(synth, name)
    top, dx = _composition(s, synth, 31)
    assert np.abs(top).max() > 0 and np.abs(dx).max() > 0
    if name == "d_gt_out":
        # OH = 1 < eh = 3 on a 7-row image without pad: windows read rows 0, 3 and 6 only
        assert not dx[:, :, [1, 2, 4, 5], :].any()


def test_the_composition_on_random_geometries(synth):
    for i, s in enumerate(random_shapes(synth, count=40)):
        _composition(s, synth, 200 + i)
