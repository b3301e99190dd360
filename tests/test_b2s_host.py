"""Plan option "b2s" without a GPU: the option's values and refusals; through tests/cpp/b2s_plan_check.cpp, compiled with
plain g++ and no ROCm include path (that compile is the proof that the rule is host-only), align_rules.h b2s_plan -- the
serve predicate, the block, the inner descriptor and the scratch sizes -- against a numpy restatement written from
include/escoin.h alone, on named shapes and on 200 seeded random ones; the composition pack -> pointwise layer of
ceil(N / B) images -> unpack against the inner product, exactly, on integer-valued inputs; a CPU-aligned plan with the
option set against one without; the InnerProduct layers of a .caffemodel; and the shim's InnerProductLayer in CPU mode."""
import os
import subprocess

import numpy as np
import pytest

from b2s_common import MAX_INNER_IMAGES, SHAPES, ip_shape, make, pack, plan_row, rule_block, unpack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "caffe-escoin_amd", "caffe_shim", "shim_b2s_selftest")


def test_option_values_and_refusals(pkg, synth):
    s = make(synth, "ip_small")
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
    plan.set_option("b2s", 1)
    plan.set_option("b2s", 0)
    for bad in (2, -1):
        with pytest.raises(pkg.EscoinError) as e:
            plan.set_option("b2s", bad)
        assert "failed (-1)" in str(e.value) and "b2s" in str(e.value)      # ESCOIN_EINVAL
    for good in (0, 4, 8, 64, 100, 256):
        plan.set_option("b2s_block", good)
    for bad in (-4, 1, 2, 3, 6, 66, 257, 260, 512):
        with pytest.raises(pkg.EscoinError) as e:
            plan.set_option("b2s_block", bad)
        assert "failed (-1)" in str(e.value) and "b2s_block" in str(e.value)
    plan.set_option("b2s", 1)
    plan.set_option("s2d", 1)
    plan.set_option("s2b", 1)                                               # all three may be set
    for key in ("b2s", "b2s_block", "b2s_scratch_bytes"):
        assert plan.stat(key) == 0                                          # nothing is active before a device align
    plan.weight_align_cpu(synth.pruned_weights(s, 11))
    for key, v in (("b2s", 0), ("b2s", 1), ("b2s_block", 0), ("b2s_block", 64)):
        with pytest.raises(pkg.EscoinError) as e:
            plan.set_option(key, v)                                         # after the align
        assert "failed (-4)" in str(e.value) and "before" in str(e.value)   # ESCOIN_ESTATE
    for key in ("b2s", "b2s_block", "b2s_scratch_bytes"):
        assert plan.stat(key) == 0
    plan.close()
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s), b2s=1, b2s_block=8)         # the constructor passes options through
    plan.close()
    assert "escoin_plan_b2s_pack" in pkg.API_SYMBOLS and "escoin_plan_b2s_unpack" in pkg.API_SYMBOLS
    assert all(hasattr(pkg.lib(), n) for n in ("escoin_plan_b2s_pack", "escoin_plan_b2s_unpack"))
    assert hasattr(pkg.Plan, "b2s_pack") and hasattr(pkg.Plan, "b2s_unpack")


def test_inner_product_descriptor(pkg, synth):
    d = pkg.ConvDesc.inner_product(256, 9216, 4096)
    assert [getattr(d, f) for f, _ in d._fields_] == [256, 9216, 1, 1, 4096, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1, 0]
    d = pkg.ConvDesc.inner_product(3, 5, 7, bias=False, relu=True)
    assert (d.N, d.C, d.M, d.has_bias, d.fuse_relu) == (3, 5, 7, 0, 1)
    assert pkg.out_shape(d) == (1, 1)
    s = ip_shape(synth, "same", 3, 5, 7, bias=False)
    e = pkg.ConvDesc.from_shape(s, fuse_relu=True)
    assert all(getattr(d, f) == getattr(e, f) for f, _ in d._fields_)


def test_cpu_entry_points_ignore_the_option(pkg, synth):
    """weight_align_cpu + forward_cpu / backward_cpu with "b2s" = 1 give the bits of "b2s" = 0, float and double."""
    for name in ("ip_small", "ip_g2"):
        s = make(synth, name)
        w, x, b = synth.pruned_weights(s, 11), synth.activations(s, 12), synth.bias_vector(s, 13)
        td = synth.uniform(21, s.N * s.M).reshape(s.N, s.M, 1, 1)
        for dt in (np.float32, np.float64):
            got = []
            for b2s in (1, 0):
                plan = pkg.Plan(pkg.ConvDesc.from_shape(s), b2s=b2s)
                plan.weight_align_cpu(w.astype(dt))
                top = plan.forward_cpu(x.astype(dt), None if b is None else b.astype(dt), n_threads=2)
                bd, wd, bsd = plan.backward_cpu(td.astype(dt), bottom=x.astype(dt), bottom_diff=True, weight_diff=True,
                                                bias_diff=True if s.bias else None, n_threads=2)
                assert plan.stat("b2s") == 0
                got.append((top, bd, wd, bsd))
                plan.close()
            for a, c in zip(*got):
                assert (a is None and c is None) or (a.dtype == dt and a.tobytes() == c.tobytes()), (name, dt)
            assert np.abs(got[0][0]).max() > 0 and np.abs(got[0][2]).max() > 0


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """g++, -Icsrc -Iinclude, nothing of ROCm."""
    tmp = tmp_path_factory.mktemp("b2s")
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    out = str(tmp / "b2s_plan_check")
    srcs = [os.path.join(ROOT, "tests", "cpp", "b2s_plan_check.cpp")] + [
        os.path.join(csrc, f) for f in ("align_rules.cpp", "csr_tables.cpp", "stream_builder.cpp", "jit_codegen.cpp")]
    flags = ["g++", "-O1", "-std=c++17", "-Wall", "-I" + csrc, "-I" + os.path.join(ROOT, "include")]
    procs = [subprocess.Popen(flags + ["-c", s, "-o", str(tmp / (os.path.basename(s) + ".o"))]) for s in srcs]
    assert all(p.wait() == 0 for p in procs)
    subprocess.check_call(flags + ["-o", out] + [str(tmp / (os.path.basename(s) + ".o")) for s in srcs] + ["-lpthread"])
    return out


def _words(s, relu=1, f64=0, block=0, n_cu=256):
    return [s.N, s.C, s.H, s.W, s.M, s.KH, s.KW, s.pad_h, s.pad_w, s.stride_h, s.stride_w, s.dil_h, s.dil_w, s.group,
            int(bool(s.bias)), relu, int(f64), block, n_cu]


def _run(exe, tmp_path, cases):
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


def _random_shapes(synth, count, seed=20271):
    rs = np.random.RandomState(seed)
    out = []
    for i in range(count):
        g = int(rs.choice([1, 1, 2, 4]))
        N = int(rs.choice([rs.randint(1, 70), rs.randint(1, 600), rs.randint(1, 70000)]))
        K, M = g * int(rs.randint(1, 300)), g * int(rs.randint(1, 300))
        # (a stride and a dilation are immaterial with one pixel and one tap)
        out.append(synth.shape("rnd%d" % i, N, K, 1, 1, M, 1, stride=int(rs.randint(1, 4)), dil=int(rs.randint(1, 4)), group=g,
                               bias=bool(rs.randint(2)), sparsity=0.5))
    return out


def test_the_rule_equals_its_restatement_on_the_shapes_and_on_random_ones(synth, exe, tmp_path):
    named = [make(synth, n) for n in SHAPES] + [
        ip_shape(synth, "fc6", 256, 9216, 4096), ip_shape(synth, "fc8_b32", 32, 4096, 1000), ip_shape(synth, "ip2", 100, 500, 10),
        ip_shape(synth, "one", 1, 1, 1), ip_shape(synth, "n64", 64, 8, 8), ip_shape(synth, "n65", 65, 8, 8),
        ip_shape(synth, "n129", 129, 8, 8), ip_shape(synth, "n300", 300, 8, 8)]
    shapes = named + _random_shapes(synth, 200)
    cases, want = [], []
    rs = np.random.RandomState(5)
    for s in shapes:
        for block in (0, int(rs.choice([4, 8, 12, 64, 100, 128, 252, 256]))):
            for n_cu in (256, 64):                                          # the shipped rule does not weigh the CU count
                cases.append(_words(s, block=block, n_cu=n_cu))
                want.append(plan_row(s, block))
    got = _run(exe, tmp_path, cases)
    served = 0
    for c, w, row in zip(cases, want, got):
        assert row == w, c
        if row[0]:
            served += 1
            B, N = row[1], c[0]
            assert B % 4 == 0 and 4 <= B <= 256 and row[4] * B >= N and (row[4] - 1) * B < N
            assert row[13:17] == [1, 1, 1, 1] and row[19] == 0             # stride, dilation normalised; no inner ReLU
    assert served > 700
    # the rule itself, as the header states it
    assert [rule_block(n) for n in (1, 3, 4, 61, 64, 65, 128, 129, 192, 193, 256, 257, 300)] == \
        [64] * 13
    assert rule_block(65535 * 64 + 1) == 128 and rule_block(65535 * 256) == 256 and rule_block(65535 * 256 + 1) is None
    # no double plan
    assert all(r == [0] for r in _run(exe, tmp_path, [_words(s, f64=1) for s in named]))


def test_predicate_refuses_what_the_option_does_not_serve(synth, exe, tmp_path):
    """H * W > 1, a pad, a kernel above 1x1, a double plan; each blob's size limit at its edge; 65536 inner images."""
    sh = synth.shape
    cases = [
        (sh("hw2", 4, 8, 1, 2, 8, 1, sparsity=0.0), 0, 0),
        (sh("h2", 4, 8, 2, 1, 8, 1, sparsity=0.0), 0, 0),
        (sh("pad", 4, 8, 1, 1, 8, 1, pad=1, sparsity=0.0), 0, 0),
        (sh("pad_w", 4, 8, 1, 1, 8, 1, pad=0, pad_w=1, sparsity=0.0), 0, 0),
        (sh("k3", 4, 8, 1, 1, 8, 3, pad=1, sparsity=0.0), 0, 0),
        (sh("kw2", 4, 8, 1, 1, 8, 1, KW=2, pad_w=1, sparsity=0.0), 0, 0),
        (sh("strided", 4, 8, 1, 1, 8, 1, stride=2, dil=3, sparsity=0.0), 0, 1),
        # X' at 2^31: N' * C * B with N = 2^16 = 1024 blocks of 64, C = 2^15; the bottom N * C is the same here ...
        (sh("huge_x", 1 << 16, 1 << 15, 1, 1, 4, 1, group=4, sparsity=0.0), 0, 0),
        (sh("fits_x", (1 << 16) - 64, 1 << 15, 1, 1, 4, 1, group=4, sparsity=0.0), 0, 1),
        # ... and X' alone: N = 2^16 - 63 images still pad to 2^16 positions, the bottom is below 2^31
        (sh("huge_x_pad", (1 << 16) - 63, 1 << 15, 1, 1, 4, 1, group=4, sparsity=0.0), 0, 0),
        # T' at 2^31 with X' far below: M = 2^15
        (sh("huge_t", 1 << 16, 4, 1, 1, 1 << 15, 1, sparsity=0.0), 0, 0),
        (sh("fits_t", (1 << 16) - 64, 4, 1, 1, 1 << 15, 1, sparsity=0.0), 0, 1),
        (sh("huge_t_pad", (1 << 16) - 63, 4, 1, 1, 1 << 15, 1, sparsity=0.0), 0, 0),
        # the forced block pads more: N = 257 at B = 256 is 512 positions
        (sh("forced_pad_fits", 257, 1 << 22, 1, 1, 256, 1, group=256, sparsity=0.0), 64, 1),
        (sh("forced_pad_huge", 257, 1 << 22, 1, 1, 256, 1, group=256, sparsity=0.0), 256, 0),
        # inner images: 65535 fit, 65536 do not (a forced block of 4; under the rule a larger block takes over)
        (sh("most_images", 65535 * 4, 4, 1, 1, 4, 1, sparsity=0.0), 4, 1),
        (sh("many_images", 65535 * 4 + 1, 4, 1, 1, 4, 1, sparsity=0.0), 4, 0),
        (sh("many_images_rule", 65535 * 4 + 1, 4, 1, 1, 4, 1, sparsity=0.0), 0, 1),
        (sh("rule_256", 65535 * 256, 1, 1, 1, 1, 1, sparsity=0.0), 0, 1),
        (sh("rule_none", 65535 * 256 + 1, 1, 1, 1, 1, 1, sparsity=0.0), 0, 0),
    ]
    got = _run(exe, tmp_path, [_words(s, block=blk) for s, blk, _ in cases])
    for (s, blk, want), row in zip(cases, got):
        assert row[0] == want, s
        assert row == plan_row(s, blk), s
        if want:
            assert row[4] <= MAX_INNER_IMAGES and max(row[2], row[3]) < 2 ** 31
    assert all(r == [0] for r in _run(exe, tmp_path, [_words(make(synth, n), f64=1) for n in SHAPES]))


def test_the_plan_check_is_clean_under_the_host_sanitizers(synth, tmp_path):
    """b2s_plan_check as a stand-alone program with -fsanitize=address,undefined on the named and the edge cases."""
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    out = str(tmp_path / "b2s_plan_check_san")
    srcs = [os.path.join(ROOT, "tests", "cpp", "b2s_plan_check.cpp")] + [
        os.path.join(csrc, f) for f in ("align_rules.cpp", "csr_tables.cpp", "stream_builder.cpp", "jit_codegen.cpp")]
    rc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + csrc,
                         "-I" + os.path.join(ROOT, "include"), "-o", out] + srcs + ["-lpthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if rc.returncode != 0 and b"sanitize" in rc.stdout.lower() and (b"cannot find" in rc.stdout or b"unrecognized" in rc.stdout):
        pytest.fail("this toolchain has no sanitizer runtime: " + rc.stdout.decode()[-300:])
    assert rc.returncode == 0, rc.stdout.decode()
    shapes = [make(synth, n) for n in SHAPES] + [ip_shape(synth, "edge", 65535 * 256 + 1, 1, 1), ip_shape(synth, "x", 1 << 16, 1 << 15, 4, group=4)]
    rows = _run(out, tmp_path, [_words(s, block=b) for s in shapes for b in (0, 4, 256)])
    assert rows == [plan_row(s, b) for s in shapes for b in (0, 4, 256)]


# ---- the composition, exactly -----------------------------------------------------------------------------------------------------------
def _integers(s, synth, seed):
    rs = np.random.RandomState(seed)
    w = synth.pruned_weights(s, seed)
    w = np.where(w != 0, rs.randint(1, 4, w.shape) * rs.choice([-1, 1], w.shape), 0).astype(np.float32)
    x = rs.randint(-3, 4, (s.N, s.C)).astype(np.float32)
    b = rs.randint(-5, 6, (s.M,)).astype(np.float32) if s.bias else np.zeros(s.M, np.float32)
    td = rs.randint(-3, 4, (s.N, s.M)).astype(np.float32)
    return w, x, b, td


def _dense(s, w):
    """The M x C matrix of a grouped M x Cg blob (zero outside the groups' blocks)."""
    mg, cg = s.M // s.group, s.C // s.group
    full = np.zeros((s.M, s.C), np.float64)
    for g in range(s.group):
        full[g * mg:(g + 1) * mg, g * cg:(g + 1) * cg] = w.reshape(s.M, cg)[g * mg:(g + 1) * mg]
    return full


@pytest.mark.parametrize("name", list(SHAPES))
def test_pack_pointwise_layer_unpack_is_the_inner_product_exactly(synth, name):
    """Integer-valued inputs, so every order of summation is exact: for the rule's block and forced ones, and for partial
    batches, forward, data gradient, weight and bias gradient through the inner layout equal the inner product's."""
    s = make(synth, name)
    w, x, b, td = _integers(s, synth, 31)
    W = _dense(s, w)
    for relu in (False, True):
        for B in (rule_block(s.N), 4, 8, 64, 256):
            for n in sorted({s.N, s.N - 1, 1}):
                lin = x[:n].astype(np.float64) @ W.T + b
                want = np.where(lin > 0, lin, 0.0) if relu else lin
                g = np.where(want > 0, td[:n], 0.0) if relu else td[:n].astype(np.float64)
                xi = pack(x, B, n)                                          # N' x C x B
                assert xi.shape == (-(-n // B), s.C, B)
                ti = np.einsum("mc,ncj->nmj", W, xi.astype(np.float64)) + b[None, :, None]
                nan = np.full((s.N, s.M), np.nan, np.float32)
                top = unpack(ti.astype(np.float32), B, n, s.M, relu=relu, out=nan)
                assert np.array_equal(top[:n], want) and np.all(np.isnan(top[n:])), (name, B, n, relu)
                gi = pack(td, B, n, mask=top if relu else None)
                assert np.array_equal(unpack(gi, B, n, s.M, out=nan)[:n], g)
                dxi = np.einsum("mc,nmj->ncj", W, gi.astype(np.float64))
                dx = unpack(dxi.astype(np.float32), B, n, s.C, out=np.full((s.N, s.C), np.nan, np.float32))
                assert np.array_equal(dx[:n], g @ W) and np.all(np.isnan(dx[n:]))
                # the padding positions are zero in both operands: the sums over the inner pixels are the batch's
                assert np.array_equal(np.einsum("nmj,ncj->mc", gi.astype(np.float64), xi.astype(np.float64)), g.T @ x[:n].astype(np.float64))
                assert np.array_equal(gi.astype(np.float64).sum(axis=(0, 2)), g.sum(axis=0))


# ---- caffemodel.py -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cm(pkg):
    from caffe_escoin_amd import caffemodel
    return caffemodel


@pytest.mark.parametrize("v1", [False, True], ids=["LayerParameter", "V1LayerParameter"])
def test_caffemodel_finds_the_inner_product_layers(pkg, synth, cm, tmp_path, v1):
    """A file with a convolution, two InnerProduct layers (with and without bias) and another layer, written in the V2 form
    (BlobShape: num_output x K) and in the V1 form (the enum type, legacy 1 x 1 x num_output x K dims)."""
    conv = synth.lenet_conv2(N=2)[0]
    ip1, ip2 = ip_shape(synth, "ip1", 8, 800, 500, sparsity=0.92), ip_shape(synth, "ip2", 8, 500, 10, bias=False, sparsity=0.81)
    w1, w2 = (synth.pruned_weights(s, 40 + i).reshape(s.M, s.C) for i, s in enumerate((ip1, ip2)))
    b1 = synth.bias_vector(ip1, 50)
    layers = [
        cm.CaffeLayer("conv2", "Convolution", [synth.pruned_weights(conv, 3), synth.bias_vector(conv, 4)], cm.conv_param_of(conv)),
        cm.CaffeLayer("ip1", "InnerProduct", [w1, b1], ip_param=dict(num_output=500, bias_term=True)),
        cm.CaffeLayer("relu1", "ReLU", []),
        cm.CaffeLayer("ip2", "InnerProduct", [w2], ip_param=dict(num_output=10, bias_term=False)),
    ]
    path = str(tmp_path / "net.caffemodel")
    cm.write_caffemodel(path, "lenet_like", layers, v1=v1)
    name, got = cm.read_caffemodel(path)
    assert name == "lenet_like" and [l.name for l in got] == ["conv2", "ip1", "relu1", "ip2"]
    assert [l.is_inner_product for l in got] == [False, True, False, True]
    assert [l.is_convolution for l in got] == [True, False, False, False]
    assert got[1].type == (cm.V1_INNER_PRODUCT if v1 else "InnerProduct")
    assert got[1].blobs[0].shape == ((1, 1, 500, 800) if v1 else (500, 800))        # the blob as the file shapes it ...
    ips = cm.inner_product_weights(got)
    assert sorted(ips) == ["ip1", "ip2"] and sorted(cm.conv_weights(got)) == ["conv2"]
    for l, w, b, s in ((got[1], w1, b1, ip1), (got[3], w2, None, ip2)):
        assert (l.num_output, l.K) == (s.M, s.C) and l.ip_weight.shape == (s.M, s.C)  # ... and as num_output x K either way
        assert l.ip_weight.tobytes() == w.tobytes() and ips[l.name][0].tobytes() == w.tobytes()
        assert (l.ip_bias is None) == (b is None) and (b is None or l.ip_bias.tobytes() == b.tobytes())
        assert l.ip_param == dict(num_output=s.M, bias_term=b is not None, axis=1, transpose=False)
        d = pkg.ConvDesc(*l.ip_desc(8))
        e = pkg.ConvDesc.inner_product(8, s.C, s.M, bias=b is not None)
        assert all(getattr(d, f) == getattr(e, f) for f, _ in d._fields_)
        # the descriptor and the blob align as any layer's
        plan = pkg.Plan(d, b2s=1)
        plan.weight_align_cpu(l.ip_weight.reshape(s.M, s.C, 1, 1))
        assert plan.nnz() == int(np.count_nonzero(w))
        plan.close()
    with pytest.raises(ValueError):
        got[0].num_output                                                             # a convolution is no inner product


def test_caffemodel_refuses_a_transposed_inner_product(cm, tmp_path):
    w = np.arange(12, dtype=np.float32).reshape(4, 3)
    path = str(tmp_path / "t.caffemodel")
    cm.write_caffemodel(path, "t", [cm.CaffeLayer("ip", "InnerProduct", [w], ip_param=dict(num_output=3, bias_term=False, transpose=True, axis=2))])
    layer = cm.read_caffemodel(path)[1][0]
    assert layer.ip_param["transpose"] is True and layer.ip_param["axis"] == 2
    with pytest.raises(ValueError) as e:
        layer.ip_weight
    assert "transpose" in str(e.value)


# ---- the shim -------------------------------------------------------------------------------------------------------------------------------
def _shim(args):
    if not os.path.exists(SHIM):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "caffe-escoin_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "caffe-escoin_amd", "caffe_shim")], stdout=subprocess.DEVNULL)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")           # CPU mode must not need a device
    out = subprocess.run([SHIM] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, env=env)
    text = out.stdout.decode()
    print(text)
    return out.returncode, text


def test_shim_inner_product_layer_in_cpu_mode_float_and_double():
    rc, text = _shim(["--cpu-only"])
    assert rc == 0 and "all OK" in text, text
    for label in ("float CPU", "double CPU"):
        assert any(l.startswith(label + " b2s 1 ran -1") and l.rstrip().endswith("OK") for l in text.splitlines()), text


def test_shim_inner_product_layer_aborts_on_transpose():
    rc, text = _shim(["--transpose"])
    assert rc == -6, (rc, text)                                                       # SIGABRT
    assert "transpose = true is not supported" in text and "ip_t" in text and "accepted" not in text
