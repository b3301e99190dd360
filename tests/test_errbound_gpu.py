"""Forward and Backward on the MI355X, every output element against the float64 reference within errbound.py's derived
bound, on inputs whose rows, input channels and images differ in scale by up to 2^48 (errbound.skew) -- so that one
channel, one image and one bias are seen, which the suite's max-norm (conftest.rel_err) does not.  Plus two exact
metamorphic checks per kernel family and weights whose bit patterns have inline-constant encodings.

Every case asserts the kernel that ran.  The worst err / bound per kernel is printed (pytest -s; profiles/errbound.md)."""
import numpy as np
import pytest

import errbound as eb
from layout_cases import GK_VARIANT, N_CU, dense_variant
from test_body_variant_gpu import CASES as BODY_CASES
from upd_common import new_weights, values_at
from wgrad_common import csr_positions, make_shape, seeded

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

L3X3 = ("eb3x3", (5, 24, 9, 11, 20, 3), dict(pad=1, sparsity=0.9))
PW_A = ("ebpw_a", (9, 96, 7, 9, 33, 1), dict(sparsity=0.95))
PW_B = ("ebpw_b", (4, 60, 5, 5, 150, 1), dict(sparsity=0.95))
G5X5 = ("ebg5x5", (2, 16, 12, 10, 12, 5), dict(pad=2, group=2, sparsity=0.8))
STR2 = ("ebs2", (3, 8, 31, 31, 8, 3), dict(pad=1, stride=2, sparsity=0.6))
# dilation 2 x 3 on a padded frame of 17 x 22 (row classes of 9 and 8 rows, column classes of 8, 7 and 7 columns); under option
# "s2b" 18 inner images of 24 x 9 x 8 with a 7 x 6 top, which forced TILED and JIT accept (seq_common.LAYERS has the reasons)
DIL = ("ebdil", (3, 24, 13, 16, 20, 3), dict(pad=2, pad_w=3, dil=2, dil_w=3, sparsity=0.9))
GK = ("gk", (64, 1024, 7, 7, 512, 1), dict(sparsity=0.0))       # test_gpu_parity.py's stream-K layer


@pytest.fixture(scope="module")
def dev(pkg):
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        pytest.fail("no HIP device visible (these tests run on the MI355X)")
    return torch.device("cuda:0")


_LAYERS = {}
_REFS = {}


def _layer(synth, spec, seed=0):
    """(shape, skewed inputs, unskewed (w, x, b)) of a layer spec, made once."""
    name, dims, kw = spec
    if (name, seed) not in _LAYERS:
        s = synth.shape(name, *dims, **kw)
        k = sum(map(ord, name)) + 1000 * seed
        w, x, b = synth.pruned_weights(s, k), synth.activations(s, k + 1), synth.bias_vector(s, k + 2)
        _LAYERS[(name, seed)] = (s, eb.skew(s, w, x, b, k + 3), (w, x, b))
    return _LAYERS[(name, seed)]


def _ref(s, sk, bias, relu, f64=False):
    """The float64 forward and its bound for a skewed layer, computed once per (layer, bias, relu, dtype)."""
    key = (s.name, id(sk), bias, relu, f64)
    if key not in _REFS:
        if relu:        # forward_bound's own rule: ReLU is 1-Lipschitz, max(want, 0) keeps the bound
            want, B = _ref(s, sk, bias, False, f64)
            _REFS[key] = (np.maximum(want, 0.0), B)
        else:
            _REFS[key] = eb.forward_bound(s, sk.w, sk.x, sk.b if bias else None, f64=f64)
    return _REFS[key]


def _up(a, dev, dt=np.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)


def _expect(pkg, kernel, name):
    """The kernel under test is the one that ran."""
    want = {pkg.KERNEL_GENERIC: ("generic",), pkg.KERNEL_TILED: ("tiled",), pkg.KERNEL_JIT: ("jit",),
            pkg.KERNEL_DENSE: ("dense_mfma",), pkg.KERNEL_AUTO: ("generic", "tiled", "jit", "dense_mfma")}[kernel]
    assert any(t in name for t in want), (kernel, name)
    if kernel == pkg.KERNEL_DENSE:
        assert name == "escoin_dense_mfma_kernel", name


def _forward_cases(pkg, dev, s, sk, kernel, combos, partial=0, f64=False, check_name=None, worst=None, **opts):
    """One plan per ReLU setting of `combos` ((bias, relu) pairs), forwards with and without bias, every element within
    the bound; yields each plan after its forwards, for the caller's stat assertions.  `worst`: errbound.within's."""
    dt = np.float64 if f64 else np.float32
    xd, bd = _up(sk.x, dev, dt), _up(sk.b, dev, dt)
    for relu in sorted(set(r for _, r in combos)):
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu), kernel=kernel, **opts)
        plan.weight_align(sk.w.astype(dt))
        name = plan.kernel_name
        (check_name or (lambda n: _expect(pkg, kernel, n)))(name)
        for bias in sorted(set(b for b, r in combos if r == relu)):
            got = plan.forward(xd, bd if bias else None)
            torch.cuda.synchronize()
            want, B = _ref(s, sk, bias, relu, f64)
            r = eb.within(got.cpu().numpy(), want, B, name, sk.row_exp, what=(s.name, "bias", bias, "relu", relu, opts), worst=worst)
            print("errbound forward %-44s %-8s bias=%d relu=%d %s: %.3g" % (name, s.name, bias, relu, opts, r))
            if partial and bias:      # the first images of the plan's batch, into the head of a full top blob
                top = torch.full_like(got, -7.5)
                plan.forward(xd[:partial], bd, top[:partial])
                torch.cuda.synchronize()
                eb.within(top[:partial].cpu().numpy(), want[:partial], B[:partial], name, sk.row_exp, what=(s.name, "first images", partial, opts),
                          worst=worst)
                assert bool((top[partial:] == -7.5).all()), (name, "images past the call's were written")
        yield plan
        plan.close()


def _run_forward(*a, **kw):
    for _ in _forward_cases(*a, **kw):
        pass


ALL4 = [(False, False), (True, False), (False, True), (True, True)]
ON_OFF = [(False, False), (True, True)]


# ---- forward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tb", [0, 256])
@pytest.mark.parametrize("kn", ["GENERIC", "TILED", "JIT", "AUTO", "DENSE"])
def test_forward_3x3_every_kernel_bias_relu_and_a_partial_batch(pkg, synth, dev, kn, tb):
    s, sk, _ = _layer(synth, L3X3)
    _run_forward(pkg, dev, s, sk, getattr(pkg, "KERNEL_" + kn), ALL4, partial=2, tiling_batch=tb)


@pytest.mark.parametrize("spec", [PW_A, PW_B], ids=["9x96x7x9x33", "4x60x5x5x150"])
@pytest.mark.parametrize("kn", ["TILED", "JIT", "AUTO"])
def test_forward_pointwise_several_images_per_tile_and_one_quad_per_lane(pkg, synth, dev, kn, spec):
    s, sk, _ = _layer(synth, spec)
    for plan in _forward_cases(pkg, dev, s, sk, getattr(pkg, "KERNEL_" + kn), ON_OFF, partial=3, tiling_batch=256):
        info = plan.tiling_info
        print("    tiling: %s" % info)
        if spec is PW_B:        # 25 pixels per image: several images per tile; generated code: one quad per lane
            assert " nseg=1 " not in info and "nseg=" in info, info
            if "jit" in plan.kernel_name and torch.cuda.get_device_properties(0).multi_processor_count == 256:
                assert " tpl=1 " in info, info


@pytest.mark.parametrize("kn", ["GENERIC", "TILED", "JIT", "AUTO", "DENSE"])
def test_forward_grouped_5x5(pkg, synth, dev, kn):
    s, sk, _ = _layer(synth, G5X5)
    _run_forward(pkg, dev, s, sk, getattr(pkg, "KERNEL_" + kn), ON_OFF, tiling_batch=256)


@pytest.mark.parametrize("kn", ["GENERIC", "DENSE", "AUTO"])
def test_forward_stride_2(pkg, synth, dev, kn):
    s, sk, _ = _layer(synth, STR2)
    _run_forward(pkg, dev, s, sk, getattr(pkg, "KERNEL_" + kn), ON_OFF, partial=1)


S2B_PACK, S2B_UNPACK = "escoin_s2b_pack_kernel", "escoin_s2b_unpack_kernel"
DIL_RUNS = [("GENERIC", 0), ("DENSE", 0), ("AUTO", 0), ("GENERIC", 1), ("TILED", 1), ("JIT", 1), ("DENSE", 1), ("AUTO", 1)]


@pytest.mark.parametrize("kn,s2b", DIL_RUNS, ids=["%s%s" % (k, "-s2b" if o else "") for k, o in DIL_RUNS])
def test_forward_dilated_with_and_without_space_to_batch(pkg, synth, dev, kn, s2b):
    """The dilated layer on its own geometry (the generic and the dense kernel: no tiled kernel takes a dilation) and under
    option "s2b" with each kernel family as the inner plan's: pack, the inner forward of N * P images, unpack (the ReLU
    there).  The partial batch is one image: P of the 3 * P inner images."""
    s, sk, _ = _layer(synth, DIL)
    kernel = getattr(pkg, "KERNEL_" + kn)

    def check_name(name):
        parts = name.split(" + ")
        if s2b:     # pack + the inner plan's own name, which names the forced family + unpack
            assert len(parts) >= 3 and parts[0] == S2B_PACK and parts[-1] == S2B_UNPACK, name
            parts = parts[1:-1]
        assert not any("s2b" in p or "s2d" in p for p in parts), name
        _expect(pkg, kernel, " + ".join(parts))

    for plan in _forward_cases(pkg, dev, s, sk, kernel, ALL4, partial=s.N // 2, check_name=check_name, **(dict(s2b=1) if s2b else {})):
        assert plan.stat("s2b") == s2b and plan.stat("s2d") == 0, plan.kernel_name
        if s2b and kn != "AUTO":
            assert plan.stat("kernel_choice") == kernel, plan.kernel_name


def test_forward_dense_stream_k_fixup(pkg, synth, dev):
    """The dense MFMA kernel with K split across workgroups: the cut tiles' partial sums are added in a fix-up (the
    split-K add of the bound's + 4)."""
    s, sk, _ = _layer(synth, GK)
    for plan in _forward_cases(pkg, dev, s, sk, pkg.KERNEL_DENSE, [(True, True)]):
        assert plan.stat("streamk") == 1 and plan.stat("streamk_gave_up") == 0
        # 128-row tiles, gathered operand and scalar stores (49 pixels), K split: the variant launch_dense's rule gives
        n_cu = torch.cuda.get_device_properties(0).multi_processor_count
        assert plan.stat("dense_variant") == dense_variant(s, s.N, n_cu) and (n_cu != N_CU or plan.stat("dense_variant") == GK_VARIANT)
        print("    dense_variant %d" % plan.stat("dense_variant"))


def test_forward_lowered_sparse(pkg, synth, dev):
    s, sk, _ = _layer(synth, L3X3)
    _run_forward(pkg, dev, s, sk, pkg.KERNEL_AUTO, ON_OFF, conv_mode=pkg.CONV_MODE_LOWERED_SPARSE,
                 check_name=lambda n: n == "escoin_csrmm_kernel" or pytest.fail(n))


def test_forward_chained_body(pkg, synth, dev):
    """The chained case of test_body_variant_gpu.CASES with the smallest bottom blob (seg7_5: 7 x 7 images, OW % 4 = 3,
    a partial second tile) on the chained body."""
    name, dims, expect, variant, options = min((c for c in BODY_CASES if c[3] == 1),
                                               key=lambda c: c[1][0] * c[1][1] * c[1][2] * c[1][3])
    N, C, H, W, M, K, pad, sp = dims
    s, sk, _ = _layer(synth, ("chain_" + name, (N, C, H, W, M, K), dict(pad=pad, sparsity=sp)))
    for plan in _forward_cases(pkg, dev, s, sk, pkg.KERNEL_AUTO, ON_OFF, tiling_batch=256, check_name=lambda n: "jit" in n or pytest.fail(n),
                               **options):
        assert plan.stat("body_variant") == variant, plan.tiling_info


@pytest.mark.parametrize("spec", [L3X3, STR2], ids=["3x3", "stride2"])
def test_forward_double_plan(pkg, synth, dev, spec):
    s, sk, _ = _layer(synth, spec)
    for plan in _forward_cases(pkg, dev, s, sk, pkg.KERNEL_AUTO, ON_OFF, f64=True, check_name=lambda n: "f64" in n or pytest.fail(n)):
        assert plan.stat("is_f64") == 1


# ---- exact metamorphic checks: no reference, no tolerance ---------------------------------------------------------------
FAMILIES = [
    ("generic", L3X3, "KERNEL_GENERIC", {}, False), ("tiled", L3X3, "KERNEL_TILED", {}, False),
    ("tiled_tb256", L3X3, "KERNEL_TILED", dict(tiling_batch=256), False),
    ("jit", L3X3, "KERNEL_JIT", {}, False), ("jit_tb256", L3X3, "KERNEL_JIT", dict(tiling_batch=256), False),
    ("dense", L3X3, "KERNEL_DENSE", {}, False),
    ("lowered_sparse", L3X3, "KERNEL_AUTO", dict(conv_mode="CONV_MODE_LOWERED_SPARSE"), False), ("double", L3X3, "KERNEL_AUTO", {}, True),
    ("jit_pointwise", PW_A, "KERNEL_JIT", dict(tiling_batch=256), False),
    ("tiled_pointwise", PW_B, "KERNEL_TILED", dict(tiling_batch=256), False),
    ("jit_5x5_groups", G5X5, "KERNEL_JIT", dict(tiling_batch=256), False),
    ("generic_stride2", STR2, "KERNEL_GENERIC", {}, False), ("dense_stride2", STR2, "KERNEL_DENSE", {}, False),
    # the options that run a layer through an inner plan: pack and unpack copy values, so the property holds through them
    ("s2d_stride2", STR2, "KERNEL_AUTO", dict(s2d=1), False),
    ("s2b_dilated", DIL, "KERNEL_AUTO", dict(s2b=1), False), ("s2b_jit_dilated", DIL, "KERNEL_JIT", dict(s2b=1), False),
    ("generic_dilated", DIL, "KERNEL_GENERIC", {}, False), ("dense_dilated", DIL, "KERNEL_DENSE", {}, False),
]


@pytest.mark.parametrize("fam,spec,kn,opts,f64", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_row_and_image_scaling_are_exact_on_every_kernel_family(pkg, synth, dev, fam, spec, kn, opts, f64):
    """No kernel's summation order depends on the values: rows (and bias) scaled by 2^e_m scale the output by 2^e_m bit
    for bit, and without a bias an image scaled by 2^g_n scales its output by 2^g_n."""
    s, sk, (w, x, b) = _layer(synth, spec)
    dt = np.float64 if f64 else np.float32
    opts = {k: getattr(pkg, v) if isinstance(v, str) else v for k, v in opts.items()}
    rows = _up(np.ldexp(1.0, sk.row_exp), dev, dt)[None, :, None, None]
    imgs = _up(np.ldexp(1.0, sk.img_exp), dev, dt)[:, None, None, None]
    xd = _up(x, dev, dt)
    outs, names = {}, []
    for key, ww, bb in (("plain", w, b), ("rows", sk.w, sk.b)):
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s), kernel=getattr(pkg, kn), **opts)
        plan.weight_align(ww.astype(dt))
        names.append((plan.kernel_name, plan.tiling_info))
        for option in ("s2d", "s2b"):       # the option is active on its rows, and on no other
            assert plan.stat(option) == opts.get(option, 0) and (("escoin_%s_pack_kernel" % option) in names[-1][0]) == (option in opts), \
                (fam, option, names[-1])
        outs[key] = plan.forward(xd, _up(bb, dev, dt)).clone()
        if key == "plain":
            outs["nobias"] = plan.forward(xd, None).clone()
            outs["images"] = plan.forward((xd * imgs).contiguous(), None).clone()
        torch.cuda.synchronize()
        plan.close()
    assert names[0] == names[1], names
    if kn != "KERNEL_AUTO":
        _expect(pkg, getattr(pkg, kn), names[0][0])
    assert ("f64" in names[0][0]) == f64 and (names[0][0] == "escoin_csrmm_kernel") == ("conv_mode" in opts), names
    bad = (outs["plain"] * rows != outs["rows"]).nonzero()
    assert bad.numel() == 0, (fam, names[0], "rows", bad[0].tolist(), int(sk.row_exp[int(bad[0][1])]))
    bad = (outs["nobias"] * imgs != outs["images"]).nonzero()
    assert bad.numel() == 0, (fam, names[0], "images", bad[0].tolist(), int(sk.img_exp[int(bad[0][0])]))
    assert bool(torch.isfinite(outs["rows"]).all()) and float(outs["rows"].abs().max()) > 0


# ---- weights whose bit patterns have inline-constant encodings -------------------------------------------------------------
INV_2PI = np.array([0x3E22F983], np.uint32).view(np.float32)[0]
SPECIALS = np.array([1.0, -1.0, 0.5, -0.5, 2.0, 4.0, INV_2PI, 1.0, -0.5, 2.0, INV_2PI, 4.0], np.float32)


@pytest.mark.parametrize("spec", [L3X3, PW_A], ids=["3x3", "pointwise"])
@pytest.mark.parametrize("kn", ["JIT", "TILED"])
def test_weights_with_inline_constant_bit_patterns(pkg, synth, dev, kn, spec):
    """+-1.0, +-0.5, 2.0, 4.0 and 1 / 2 pi can be encoded as inline constants of an instruction; the generated code must
    carry the full literal for each (jit_codegen.cpp).  A dozen nonzeros take these values, then set_values() writes
    ordinary values over them in place, then the special ones again."""
    s, sk, _ = _layer(synth, spec)
    rs = np.random.RandomState(5)
    w_special = sk.w.copy()
    nz = np.flatnonzero(w_special.ravel())
    w_special.ravel()[rs.choice(nz, SPECIALS.size, replace=False)] = SPECIALS
    w_plain = (new_weights(w_special, 17, zeros=False)[0] * np.ldexp(1.0, sk.row_exp).astype(np.float32)[:, None, None, None])
    xd, bd = _up(sk.x, dev), _up(sk.b, dev)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=True), kernel=getattr(pkg, "KERNEL_" + kn), tiling_batch=256)
    plan.weight_align(w_special)
    _expect(pkg, getattr(pkg, "KERNEL_" + kn), plan.kernel_name)
    for step, ww in enumerate((w_special, w_plain, w_special)):
        if step:
            plan.set_values(_up(values_at(plan, ww)[2], dev))
            assert plan.stat("update_fast") == 1, (kn, step)
        got = plan.forward(xd, bd)
        torch.cuda.synchronize()
        want, B = eb.forward_bound(s, ww, sk.x, sk.b, relu=True)
        r = eb.within(got.cpu().numpy(), want, B, plan.kernel_name, sk.row_exp, what=(s.name, "special weights, step", step))
        print("errbound special %-44s %-8s step %d: %.3g" % (plan.kernel_name, s.name, step, r))
    plan.close()


# ---- Backward -----------------------------------------------------------------------------------------------------------------
def _transposable(s):
    return (s.stride_h == 1 and s.stride_w == 1 and s.pad_h <= s.dil_h * (s.KH - 1) and s.pad_w <= s.dil_w * (s.KW - 1))


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("name", ["straddle3x3", "small7x7g2", "pointwise", "stride2"])
def test_backward_every_data_and_weight_gradient_kernel(pkg, synth, dev, name, relu):
    """The data gradient under every backward_kernel the geometry admits, the weight and bias gradient under wgrad_kernel
    entry and staged (staged: stride 1 only) in dense and compact form; every element within its bound."""
    s = make_shape(synth, name)
    w, x, b = synth.pruned_weights(s, 91), synth.activations(s, 92), synth.bias_vector(s, 93)
    td = seeded((s.N, s.M) + synth.out_hw(s), 94)
    sk = eb.skew(s, w, x, b, 95, top_diff=td)
    xd, bd_, tdd = _up(sk.x, dev), _up(sk.b, dev), _up(sk.top_diff, dev)
    desc = pkg.ConvDesc.from_shape(s, fuse_relu=relu)
    top_np = topd = None
    if relu:        # one top for every plan of the case: one mask, one reference
        plan = pkg.Plan(desc, kernel=pkg.KERNEL_GENERIC)
        plan.weight_align(sk.w)
        topd = plan.forward(xd, bd_)
        torch.cuda.synchronize()
        top_np = topd.cpu().numpy()
        plan.close()
    want, Bs = eb.backward_bound(s, sk.w, sk.x, sk.b, sk.top_diff, top_np)
    data = ["AUTO", "GENERIC"] + (["TILED", "JIT", "DENSE"] if _transposable(s) else [])
    runs = [(kn, "AUTO", True) for kn in data]
    runs += [("GENERIC", wk, False) for wk in ["ENTRY"] + (["STAGED"] if s.stride_h == 1 == s.stride_w else [])]
    for kn, wk, want_bd in runs:
        plan = pkg.Plan(desc, backward_kernel=getattr(pkg, "KERNEL_" + kn), wgrad_kernel=getattr(pkg, "WGRAD_" + wk))
        plan.weight_align(sk.w)
        bdiff, wd, bsd = plan.backward(tdd, bottom=xd, top=topd, bottom_diff=True if want_bd else None, weight_diff=True,
                                       bias_diff=True)
        torch.cuda.synchronize()
        ran_k, ran_w = plan.stat("bwd_data_kernel"), plan.stat("wgrad_kernel")
        what = (name, "relu", relu, kn, wk)
        if want_bd:
            if kn != "AUTO":
                assert ran_k == (getattr(pkg, "KERNEL_" + kn) if _transposable(s) else pkg.KERNEL_GENERIC), what
            r = eb.within(bdiff.cpu().numpy(), want[0], Bs[0], "bwd_data_kernel %d" % ran_k, sk.chan_exp, what=what)
            print("errbound backward data   kernel %d (%s) %-12s relu=%d: %.3g" % (ran_k, kn, name, relu, r))
        if wk != "AUTO":
            assert ran_w == getattr(pkg, "WGRAD_" + wk), what
        wdn = wd.cpu().numpy()
        r = eb.within(wdn, want[1], Bs[1], "wgrad_kernel %d" % ran_w, sk.td_row_exp, axis=0, what=what)
        rb = eb.within(bsd.cpu().numpy(), want[2], Bs[2], "wgrad_kernel %d bias" % ran_w, sk.td_row_exp, axis=0, what=what)
        assert np.all(wdn[sk.w == 0] == 0), what
        print("errbound backward weight kernel %d (%s) %-12s relu=%d: %.3g, bias %.3g" % (ran_w, wk, name, relu, r, rb))
        if not want_bd:
            _, vd, bsd2 = plan.backward(tdd, bottom=xd, top=topd, bottom_diff=None, values_diff=True, bias_diff=True)
            torch.cuda.synchronize()
            pos = csr_positions(plan)
            rv = eb.within(vd.cpu().numpy(), want[1].reshape(-1)[pos], Bs[1].reshape(-1)[pos], "wgrad_kernel %d compact" % ran_w, what=what)
            eb.within(bsd2.cpu().numpy(), want[2], Bs[2], "wgrad_kernel %d compact bias" % ran_w, sk.td_row_exp, axis=0, what=what)
            print("errbound backward values kernel %d (%s) %-12s relu=%d: %.3g" % (ran_w, wk, name, relu, rv))
        plan.close()
