"""Plan option "b2s" on the MI355X: inner-product layers through escoin_b2s_pack_kernel, a pointwise inner plan of
ceil(N / B) images of 1 x B and escoin_b2s_unpack_kernel.  The two transposes alone against numpy, exactly; forward and the
whole backward against float64 and the per-element bound of errbound.py on skewed inputs, for every inner kernel; the bit
equalities the header states (the generic kernel against the plan without the option; sparse kernels across blocks and
n_images); non-finite containment; updates, prune, rewire, export / import and a conv_mode flip against fresh plans; a
captured training step; the layers the option does not serve; the bench tool."""
import ctypes

import numpy as np
import pytest

import errbound as eb
from b2s_common import SHAPES, TILE, ip_shape, make, pack, rule_block, unpack
from upd_common import new_weights, same_bits, values_at

torch = pytest.importorskip("torch")

from wgrad_common import seeded  # noqa: E402

pytestmark = pytest.mark.gpu
PACK = "escoin_b2s_pack_kernel + "
UNPACK = " + escoin_b2s_unpack_kernel"
KERNELS = ["AUTO", "GENERIC", "TILED", "JIT", "DENSE"]


@pytest.fixture(scope="module")
def dev(pkg):
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        pytest.fail("no HIP device visible (these tests run on the MI355X)")
    return torch.device("cuda:0")


_CASES, _BOUNDS = {}, {}


def _case(synth, s, w_seed=11):
    """(shape, skewed inputs) of a shape: made once, never written."""
    if s.name not in _CASES:
        w = synth.pruned_weights(s, w_seed)
        x, b = synth.activations(s, 12), synth.bias_vector(s, 13)
        td = seeded((s.N, s.M, 1, 1), 21)
        _CASES[s.name] = (s, eb.skew(s, w, x, b, 95, top_diff=td))
    return _CASES[s.name]


def _fwd_bound(s, sk, relu, bias=True):
    key = (s.name, relu, bias)
    if key not in _BOUNDS:
        _BOUNDS[key] = eb.forward_bound(s, sk.w, sk.x, sk.b if bias else None, relu=relu)
    return _BOUNDS[key]


def _up(a, dev, dt=np.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)


def _k(pkg, name):
    return getattr(pkg, "KERNEL_" + name)


def _plan(pkg, s, w, relu=False, b2s=1, **opts):
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu), b2s=b2s, **opts)
    plan.weight_align(w)
    return plan


def _active(pkg, plan, s, block=None):
    """The option is active: the stats, the names and the accounting of the scratches."""
    B = block or rule_block(s.N)
    np_ = -(-s.N // B)
    assert plan.stat("b2s") == 1 and plan.stat("b2s_block") == B and plan.stat("s2d") == 0 and plan.stat("s2b") == 0
    assert plan.stat("b2s_scratch_bytes") == 4 * np_ * B * (2 * s.C + s.M)          # X', dX' and T' / G'
    name = plan.kernel_name
    assert name.startswith(PACK) and name.endswith(UNPACK) and len(name) > len(PACK) + len(UNPACK)
    assert "escoin_b2s" not in name[len(PACK):-len(UNPACK)]                         # the inner plan's own name in between
    assert plan.stat("device_bytes") > plan.stat("b2s_scratch_bytes")
    assert plan.workspace_bytes == (plan.stat("device_bytes") + plan.stat("bwd_device_bytes") + plan.stat("upd_device_bytes") +
                                    plan.stat("dwg_device_bytes"))


def _nan(shape, dev):
    return torch.full(shape, float("nan"), device=dev)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. the kernels alone, exactly -------------------------------------------------------------------------------------------
def _special(shape, seed):
    """Values with NaN, infinities, -0.0 and subnormals sprinkled in: the transposes are copies, bit for bit."""
    a = seeded(shape, seed)
    flat = a.reshape(-1)
    sp = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-45, -1e-45, 1e-39], np.float32)
    idx = np.random.RandomState(seed).choice(flat.size, size=min(flat.size, 2 * sp.size), replace=False)
    flat[idx] = np.resize(sp, idx.size)
    return a


@pytest.mark.parametrize("N", [1, 3, TILE - 1, TILE, TILE + 1, 4 * TILE + 1])
def test_pack_and_unpack_alone_are_exact_copies(pkg, synth, dev, N):
    """N x CH for CH one below, at and above the tile edge and past two tiles, both sides, with and without mask / ReLU,
    n_images in {0, 1, N - 1, N}, blocks {4, 8, 64, 256}, into NaN-filled buffers with a guard past the end: every element
    the definition names is written (zeros included), nothing else changes."""
    guard = 37
    for CH in (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 2):
        s = ip_shape(synth, "alone_%d_%d" % (N, CH), N, CH, CH, sparsity=0.5)
        w = synth.pruned_weights(s, 11)
        src = _special((N, CH), 1000 + N + CH)
        mask = _special((N, CH), 2000 + N + CH)
        srcd, maskd = _up(src, dev), _up(mask, dev)
        for B in (4, 8, 64, 256):
            plan = _plan(pkg, s, w, kernel=pkg.KERNEL_GENERIC, b2s_block=B)
            assert plan.stat("b2s") == 1 and plan.stat("b2s_block") == B
            np_full = -(-N // B)
            for top_side in (False, True):
                for n in sorted({0, 1, N - 1, N}):
                    for use_mask in (False, True):
                        pre = seeded((np_full * CH * B + guard,), 7)
                        pre[::3] = np.nan
                        dst = _up(pre, dev)
                        plan.b2s_pack(srcd, dst, mask=maskd if use_mask else None, top_side=top_side, n_images=n)
                        want = pack(src, B, n, mask=mask if use_mask else None, out=pre) if n else pre
                        torch.cuda.synchronize()
                        assert np.array_equal(_bits(dst.cpu().numpy()), _bits(want)), ("pack", N, CH, B, top_side, n, use_mask)
                    inner = _special((np_full * CH * B,), 3000 + N + CH + B)
                    innerd = _up(inner, dev)
                    for relu in (False, True):
                        pre = np.full((N, CH), np.nan, np.float32)
                        pre[:, ::2] = 5.0
                        out = _up(pre, dev)
                        plan.b2s_unpack(innerd, out, top_side=top_side, relu=relu, n_images=n)
                        want = unpack(inner, B, n, CH, relu=relu, out=pre) if n else pre
                        torch.cuda.synchronize()
                        assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)), ("unpack", N, CH, B, top_side, n, relu)
            plan.close()


def test_the_mask_follows_its_expression(pkg, synth, dev):
    """mask > 0 ? v : 0: a NaN, a -0.0, a +0.0 and a negative subnormal close the gate; a positive subnormal opens it."""
    s = ip_shape(synth, "mask", 5, 7, 7, sparsity=0.5)
    plan = _plan(pkg, s, synth.pruned_weights(s, 11), kernel=pkg.KERNEL_GENERIC, b2s_block=8)
    src = np.arange(1, 36, dtype=np.float32).reshape(5, 7)
    src[0, 0] = np.nan
    mask = np.resize(np.array([np.nan, -0.0, 0.0, -1e-45, 1e-45, 1e-39, 1.0, -1.0, np.inf, -np.inf], np.float32), (5, 7)).copy()
    dst = _nan((1 * 7 * 8,), dev)
    plan.b2s_pack(_up(src, dev), dst, mask=_up(mask, dev))
    got = dst.cpu().numpy().reshape(1, 7, 8)
    for n in range(5):
        for c in range(7):
            m = mask[n, c]
            want = src[n, c] if (m > 0) else np.float32(0)                        # (NaN > 0 is False)
            assert _bits(got[0, c, n]) == _bits(want), (n, c, m)
    assert not got[0, :, 5:].any() and not np.signbit(got[0, :, 5:]).any()           # the padding positions are +0
    with pytest.raises(pkg.EscoinError) as e:
        pkg.check(pkg.lib().escoin_plan_b2s_pack(plan._h, None, None, ctypes.c_void_p(dst.data_ptr()), 0, 1, None), "b2s_pack")
    assert "failed (-1)" in str(e.value)
    for n in (-1, 6):
        with pytest.raises(pkg.EscoinError) as e:
            plan.b2s_pack(_up(src, dev), dst, n_images=n) if n < 0 else pkg.check(
                pkg.lib().escoin_plan_b2s_unpack(plan._h, ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(dst.data_ptr()), 0, 0, n, None), "b2s_unpack")
        assert "failed (-1)" in str(e.value)
    plan.close()
    plain = _plan(pkg, s, synth.pruned_weights(s, 11), b2s=0)
    for call in (lambda: plain.b2s_pack(_up(src, dev), dst), lambda: plain.b2s_unpack(dst, _up(src, dev))):
        with pytest.raises(pkg.EscoinError) as e:
            call()
        assert "failed (-4)" in str(e.value)                                          # ESCOIN_ESTATE
    plain.close()


# ---- 2. forward ---------------------------------------------------------------------------------------------------------------------
def _forward(pkg, dev, s, sk, plan, relu, bias=True, n=None):
    n = s.N if n is None else n
    top = _nan((s.N, s.M, 1, 1), dev)
    L = pkg.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    xd = _up(sk.x, dev)
    bd_ = _up(sk.b, dev) if bias else None
    pkg.check(L.escoin_forward(plan._h, ctypes.c_void_p(xd.data_ptr()), None if bd_ is None else ctypes.c_void_p(bd_.data_ptr()),
                               ctypes.c_void_p(top.data_ptr()), n, stream), "escoin_forward")
    torch.cuda.synchronize()
    return top.cpu().numpy()


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_within_the_float64_error_bound(pkg, synth, dev, name, kernel, relu):
    """Every shape (bias / none, group 2, M of 1 / 10 / 65) on every inner kernel; a forced TILED / JIT that the inner layer
    does not fit refuses with ESCOIN_EINVAL."""
    s, sk = _case(synth, make(synth, name))
    opts = {} if kernel == "AUTO" else dict(kernel=_k(pkg, kernel))
    try:
        plan = _plan(pkg, s, sk.w, relu, **opts)
    except pkg.EscoinError as e:
        assert kernel in ("TILED", "JIT") and "failed (-1)" in str(e), (name, kernel, str(e))
        print("b2s %s: forced %s does not fit the inner layer: %s" % (name, kernel, e))
        return
    _active(pkg, plan, s)
    if kernel != "AUTO":
        assert plan.stat("kernel_choice") == _k(pkg, kernel), plan.kernel_name
    want, B = _fwd_bound(s, sk, relu)
    got = _forward(pkg, dev, s, sk, plan, relu)
    r = eb.within(got, want, B, plan.kernel_name, sk.row_exp, what=(name, kernel, relu))
    if not s.bias:
        assert _forward(pkg, dev, s, sk, plan, relu, bias=False).tobytes() == got.tobytes()
    else:                                                                              # a NULL bias on a has_bias plan
        want0, B0 = _fwd_bound(s, sk, relu, bias=False)
        eb.within(_forward(pkg, dev, s, sk, plan, relu, bias=False), want0, B0, plan.kernel_name, sk.row_exp, what=(name, kernel, "NULL bias"))
    print("errbound b2s %-8s relu=%d %-70s forward %.3g" % (name, relu, plan.kernel_name, r))
    plan.close()


@pytest.mark.parametrize("name", ["ip_g2", "ip_wide"])
def test_tiled_kernels_fit_an_inner_layer_of_full_rows(pkg, synth, dev, name):
    """The rule's 64-wide rows are a layer the tiled kernels serve: forced TILED and JIT align."""
    s, sk = _case(synth, make(synth, name))
    for kernel in ("TILED", "JIT"):
        plan = _plan(pkg, s, sk.w, kernel=_k(pkg, kernel))
        assert plan.stat("b2s") == 1 and plan.stat("kernel_choice") == _k(pkg, kernel) and plan.stat("b2s_block") == 64
        plan.close()


@pytest.mark.parametrize("name", ["ip_g2", "ip_wide", "ip_m65"])
def test_partial_batches_tiling_batch_and_the_sub_batch_loop(pkg, synth, dev, name):
    """n_images in {0, 1, N - 1} into a NaN-filled top whose other images stay NaN, the bottom's images past n_images NaN
    (not read); a plan tiled as for a batch of 4096; a max_launch_bytes of one inner image."""
    s, sk = _case(synth, make(synth, name))
    want, B = _fwd_bound(s, sk, False)
    for opts in ({}, dict(tiling_batch=4096), dict(max_launch_bytes=4 * s.C * 64)):
        plan = _plan(pkg, s, sk.w, **opts)
        _active(pkg, plan, s)
        for n in (0, 1, s.N - 1, s.N):
            x = sk.x.copy()
            x[n:] = np.nan
            got = _forward(pkg, dev, s, sk._replace(x=x), plan, False, n=n)
            assert np.all(np.isnan(got[n:])) and not np.any(np.isnan(got[:n])), (name, n, opts)
            eb.within(got[:n], want[:n], B[:n], plan.kernel_name, sk.row_exp, what=(name, "n_images", n, opts))
        plan.close()


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_the_generic_kernel_inside_gives_the_bits_of_the_plan_without_the_option(pkg, synth, dev, name, relu):
    s, sk = _case(synth, make(synth, name))
    out = []
    for b2s in (1, 0):
        plan = _plan(pkg, s, sk.w, relu, b2s=b2s, kernel=pkg.KERNEL_GENERIC)
        assert plan.stat("b2s") == b2s and plan.stat("kernel_choice") == pkg.KERNEL_GENERIC
        out.append(_forward(pkg, dev, s, sk, plan, relu))
        plan.close()
    assert same_bits(out[0], out[1]) and np.all(np.isfinite(out[0]))


@pytest.mark.parametrize("name", ["ip_small", "ip_g2", "ip_wide"])
def test_sparse_inner_kernels_do_not_depend_on_the_block_or_on_n_images(pkg, synth, dev, name):
    """An element's sum order is a function of the pattern: the same bits for blocks 4, 64, 256 and the rule's, and for
    every n_images that covers the image ("dense_threshold_pct" = 100 keeps AUTO on the sparse kernels)."""
    s, sk = _case(synth, make(synth, name))
    for kernel in ("AUTO", "JIT", "TILED"):           # (AUTO takes the generic kernel on launches this small)
        opts = dict(dense_threshold_pct=100) if kernel == "AUTO" else dict(kernel=_k(pkg, kernel))
        ref, names = None, []
        for B in (0, 4, 64, 256):
            plan = _plan(pkg, s, sk.w, b2s_block=B, **opts)
            assert plan.stat("b2s") == 1 and plan.stat("kernel_choice") == (pkg.KERNEL_GENERIC if kernel == "AUTO" else _k(pkg, kernel))
            names.append(plan.tiling_info[:40])
            full = _forward(pkg, dev, s, sk, plan, False)
            ref = full if ref is None else ref
            assert same_bits(full, ref), (name, kernel, B, names)
            for n in (1, s.N - 1):
                assert same_bits(_forward(pkg, dev, s, sk, plan, False, n=n)[:n], ref[:n]), (name, kernel, B, n, names)
            plan.close()
        print("b2s %s %s: equal bits across %s" % (name, kernel, names))


# ---- 3. backward ------------------------------------------------------------------------------------------------------------------
def _backward_all(pkg, dev, s, sk, plan, relu, top_np=None, explicit=None):
    """Data, dense-layout weight, compact weight and bias gradients into prefilled outputs, each within its bound."""
    xd, tdd = _up(sk.x, dev), _up(sk.top_diff, dev)
    topd = _up(top_np, dev) if relu else None
    pattern = (sk.w != 0) if explicit is None else explicit
    wantb, Bs = eb.backward_bound(s, sk.w, sk.x, sk.b, sk.top_diff, top_np if relu else None, mask=pattern)
    base_w = seeded(sk.w.shape, 61)
    pre_w = np.where(pattern, base_w, np.nan).astype(np.float32)                      # += inside the pattern, NaN outside it stays
    base_b = seeded((s.M,), 62)
    bd, wd, bsd = plan.backward(tdd, bottom=xd, top=topd, bottom_diff=_nan((s.N, s.C, 1, 1), dev), weight_diff=_up(pre_w, dev),
                                bias_diff=_up(base_b, dev) if s.bias else None)
    torch.cuda.synchronize()
    label = "b2s dgrad %d wgrad %d" % (plan.stat("bwd_data_kernel"), plan.stat("wgrad_kernel"))
    r0 = eb.within(bd.cpu().numpy(), wantb[0], Bs[0], label, sk.chan_exp, what=(s.name, "data"))
    wd = wd.cpu().numpy()
    assert np.all(np.isnan(wd[~pattern])) and not np.any(np.isnan(wd[pattern]))
    u = 2.0 ** -24
    r1 = eb.within(np.where(pattern, wd - base_w.astype(np.float64), 0.0), wantb[1] * pattern, Bs[1] + u * (np.abs(base_w) + np.abs(wantb[1])),
                   label, what=(s.name, "weights +="))
    r2 = 0.0 if not s.bias else eb.within(bsd.cpu().numpy() - base_b.astype(np.float64), wantb[2],
                                          Bs[2] + u * (np.abs(base_b) + np.abs(wantb[2])), label, what=(s.name, "bias +="))
    _, vd, _ = plan.backward(tdd, bottom=xd, top=topd, bottom_diff=None, values_diff=True)
    torch.cuda.synchronize()
    rp, ci, _, ng = plan.get_csr()
    from prune_common import positions
    pos = positions(s, rp, ci, ng)
    r3 = eb.within(vd.cpu().numpy(), wantb[1].reshape(-1)[pos], Bs[1].reshape(-1)[pos], label, what=(s.name, "compact"))
    return label, (r0, r1, r2, r3)


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("kernel", ["AUTO", "GENERIC", "DENSE"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_backward_within_the_float64_error_bound(pkg, synth, dev, name, kernel, relu):
    s, sk = _case(synth, make(synth, name))
    plan = _plan(pkg, s, sk.w, relu, **({} if kernel == "AUTO" else dict(kernel=_k(pkg, kernel), backward_kernel=_k(pkg, kernel))))
    top = _forward(pkg, dev, s, sk, plan, relu)
    label, r = _backward_all(pkg, dev, s, sk, plan, relu, top)
    _active(pkg, plan, s)
    assert plan.stat("bwd_device_bytes") > 0
    print("errbound b2s %-8s relu=%d %s: data %.3g, weights %.3g, bias %.3g, compact %.3g" % ((name, relu, label) + r))
    plan.close()


def test_every_backward_and_weight_gradient_kernel_or_a_refusal(pkg, synth, dev):
    """backward_kernel and wgrad_kernel go to the inner plan as they stand: each one it serves within the bound, each one it
    does not refused with ESCOIN_EINVAL at the first backward, the plan still usable."""
    s, sk = _case(synth, make(synth, "ip_wide"))
    served, refused = [], []
    for bk in ("KERNEL_AUTO", "KERNEL_GENERIC", "KERNEL_TILED", "KERNEL_JIT", "KERNEL_DENSE", "BWD_MFMA"):
        for wk in ("WGRAD_AUTO", "WGRAD_ENTRY", "WGRAD_STAGED", "WGRAD_MFMA"):
            plan = _plan(pkg, s, sk.w, backward_kernel=getattr(pkg, bk), wgrad_kernel=getattr(pkg, wk))
            try:
                label, r = _backward_all(pkg, dev, s, sk, plan, False)
            except pkg.EscoinError as e:
                assert "failed (-1)" in str(e), (bk, wk, str(e))
                refused.append((bk, wk))
                assert plan.stat("b2s") == 1 and np.all(np.isfinite(_forward(pkg, dev, s, sk, plan, False)))
            else:
                served.append((bk, wk, label))
                if bk not in ("KERNEL_AUTO", "KERNEL_TILED", "KERNEL_JIT"):
                    want = {"KERNEL_GENERIC": pkg.KERNEL_GENERIC, "KERNEL_DENSE": pkg.KERNEL_DENSE, "BWD_MFMA": pkg.BWD_MFMA}[bk]
                    assert plan.stat("bwd_data_kernel") == want, (bk, plan.stat("bwd_data_kernel"))
                if wk != "WGRAD_AUTO":
                    assert plan.stat("wgrad_kernel") == getattr(pkg, wk)
            plan.close()
    print("b2s served %s\nb2s refused %s" % (served, refused))
    assert {(b, w) for b, w, _ in served} >= {(b, w) for b in ("KERNEL_AUTO", "KERNEL_GENERIC") for w in ("WGRAD_AUTO", "WGRAD_ENTRY")}


def test_an_explicit_zero_receives_its_gradient_and_null_outputs_are_skipped(pkg, synth, dev):
    s, sk = _case(synth, make(synth, "ip_g2"))
    plan = _plan(pkg, s, sk.w)
    rp, ci, vals, ng = plan.get_csr()
    vals = vals.copy()
    vals[::5] = 0.0                                                                   # explicit zeros: still entries
    plan.set_values(_up(vals, dev))
    from prune_common import positions
    pos = positions(s, rp, ci, ng)
    w = np.zeros(sk.w.size, np.float32)
    w[pos] = vals
    pattern = np.zeros(sk.w.size, bool)
    pattern[pos] = True
    sk0 = sk._replace(w=w.reshape(sk.w.shape))
    label, r = _backward_all(pkg, dev, s, sk0, plan, False, explicit=pattern.reshape(sk.w.shape))
    # NULL outputs: each gradient alone equals the same gradient of the full call, bit for bit
    xd, tdd = _up(sk.x, dev), _up(sk.top_diff, dev)
    full = plan.backward(tdd, bottom=xd, bottom_diff=True, weight_diff=True, bias_diff=True)
    only = (plan.backward(tdd, bottom_diff=True)[0], plan.backward(tdd, bottom=xd, bottom_diff=None, weight_diff=True)[1],
            plan.backward(tdd, bottom_diff=None, bias_diff=True)[2])
    torch.cuda.synchronize()
    for a, b in zip(full, only):
        assert same_bits(a.cpu().numpy(), b.cpu().numpy())
    plan.close()


def test_two_calls_on_two_streams_give_identical_bits(pkg, synth, dev):
    s, sk = _case(synth, make(synth, "ip_wide"))
    plan = _plan(pkg, s, sk.w, relu=True)
    xd, bd_, tdd = _up(sk.x, dev), _up(sk.b, dev), _up(sk.top_diff, dev)
    outs = []
    for stream in (torch.cuda.current_stream(), torch.cuda.Stream()):
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            top = plan.forward(xd, bd_)
            bd, wd, bsd = plan.backward(tdd, bottom=xd, top=top, bottom_diff=True, weight_diff=True, bias_diff=True)
        stream.synchronize()
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy() for t in (top, bd, wd, bsd)])
    for a, b in zip(*outs):
        assert same_bits(a, b) and np.all(np.isfinite(a))
    assert np.abs(outs[0][1]).max() > 0 and np.abs(outs[0][2]).max() > 0
    plan.close()


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
def test_dense_wgrad_against_the_full_float64_weight_gradient(pkg, synth, dev, relu):
    s, sk = _case(synth, make(synth, "ip_g2"))
    plan = _plan(pkg, s, sk.w, relu)
    top = _forward(pkg, dev, s, sk, plan, relu)
    everywhere = np.ones(sk.w.shape, bool)
    wantb, Bs = eb.backward_bound(s, sk.w, sk.x, sk.b, sk.top_diff, top if relu else None, mask=everywhere)
    xd, tdd, topd = _up(sk.x, dev), _up(sk.top_diff, dev), _up(top, dev) if relu else None
    got = plan.dense_wgrad(tdd, xd, top=topd)
    torch.cuda.synchronize()
    eb.within(got.cpu().numpy(), wantb[1], Bs[1], "b2s dense_wgrad", what=(s.name, relu))
    part = plan.dense_wgrad(tdd, xd, top=topd, n_images=s.N - 1)
    wantp, Bp = eb.backward_bound(s, sk.w, sk.x[:-1], sk.b, sk.top_diff[:-1], top[:-1] if relu else None, mask=everywhere)
    eb.within(part.cpu().numpy(), wantp[1], Bp[1], "b2s dense_wgrad", what=(s.name, relu, "partial"))
    assert plan.stat("b2s") == 1 and plan.stat("dwg_count") == 2 and plan.stat("dwg_device_bytes") > 0
    _active(pkg, plan, s)
    plan.close()


# ---- 4. non-finite containment -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["AUTO", "DENSE", "GENERIC"])
def test_a_non_finite_image_changes_its_own_outputs_only(pkg, synth, dev, kernel):
    """A NaN and an infinity in one bottom image (and in one top_diff image): every other image keeps the bits of the clean
    run, with the DENSE kernel inside too -- the poisoned image's neighbours in its inner image are other pixels of the
    pointwise layer, and the padding is +0 written by the pack kernel."""
    s, sk = _case(synth, make(synth, "ip_wide"))
    opts = {} if kernel == "AUTO" else dict(kernel=_k(pkg, kernel), backward_kernel=_k(pkg, kernel))
    plan = _plan(pkg, s, sk.w, **opts)
    tdd = _up(sk.top_diff, dev)
    clean = _forward(pkg, dev, s, sk, plan, False)
    clean_bd = plan.backward(tdd, bottom_diff=True)[0].cpu().numpy()
    for victim in (0, 65, s.N - 1):
        x = sk.x.copy()
        x[victim, 3], x[victim, 10] = np.nan, np.inf
        got = _forward(pkg, dev, s, sk._replace(x=x), plan, False)
        others = np.arange(s.N) != victim
        assert same_bits(got[others], clean[others]), (kernel, victim)
        assert not np.all(np.isfinite(got[victim]))
        td = sk.top_diff.copy()
        td[victim, 2], td[victim, 5] = np.nan, -np.inf
        bd = plan.backward(_up(td, dev), bottom_diff=True)[0].cpu().numpy()
        assert same_bits(bd[others], clean_bd[others]), (kernel, victim)
        assert not np.all(np.isfinite(bd[victim]))
    # the last inner image is partial (130 = 2 * 64 + 2): a run of fewer images reads no stale pixel of the scratch either
    x = sk.x.copy()
    x[100:] = np.nan
    _forward(pkg, dev, s, sk._replace(x=x), plan, False)
    assert same_bits(_forward(pkg, dev, s, sk, plan, False, n=70)[:70], clean[:70])
    plan.close()


# ---- 5. lifecycle ----------------------------------------------------------------------------------------------------------------------
def _fresh_equals(pkg, dev, s, sk, plan, step, **opts):
    """Forward and the whole backward of `plan` equal, bit for bit, those of a fresh b2s plan aligned by set_csr on its CSR."""
    xd, bd_, tdd = _up(sk.x, dev), _up(sk.b, dev), _up(sk.top_diff, dev)
    rp, ci, vals, ng = plan.get_csr()               # (brings the host values up to date)
    fresh = pkg.Plan(pkg.ConvDesc.from_shape(s), b2s=1, **opts)
    fresh.set_csr(rp, ci, vals, ng)
    out = []
    for p in (plan, fresh):
        top = p.forward(xd, bd_)
        bd, vd, bsd = p.backward(tdd, bottom=xd, bottom_diff=_nan((s.N, s.C, 1, 1), dev), values_diff=True, bias_diff=True if s.bias else None)
        torch.cuda.synchronize()
        assert p.stat("b2s") == 1
        out.append([t.cpu().numpy() for t in (top, bd, vd)])
    assert plan.kernel_name == fresh.kernel_name and plan.stat("bwd_data_kernel") == fresh.stat("bwd_data_kernel")
    fresh.close()
    for a, b in zip(*out):
        assert same_bits(a, b) and np.all(np.isfinite(a)), (s.name, step)
    return out[0]


@pytest.mark.parametrize("kernel", ["AUTO", "DENSE"])
@pytest.mark.parametrize("name", ["ip_g2", "ip_wide"])
def test_updates_reach_the_inner_plan_in_place(pkg, synth, dev, name, kernel):
    s, sk = _case(synth, make(synth, name))
    opts = {} if kernel == "AUTO" else dict(kernel=pkg.KERNEL_DENSE)
    plan = _plan(pkg, s, sk.w, **opts)
    nnz = plan.nnz()
    v1 = values_at(plan, new_weights(sk.w, 41)[0])[2]
    plan.set_values(_up(v1, dev))                       # before the inner backward state exists
    assert plan.stat("update_fast") == 1 and plan.stat("b2s") == 1
    before = plan.stat("update_destinations")
    assert before >= 2 * nnz                            # the value array and the inner plan's copies
    assert same_bits(plan.get_csr()[2], v1)
    g0 = _fresh_equals(pkg, dev, s, sk, plan, "set_values before the first backward", **opts)
    v2 = values_at(plan, new_weights(sk.w, 42)[0])[2]
    plan.set_values(_up(v2, dev))
    assert plan.stat("update_fast") == 1
    assert plan.stat("update_destinations") > before    # the inner backward state's copies joined the list
    g1 = _fresh_equals(pkg, dev, s, sk, plan, "set_values", **opts)
    assert not np.array_equal(g0[0], g1[0]) and not np.array_equal(g0[1], g1[1])
    _, w3_nan = new_weights(sk.w, 43)
    plan.update_values(_up(w3_nan, dev))                # device source, NaN outside the pattern
    assert plan.stat("update_fast") == 1
    g2 = _fresh_equals(pkg, dev, s, sk, plan, "update_values", **opts)
    assert not np.array_equal(g1[1], g2[1])
    after = plan.stat("update_destinations")
    vd, h = _up(seeded((nnz,), 44), dev), torch.zeros(nnz, device=dev)
    plan.solver_step(vd, h, type="sgd", rate=0.05, momentum=0.9)
    assert plan.stat("update_fast") == 1 and plan.stat("update_destinations") == after
    g3 = _fresh_equals(pkg, dev, s, sk, plan, "solver_step", **opts)
    assert not np.array_equal(g2[0], g3[0])
    plan.set_values(v1)                                 # host source
    assert plan.stat("update_fast") == 1 and same_bits(plan.get_csr()[2], v1)
    g4 = _fresh_equals(pkg, dev, s, sk, plan, "set_values from the host", **opts)
    assert same_bits(g4[0], g0[0]) and same_bits(g4[1], g0[1])
    plan.close()


def _passes_case_2(pkg, dev, s, plan, what):
    """The plan, whatever it went through, still computes its own CSR's layer within the bound, with the option active."""
    rp, ci, vals, ng = plan.get_csr()
    from prune_common import positions
    w = np.zeros(s.M * (s.C // s.group), np.float32)
    w[positions(s, rp, ci, ng)] = vals
    w = w.reshape(s.M, s.C // s.group, 1, 1)
    x, b = np.ascontiguousarray(seeded((s.N, s.C, 1, 1), 71)), seeded((s.M,), 72)
    want, B = eb.forward_bound(s, w, x, b)
    top = plan.forward(_up(x, dev), _up(b, dev)).cpu().numpy()
    assert plan.stat("b2s") == 1 and plan.kernel_name.startswith(PACK) and plan.kernel_name.endswith(UNPACK)
    eb.within(top, want, B, plan.kernel_name, what=(s.name, what))


def test_prune_rewire_set_csr_import_and_a_conv_mode_flip_leave_a_working_plan(pkg, synth, dev):
    s, sk = _case(synth, make(synth, "ip_g2"))
    plan = _plan(pkg, s, sk.w)
    xd, tdd = _up(sk.x, dev), _up(sk.top_diff, dev)
    plan.forward(xd)
    plan.backward(tdd, bottom=xd, weight_diff=True)     # (the states a prune has to drop exist)
    n = plan.nnz()
    entry_map = plan.prune(keep=n - n // 3)
    assert plan.nnz() == n - n // 3 and int((entry_map >= 0).sum()) == plan.nnz()
    _passes_case_2(pkg, dev, s, plan, "prune")
    _fresh_equals(pkg, dev, s, sk, plan, "prune")
    score = plan.dense_wgrad(tdd, xd)                   # rewire's grow score, through the inner plan
    n1 = plan.nnz()
    plan.rewire(n // 4, score.reshape(-1), drop_keep=n1 - n // 8)
    assert plan.nnz() == n1 - n // 8 + n // 4
    plan.set_values(_up(seeded((plan.nnz(),), 52), dev))     # grown zeros become weights, in place
    assert plan.stat("update_fast") == 1
    _passes_case_2(pkg, dev, s, plan, "rewire")
    _fresh_equals(pkg, dev, s, sk, plan, "rewire")
    rp, ci, vals, ng = plan.get_csr()
    plan.set_csr(rp, ci, vals * 2, ng)
    _passes_case_2(pkg, dev, s, plan, "set_csr")
    # export -> import: the outer CSR and no code section
    blob = plan.export_aligned()
    plain = pkg.Plan(pkg.ConvDesc.from_shape(s), kernel=pkg.KERNEL_GENERIC)
    plain.set_csr(rp, ci, vals * 2, ng)
    assert blob.size == plain.export_aligned().size
    plain.close()
    other = pkg.Plan(pkg.ConvDesc.from_shape(s), b2s=1)
    assert other.import_aligned(blob) is False
    _passes_case_2(pkg, dev, s, other, "import")
    assert all(same_bits(a, b) for a, b in zip(plan.get_csr(), other.get_csr()))
    other.close()
    # a flip to a lowered mode runs on the original geometry, and back rebuilds the inner plan
    before = plan.forward(xd).cpu().numpy()
    for mode in (pkg.CONV_MODE_LOWERED_GEMM, pkg.CONV_MODE_LOWERED_SPARSE):
        plan.set_option("conv_mode", mode)
        assert plan.stat("b2s") == 0 and "escoin_b2s" not in plan.kernel_name
        assert np.all(np.isfinite(plan.forward(xd).cpu().numpy()))
        plan.set_option("conv_mode", pkg.CONV_MODE_SCONV_PAR)
        _passes_case_2(pkg, dev, s, plan, "flip")
        assert same_bits(plan.forward(xd).cpu().numpy(), before)
    plan.close()


def test_forward_backward_and_solver_step_captured_into_one_graph(pkg, synth, dev):
    """After one uncaptured pass, forward + backward + solver step captured into one graph and replayed twice on new data:
    nothing is allocated, and each replay equals the same step run eagerly on a twin plan, bit for bit."""
    s = make(synth, "ip_wide")
    w, b = synth.pruned_weights(s, 11), synth.bias_vector(s, 13)

    def state():
        plan = _plan(pkg, s, w, relu=True)
        nnz = plan.nnz()
        u = dict(x=torch.zeros((s.N, s.C, 1, 1), device=dev), td=torch.zeros((s.N, s.M, 1, 1), device=dev),
                 y=torch.zeros((s.N, s.M, 1, 1), device=dev), bd=torch.zeros((s.N, s.C, 1, 1), device=dev), b=_up(b, dev),
                 vd=torch.zeros(nnz, device=dev), bsd=torch.zeros(s.M, device=dev), h=torch.zeros(nnz, device=dev))
        return plan, u

    def step(plan, u):
        plan.forward(u["x"], u["b"], u["y"])
        u["vd"].zero_(), u["bsd"].zero_()
        plan.backward(u["td"], bottom=u["x"], top=u["y"], bottom_diff=u["bd"], values_diff=u["vd"], bias_diff=u["bsd"])
        plan.solver_step(u["vd"], u["h"], type="sgd", rate=0.01, momentum=0.9)

    def feed(u, rnd):
        u["x"].copy_(torch.from_numpy(synth.activations(s, 900 + rnd)))
        u["td"].copy_(torch.from_numpy(seeded(tuple(u["td"].shape), 950 + rnd)))
        u["bd"].fill_(float("nan"))

    plan, u = state()
    twin, v = state()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for p, q in ((plan, u), (twin, v)):
            feed(q, 0)
            step(p, q)              # the first pass builds the inner backward state and the update state outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert plan.stat("b2s") == 1 and plan.stat("update_fast") == 1
    ws1 = plan.workspace_bytes
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(plan, u)
    assert plan.workspace_bytes == ws1
    for rnd in (1, 2):              # (a capture runs nothing: both plans have taken one step so far)
        feed(u, rnd), feed(v, rnd)
        g.replay()
        step(twin, v)
        torch.cuda.synchronize()
        for k in ("y", "bd", "vd", "bsd", "h"):
            assert same_bits(u[k].cpu().numpy(), v[k].cpu().numpy()), (k, rnd)
        assert np.all(np.isfinite(u["bd"].cpu().numpy())) and float(u["bd"].abs().max()) > 0
    assert plan.workspace_bytes == ws1 == twin.workspace_bytes
    assert same_bits(plan.get_csr()[2], twin.get_csr()[2])
    plan.close(), twin.close()


# ---- 6. where the option changes nothing ----------------------------------------------------------------------------------------------
def _unserved(synth):
    sh = synth.shape
    return [sh("u3x3", 2, 8, 9, 9, 8, 3, pad=1, sparsity=0.8), sh("upw", 2, 16, 4, 4, 24, 1, sparsity=0.8),
            sh("urow", 3, 16, 1, 6, 8, 1, sparsity=0.7), sh("upad", 3, 16, 1, 1, 8, 1, pad=1, sparsity=0.7)]


@pytest.mark.parametrize("i", range(4))
def test_unserved_layers_run_as_without_the_option(pkg, synth, dev, i):
    s = _unserved(synth)[i]
    w, x, b = synth.pruned_weights(s, 11), synth.activations(s, 12), synth.bias_vector(s, 13)
    td = seeded((s.N, s.M) + synth.out_hw(s), 21)
    out, names = [], []
    for b2s in (1, 0):
        plan = _plan(pkg, s, w, b2s=b2s)
        top = plan.forward(_up(x, dev), _up(b, dev))
        bd, wd, _ = plan.backward(_up(td, dev), bottom=_up(x, dev), bottom_diff=True, weight_diff=True)
        torch.cuda.synchronize()
        assert plan.stat("b2s") == 0 and plan.stat("b2s_block") == 0 and plan.stat("b2s_scratch_bytes") == 0
        out.append((top.cpu().numpy(), bd.cpu().numpy(), wd.cpu().numpy(), plan.workspace_bytes))
        names.append((plan.kernel_name, plan.tiling_info) + tuple(plan.stat(k) for k in (
            "kernel_choice", "bwd_data_kernel", "wgrad_kernel", "device_bytes", "bwd_device_bytes", "code_bytes", "lds_bytes", "workgroup_columns")))
        plan.close()
    assert names[0] == names[1]
    assert all(same_bits(a, c) for a, c in zip(out[0][:3], out[1][:3])) and out[0][3] == out[1][3]


def test_a_double_plan_and_the_lowered_modes_run_on_the_original_geometry(pkg, synth, dev):
    s, sk = _case(synth, make(synth, "ip_g2"))
    x64, b64 = _up(sk.x, dev, np.float64), _up(sk.b, dev, np.float64)
    ref = _plan(pkg, s, sk.w.astype(np.float64), b2s=0)
    plan = _plan(pkg, s, sk.w.astype(np.float64))
    assert plan.stat("b2s") == 0 and plan.kernel_name == ref.kernel_name and plan.workspace_bytes == ref.workspace_bytes
    assert same_bits(plan.forward(x64, b64).cpu().numpy(), ref.forward(x64, b64).cpu().numpy())
    plan.close(), ref.close()
    xd, bd_ = _up(sk.x, dev), _up(sk.b, dev)
    for mode in (pkg.CONV_MODE_LOWERED_GEMM, pkg.CONV_MODE_LOWERED_SPARSE):
        ref = _plan(pkg, s, sk.w, b2s=0, conv_mode=mode)
        plan = _plan(pkg, s, sk.w, conv_mode=mode)
        assert plan.stat("b2s") == 0 and plan.kernel_name == ref.kernel_name and plan.workspace_bytes == ref.workspace_bytes
        assert same_bits(plan.forward(xd, bd_).cpu().numpy(), ref.forward(xd, bd_).cpu().numpy())
        plan.close(), ref.close()


# ---- 7. the tool ------------------------------------------------------------------------------------------------------------------------
def test_fc_bench_runs_at_a_small_batch(tmp_path):
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    md = str(tmp_path / "b2s.md")
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "fc_bench.py"), "--tiny", "--only", "ip2,fc8", "--batch", "8",
                          "--markdown", md], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr.decode()
    res = json.loads(out.stdout.decode().strip().splitlines()[-1])
    rows = res["layers"]
    assert [r["layer"] for r in rows] == ["tiny_fc8", "tiny_ip2"] and res["batches"] == [8]
    for row in rows:
        assert row["N"] == 8 and row["forward"]["b2s"]["kernel"].startswith(PACK) and row["forward"]["b2s"]["kernel"].endswith(UNPACK)
        assert "escoin_b2s" not in row["forward"]["plain"]["kernel"]
        for k in ("forward", "data_gradient", "compact_wgrad"):
            assert row[k]["b2s"]["median_us"] > 0 and row[k]["plain"]["median_us"] > 0
        for k in ("pack", "unpack", "pack_copy", "unpack_copy"):
            assert row[k]["median_us"] > 0
        assert set(row["blocks"]) == {"64", "128", "256"} and row["dense"]["median_us"] > 0
        assert row["align_us"] > 0 and row["code_bytes"] >= 0
    assert "pack GB/s" in open(md).read()
