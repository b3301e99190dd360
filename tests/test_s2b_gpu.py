"""Plan option "s2b" on the MI355X: dilated stride-1 layers through escoin_s2b_pack_kernel, an undilated inner plan of
N * P images and escoin_s2b_unpack_kernel.  Forward and data gradient of the shapes of s2b_common.SHAPES and a seeded slice
of random geometries against torch float64 and the per-element bound of errbound.py, on inputs whose rows, channels and
images differ in scale by up to 2^48 (errbound.skew); the inner kernel forced and automatic; partial batches into NaN-filled
blobs; exact zeros where no window reads; determinism; the weight gradients and dense_wgrad against the same plan without
the option; in-place updates, prune and rewire against fresh plans; export / import; a captured training step; the layers
the option does not serve; the two measurement hooks and the bench tool.  Every case that the option serves asserts
stat("s2b") == 1, the three-part kernel name and the byte accounting."""
import ctypes

import numpy as np
import pytest

import errbound as eb
from s2b_common import SHAPES, UNSERVED, inner_dims, make, random_shapes
from upd_common import new_weights, same_bits, values_at

torch = pytest.importorskip("torch")

from wgrad_common import seeded  # noqa: E402

pytestmark = pytest.mark.gpu
PACK = "escoin_s2b_pack_kernel + "
UNPACK = " + escoin_s2b_unpack_kernel"


@pytest.fixture(scope="module")
def dev(pkg):
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        pytest.fail("no HIP device visible (these tests run on the MI355X)")
    return torch.device("cuda:0")


_CASES = {}


def _case(synth, s, w_seed=11):
    """(shape, skewed inputs) of a shape: made once, never written."""
    if s.name not in _CASES:
        w = synth.pruned_weights(s, w_seed)
        x, b = synth.activations(s, 12), synth.bias_vector(s, 13)
        td = seeded((s.N, s.M) + synth.out_hw(s), 21)
        _CASES[s.name] = (s, eb.skew(s, w, x, b, 95, top_diff=td))
    return _CASES[s.name]


_BOUNDS = {}


def _fwd_bound(s, sk, relu):
    key = (s.name, relu)
    if key not in _BOUNDS:
        _BOUNDS[key] = eb.forward_bound(s, sk.w, sk.x, sk.b, relu=relu)
    return _BOUNDS[key]


def _up(a, dev, dt=np.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)


def _plan(pkg, s, w, relu=False, s2b=1, **opts):
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu), s2b=s2b, **opts)
    plan.weight_align(w)
    return plan


def _active(pkg, synth, plan, s):
    """The option is active: the stats, the names and the accounting of the scratch."""
    _, _, P, hi, wi, ohi, owi = inner_dims(s, synth)
    assert plan.stat("s2b") == 1 and plan.stat("s2d") == 0
    assert plan.stat("s2b_scratch_bytes") == 4 * (s.N * P * s.C * hi * wi + s.N * P * s.M * ohi * owi)
    name = plan.kernel_name
    assert name.startswith(PACK) and name.endswith(UNPACK) and len(name) > len(PACK) + len(UNPACK)
    assert "escoin_s2b" not in name[len(PACK):-len(UNPACK)]               # the inner plan's own name in between
    assert plan.stat("device_bytes") > plan.stat("s2b_scratch_bytes")
    assert plan.workspace_bytes == (plan.stat("device_bytes") + plan.stat("bwd_device_bytes") + plan.stat("upd_device_bytes") +
                                    plan.stat("dwg_device_bytes"))


def _nan_like(s, dev):
    return torch.full((s.N, s.C, s.H, s.W), float("nan"), device=dev)


def _check_shape(pkg, synth, dev, s, sk, relu, kernel=None, **opts):
    """Forward and data gradient of one skewed layer under the option: every element within the bound of the float64 reference."""
    kw = dict(opts) if kernel is None else dict(opts, kernel=kernel)
    xd, bd_, tdd = _up(sk.x, dev), _up(sk.b, dev), _up(sk.top_diff, dev)
    plan = _plan(pkg, s, sk.w, relu, **kw)
    _active(pkg, synth, plan, s)
    if kernel in (pkg.KERNEL_GENERIC, pkg.KERNEL_DENSE, pkg.KERNEL_JIT, pkg.KERNEL_TILED):
        assert plan.stat("kernel_choice") == kernel, plan.kernel_name
    what = (s.name, "relu", relu, "kernel", kernel)
    want, B = _fwd_bound(s, sk, relu)
    oh, ow = synth.out_hw(s)
    top = plan.forward(xd, bd_, torch.full((s.N, s.M, oh, ow), float("nan"), device=dev))
    torch.cuda.synchronize()
    top_np = top.cpu().numpy()
    rf = eb.within(top_np, want, B, plan.kernel_name, sk.row_exp, what=what)
    wantb, Bs = eb.backward_bound(s, sk.w, sk.x, sk.b, sk.top_diff, top_np if relu else None)
    got, _, _ = plan.backward(tdd, top=top if relu else None, bottom_diff=_nan_like(s, dev))
    torch.cuda.synchronize()
    rb = eb.within(got.cpu().numpy(), wantb[0], Bs[0], "s2b bwd_data_kernel %d" % plan.stat("bwd_data_kernel"), sk.chan_exp, what=what)
    _active(pkg, synth, plan, s)
    print("errbound s2b %-14s relu=%d %-60s forward %.3g, data gradient %.3g" % (s.name, relu, plan.kernel_name, rf, rb))
    assert rf <= 1.0 and rb <= 1.0
    plan.close()


# ---- 1. every shape against the float64 reference ------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("kernel", ["AUTO", "GENERIC", "DENSE"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_element_within_the_float64_error_bound(pkg, synth, dev, name, kernel, relu):
    s, sk = _case(synth, make(synth, name))
    _check_shape(pkg, synth, dev, s, sk, relu, None if kernel == "AUTO" else getattr(pkg, "KERNEL_" + kernel))


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("kernel", ["JIT", "TILED"])
@pytest.mark.parametrize("name", ["res_like"])
def test_forced_tiled_inner_kernels_within_the_bound(pkg, synth, dev, name, kernel, relu):
    s, sk = _case(synth, make(synth, name))
    _check_shape(pkg, synth, dev, s, sk, relu, getattr(pkg, "KERNEL_" + kernel), backward_kernel=getattr(pkg, "KERNEL_" + kernel))


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
def test_random_geometries_within_the_bound(pkg, synth, dev, relu):
    for i, s in enumerate(random_shapes(synth)):
        s, sk = _case(synth, s, w_seed=100 + i)
        _check_shape(pkg, synth, dev, s, sk, relu)


@pytest.mark.parametrize("bk", ["GENERIC", "BWD_MFMA"])
def test_generic_and_mfma_backward_kernels_stay_with_the_outer_plan(pkg, synth, dev, bk):
    s, sk = _case(synth, make(synth, "3x3_d2x3_g2"))
    code = pkg.KERNEL_GENERIC if bk == "GENERIC" else pkg.BWD_MFMA
    plan = _plan(pkg, s, sk.w, backward_kernel=code)
    wantb, Bs = eb.backward_bound(s, sk.w, sk.x, sk.b, sk.top_diff)
    got, _, _ = plan.backward(_up(sk.top_diff, dev), bottom_diff=_nan_like(s, dev))
    torch.cuda.synchronize()
    _active(pkg, synth, plan, s)
    assert plan.stat("bwd_data_kernel") == code
    eb.within(got.cpu().numpy(), wantb[0], Bs[0], bk, sk.chan_exp, what=(s.name, bk))
    plan.close()


def test_forced_tiled_kernels_refuse_an_inner_layer_they_do_not_fit(pkg, synth, dev):
    """A 7-wide row kernel stays 7 wide in the inner plan: KW > 5 is no tiled layer."""
    s = synth.shape("k7_d2", 1, 2, 5, 40, 3, 1, KW=7, dil=2, sparsity=0.5)
    w = synth.pruned_weights(s, 11)
    for k in (pkg.KERNEL_TILED, pkg.KERNEL_JIT):
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s), kernel=k, s2b=1)
        with pytest.raises(pkg.EscoinError) as e:
            plan.weight_align(w)
        assert "failed (-1)" in str(e.value)            # ESCOIN_EINVAL
        plan.close()
    plan = _plan(pkg, s, w)                              # AUTO serves it
    assert plan.stat("s2b") == 1
    plan.close()


# ---- 2. partial batches ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["3x3_d2", "3x3_d2x3_g2", "one_tap_axis", "d_gt_out"])
def test_partial_batches_leave_the_other_images_untouched(pkg, synth, dev, name):
    """top and bottom_diff pre-filled with NaN: images at or past n_images stay NaN, none survives below; n_images = 0
    writes nothing.  The bottom's and top_diff's images past n_images are NaN too: they are not read."""
    s, sk = _case(synth, make(synth, name))
    want, B = _fwd_bound(s, sk, False)
    wantb, Bs = eb.backward_bound(s, sk.w, sk.x, sk.b, sk.top_diff)
    plan = _plan(pkg, s, sk.w)
    oh, ow = synth.out_hw(s)
    L = pkg.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for n in (0, s.N - 1, 1):
        assert 0 <= n < s.N
        x, td = sk.x.copy(), sk.top_diff.copy()
        x[n:], td[n:] = np.nan, np.nan
        xd, tdd, bd_ = _up(x, dev), _up(td, dev), _up(sk.b, dev)
        top = torch.full((s.N, s.M, oh, ow), float("nan"), device=dev)
        full = _nan_like(s, dev)
        pkg.check(L.escoin_forward(plan._h, p(xd), p(bd_), p(top), n, stream), "escoin_forward")
        pkg.check(L.escoin_backward(plan._h, None, None, p(tdd), p(full), None, None, n, stream), "escoin_backward")
        torch.cuda.synchronize()
        assert plan.stat("s2b") == 1
        got, gotb = top.cpu().numpy(), full.cpu().numpy()
        assert np.all(np.isnan(got[n:])) and np.all(np.isnan(gotb[n:])), (name, n)
        assert not np.any(np.isnan(got[:n])) and not np.any(np.isnan(gotb[:n])), (name, n)
        eb.within(got[:n], want[:n], B[:n], plan.kernel_name, sk.row_exp, what=(name, "n_images", n))
        eb.within(gotb[:n], wantb[0][:n], Bs[0][:n], "s2b backward", sk.chan_exp, what=(name, "n_images", n))
    plan.close()


def test_rows_and_columns_no_window_reads_get_a_zero_gradient(pkg, synth, dev):
    """d_gt_out: OH = 1 < eh = 3 on a 7-row image without pad.  Windows read rows 0, 3 and 6 alone; the residue classes of
    rows 1 and 2 are inner images whose G' is all zeros, and their rows of bottom_diff are exact +0."""
    s, sk = _case(synth, make(synth, "d_gt_out"))
    assert synth.out_hw(s)[0] == 1
    plan = _plan(pkg, s, sk.w)
    got, _, _ = plan.backward(_up(sk.top_diff, dev), bottom_diff=_nan_like(s, dev))
    torch.cuda.synchronize()
    assert plan.stat("s2b") == 1
    got = got.cpu().numpy()
    dead = got[:, :, [1, 2, 4, 5], :]
    assert not dead.any() and not np.signbit(dead).any()
    assert np.abs(got[:, :, 0::3, :]).max() > 0
    plan.close()


# ---- 3. determinism, and the gradients the option leaves alone -----------------------------------------------------------
@pytest.mark.parametrize("name", ["3x3_d2", "res_like"])
def test_calling_twice_gives_equal_bits(pkg, synth, dev, name):
    s, sk = _case(synth, make(synth, name))
    xd, bd_, tdd = _up(sk.x, dev), _up(sk.b, dev), _up(sk.top_diff, dev)
    plan = _plan(pkg, s, sk.w)
    outs = []
    for _ in range(2):
        top = plan.forward(xd, bd_)
        bd, _, _ = plan.backward(tdd, bottom_diff=_nan_like(s, dev))
        torch.cuda.synchronize()
        outs.append((top.cpu().numpy(), bd.cpu().numpy()))
    assert plan.stat("s2b") == 1
    assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1])
    assert np.all(np.isfinite(outs[0][0])) and np.abs(outs[0][1]).max() > 0
    plan.close()


@pytest.mark.parametrize("name", ["3x3_d2x3_g2", "5x5_d2"])
def test_weight_bias_compact_and_dense_gradients_equal_the_plan_without_the_option(pkg, synth, dev, name):
    s, sk = _case(synth, make(synth, name))
    xd, tdd = _up(sk.x, dev), _up(sk.top_diff, dev)
    got = []
    for s2b in (1, 0):
        plan = _plan(pkg, s, sk.w, s2b=s2b)
        _, wd, bsd = plan.backward(tdd, bottom=xd, bottom_diff=None, weight_diff=True, bias_diff=bool(s.bias) or None)
        _, vd, _ = plan.backward(tdd, bottom=xd, bottom_diff=True, values_diff=True)
        dw = plan.dense_wgrad(tdd, xd)
        torch.cuda.synchronize()
        assert plan.stat("s2b") == s2b
        got.append((wd.cpu().numpy(), None if bsd is None else bsd.cpu().numpy(), vd.cpu().numpy(), dw.cpu().numpy()))
        plan.close()
    assert same_bits(got[0][0], got[1][0]) and same_bits(got[0][2], got[1][2]) and np.abs(got[0][0]).max() > 0
    assert same_bits(got[0][3], got[1][3]) and np.abs(got[0][3]).max() > 0
    assert got[0][1] is None or same_bits(got[0][1], got[1][1])


# ---- 4. in-place updates, prune, rewire: bit-equal to a fresh plan ---------------------------------------------------------
def _fresh_equals(pkg, synth, dev, s, sk, plan, step, **opts):
    """Forward and data gradient of `plan` equal, bit for bit, those of a fresh s2b plan aligned by set_csr on its CSR."""
    xd, bd_, tdd = _up(sk.x, dev), _up(sk.b, dev), _up(sk.top_diff, dev)
    rp, ci, vals, ng = plan.get_csr()               # (brings the host values up to date)
    fresh = pkg.Plan(pkg.ConvDesc.from_shape(s), s2b=1, **opts)
    fresh.set_csr(rp, ci, vals, ng)
    out = []
    for p in (plan, fresh):
        top = p.forward(xd, bd_)
        bd, _, _ = p.backward(tdd, bottom_diff=_nan_like(s, dev))
        torch.cuda.synchronize()
        assert p.stat("s2b") == 1
        out.append((top.cpu().numpy(), bd.cpu().numpy()))
    assert plan.kernel_name == fresh.kernel_name and plan.stat("bwd_data_kernel") == fresh.stat("bwd_data_kernel")
    fresh.close()
    assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1]), (s.name, step)
    assert np.all(np.isfinite(out[0][0])) and np.all(np.isfinite(out[0][1])), (s.name, step)
    return out[0]


@pytest.mark.parametrize("kernel", ["AUTO", "DENSE"])
@pytest.mark.parametrize("name", ["3x3_d2x3_g2", "res_like"])
def test_updates_reach_the_inner_plan_in_place(pkg, synth, dev, name, kernel):
    """set_values before the backward state exists, then set_values, update_values and one solver step after it: each
    in place (update_fast == 1), each equal to a fresh plan on the new values, and get_csr returns them."""
    s, sk = _case(synth, make(synth, name))
    opts = {} if kernel == "AUTO" else dict(kernel=pkg.KERNEL_DENSE)
    plan = _plan(pkg, s, sk.w, **opts)
    nnz = plan.nnz()
    assert nnz > 0
    w1, _ = new_weights(sk.w, 41)
    v1 = values_at(plan, w1)[2]
    plan.set_values(_up(v1, dev))                       # before the backward state exists
    assert plan.stat("update_fast") == 1 and plan.stat("s2b") == 1
    before = plan.stat("update_destinations")
    assert before >= 2 * nnz                            # the value array and the inner plan's copies
    assert same_bits(plan.get_csr()[2], v1)
    g0 = _fresh_equals(pkg, synth, dev, s, sk, plan, "set_values before the first backward", **opts)
    w2, _ = new_weights(sk.w, 42)
    v2 = values_at(plan, w2)[2]
    plan.set_values(_up(v2, dev))
    assert plan.stat("update_fast") == 1
    assert plan.stat("update_destinations") > before    # the inner backward state's copies joined the list
    assert same_bits(plan.get_csr()[2], v2)
    g1 = _fresh_equals(pkg, synth, dev, s, sk, plan, "set_values", **opts)
    assert not np.array_equal(g0[0], g1[0]) and not np.array_equal(g0[1], g1[1])
    w3, w3_nan = new_weights(sk.w, 43)
    plan.update_values(_up(w3_nan, dev))                # device source, NaN outside the pattern
    assert plan.stat("update_fast") == 1
    g2 = _fresh_equals(pkg, synth, dev, s, sk, plan, "update_values", **opts)
    assert not np.array_equal(g1[1], g2[1])
    after = plan.stat("update_destinations")
    vd, h = _up(seeded((nnz,), 44), dev), torch.zeros(nnz, device=dev)
    plan.solver_step(vd, h, type="sgd", rate=0.05, momentum=0.9)
    assert plan.stat("update_fast") == 1 and plan.stat("update_destinations") == after
    g3 = _fresh_equals(pkg, synth, dev, s, sk, plan, "solver_step", **opts)
    assert not np.array_equal(g2[0], g3[0]) and not np.array_equal(g2[1], g3[1])
    plan.set_values(v1)                                 # host source
    assert plan.stat("update_fast") == 1 and same_bits(plan.get_csr()[2], v1)
    g4 = _fresh_equals(pkg, synth, dev, s, sk, plan, "set_values from the host", **opts)
    assert same_bits(g4[0], g0[0]) and same_bits(g4[1], g0[1])
    plan.close()


@pytest.mark.parametrize("bk", ["GENERIC", "BWD_MFMA"])
def test_updates_reach_an_outer_backward_copy_and_the_inner_plan(pkg, synth, dev, bk):
    """The data gradient stays with the outer plan (the gather kernel's value array, the MFMA kernel's phase matrices):
    one update list then holds that array and the inner plan's forward copies, and a set_values from the device after the
    first backward reaches both in place."""
    s, sk = _case(synth, make(synth, "3x3_d2x3_g2"))
    code = pkg.KERNEL_GENERIC if bk == "GENERIC" else pkg.BWD_MFMA
    plan = _plan(pkg, s, sk.w, backward_kernel=code)
    plan.set_values(_up(values_at(plan, new_weights(sk.w, 41)[0])[2], dev))     # before the backward state exists
    assert plan.stat("update_fast") == 1 and plan.stat("s2b") == 1
    before = plan.stat("update_destinations")
    plan.backward(_up(sk.top_diff, dev), bottom_diff=_nan_like(s, dev))
    assert plan.stat("bwd_data_kernel") == code
    v2 = values_at(plan, new_weights(sk.w, 42)[0])[2]
    plan.set_values(_up(v2, dev))
    assert plan.stat("update_fast") == 1
    assert plan.stat("update_destinations") > before    # the outer backward state's array joined the list
    assert same_bits(plan.get_csr()[2], v2)
    _fresh_equals(pkg, synth, dev, s, sk, plan, "set_values after the outer backward", backward_kernel=code)
    plan.close()


def test_a_pruned_and_a_rewired_plan_equal_fresh_plans(pkg, synth, dev):
    s, sk = _case(synth, make(synth, "3x3_d2x3_g2"))
    plan = _plan(pkg, s, sk.w)
    xd, tdd = _up(sk.x, dev), _up(sk.top_diff, dev)
    plan.forward(xd)
    plan.backward(tdd)                                  # (the states a prune has to drop exist)
    n = plan.nnz()
    entry_map = plan.prune(keep=n - n // 3)
    assert plan.nnz() == n - n // 3 and int((entry_map >= 0).sum()) == plan.nnz()
    assert plan.stat("s2b") == 1
    _fresh_equals(pkg, synth, dev, s, sk, plan, "prune")
    D = s.M * (s.C // s.group) * s.KH * s.KW
    score = _up(seeded((D,), 51), dev)
    n1 = plan.nnz()
    plan.rewire(n // 4, score, drop_keep=n1 - n // 8)
    assert plan.nnz() == n1 - n // 8 + n // 4 and plan.stat("s2b") == 1
    _fresh_equals(pkg, synth, dev, s, sk, plan, "rewire")
    plan.set_values(_up(seeded((plan.nnz(),), 52), dev))     # grown zeros become weights, in place
    assert plan.stat("update_fast") == 1
    _fresh_equals(pkg, synth, dev, s, sk, plan, "set_values after rewire")
    plan.close()


# ---- 5. the persisted form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["3x3_d2", "res_like"])
def test_export_then_import_round_trips(pkg, synth, dev, name):
    """export_aligned writes the outer CSR and no code section; import_aligned on an s2b plan aligns from it."""
    s, sk = _case(synth, make(synth, name))
    xd, bd_, tdd = _up(sk.x, dev), _up(sk.b, dev), _up(sk.top_diff, dev)
    plan = _plan(pkg, s, sk.w)
    plain = _plan(pkg, s, sk.w, kernel=pkg.KERNEL_GENERIC, s2b=0)
    blob = plan.export_aligned()
    assert blob.size == plain.export_aligned().size     # CSR only
    plain.close()
    other = pkg.Plan(pkg.ConvDesc.from_shape(s), s2b=1)
    assert other.import_aligned(blob) is False
    out = []
    for p in (plan, other):
        top = p.forward(xd, bd_)
        bd, _, _ = p.backward(tdd, bottom_diff=_nan_like(s, dev))
        torch.cuda.synchronize()
        assert p.stat("s2b") == 1
        out.append((top.cpu().numpy(), bd.cpu().numpy()))
    assert plan.kernel_name == other.kernel_name
    assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1]) and np.abs(out[0][0]).max() > 0
    assert all(same_bits(a, b) for a, b in zip(plan.get_csr(), other.get_csr()))
    plan.close(), other.close()


# ---- 6. a captured training step -----------------------------------------------------------------------------------------------
def test_forward_backward_and_solver_step_captured_into_one_graph(pkg, synth, dev):
    """After one uncaptured pass, forward + backward + solver step captured into one graph and replayed twice on new data:
    nothing is allocated, and each replay equals the same step run eagerly on a twin plan, bit for bit."""
    s = make(synth, "res_like")
    w, b = synth.pruned_weights(s, 11), synth.bias_vector(s, 13)
    oh, ow = synth.out_hw(s)

    def state():
        plan = _plan(pkg, s, w, relu=True)
        nnz = plan.nnz()
        u = dict(x=torch.zeros((s.N, s.C, s.H, s.W), device=dev), td=torch.zeros((s.N, s.M, oh, ow), device=dev),
                 y=torch.zeros((s.N, s.M, oh, ow), device=dev), bd=torch.zeros((s.N, s.C, s.H, s.W), device=dev), b=_up(b, dev),
                 vd=torch.zeros(nnz, device=dev), h=torch.zeros(nnz, device=dev))
        return plan, u

    def step(plan, u):
        plan.forward(u["x"], u["b"], u["y"])
        u["vd"].zero_()
        plan.backward(u["td"], bottom=u["x"], top=u["y"], bottom_diff=u["bd"], values_diff=u["vd"])
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
            step(p, q)              # the first pass builds the backward and update states outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert plan.stat("s2b") == 1 and plan.stat("update_fast") == 1
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
        for k in ("y", "bd", "vd", "h"):
            assert same_bits(u[k].cpu().numpy(), v[k].cpu().numpy()), (k, rnd)
        assert np.all(np.isfinite(u["bd"].cpu().numpy())) and float(u["bd"].abs().max()) > 0
    assert plan.workspace_bytes == ws1 == twin.workspace_bytes
    assert same_bits(plan.get_csr()[2], twin.get_csr()[2])
    plan.close(), twin.close()


# ---- 7. where the option changes nothing ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(UNSERVED))
def test_unserved_layers_run_as_without_the_option(pkg, synth, dev, name):
    s, sk = _case(synth, make(synth, name))
    xd, bd_, tdd = _up(sk.x, dev), _up(sk.b, dev), _up(sk.top_diff, dev)
    out, names = [], []
    for s2b in (1, 0):
        plan = _plan(pkg, s, sk.w, s2b=s2b)
        top = plan.forward(xd, bd_)
        bd, _, _ = plan.backward(tdd, bottom_diff=_nan_like(s, dev))
        torch.cuda.synchronize()
        assert plan.stat("s2b") == 0 and plan.stat("s2b_scratch_bytes") == 0
        out.append((top.cpu().numpy(), bd.cpu().numpy(), plan.workspace_bytes))
        names.append((plan.kernel_name, plan.stat("kernel_choice"), plan.stat("bwd_data_kernel"), plan.tiling_info))
        plan.close()
    assert names[0] == names[1]
    assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1]) and out[0][2] == out[1][2]


def test_a_double_plan_and_the_lowered_modes_run_on_the_original_geometry(pkg, synth, dev):
    s, sk = _case(synth, make(synth, "3x3_d2"))
    want, B = _fwd_bound(s, sk, False)
    xd, bd_ = _up(sk.x, dev), _up(sk.b, dev)
    ref = _plan(pkg, s, sk.w.astype(np.float64), s2b=0)
    plan = _plan(pkg, s, sk.w.astype(np.float64))
    assert plan.stat("s2b") == 0 and plan.kernel_name == ref.kernel_name
    x64, b64 = _up(sk.x, dev, np.float64), _up(sk.b, dev, np.float64)
    assert same_bits(plan.forward(x64, b64).cpu().numpy(), ref.forward(x64, b64).cpu().numpy())
    plan.close(), ref.close()
    for mode in (pkg.CONV_MODE_LOWERED_GEMM, pkg.CONV_MODE_LOWERED_SPARSE):
        ref = _plan(pkg, s, sk.w, s2b=0, conv_mode=mode)
        plan = _plan(pkg, s, sk.w, conv_mode=mode)
        assert plan.stat("s2b") == 0 and plan.kernel_name == ref.kernel_name
        a, b = plan.forward(xd, bd_).cpu().numpy(), ref.forward(xd, bd_).cpu().numpy()
        assert same_bits(a, b)
        ref.close()
        # a flip to the direct mode rebuilds the plan with the option, and back without it
        plan.set_option("conv_mode", pkg.CONV_MODE_SCONV_PAR)
        assert plan.stat("s2b") == 1 and plan.kernel_name.startswith(PACK) and plan.kernel_name.endswith(UNPACK)
        eb.within(plan.forward(xd, bd_).cpu().numpy(), want, B, plan.kernel_name, sk.row_exp, what=(s.name, "flipped", mode))
        plan.set_option("conv_mode", mode)
        assert plan.stat("s2b") == 0
        assert same_bits(plan.forward(xd, bd_).cpu().numpy(), b)
        plan.close()


# ---- 8. the measurement hook and the tool -----------------------------------------------------------------------------------------
def test_pack_and_unpack_alone_run_on_an_s2b_plan_only(pkg, synth, dev):
    s, sk = _case(synth, make(synth, "3x3_d2"))
    xd, bd_ = _up(sk.x, dev), _up(sk.b, dev)
    oh, ow = synth.out_hw(s)
    plan = _plan(pkg, s, sk.w)
    before = plan.forward(xd, bd_).cpu().numpy()
    ws = plan.workspace_bytes
    # the unpack alone interleaves what the forward left in T': the same top again
    again = torch.full((s.N, s.M, oh, ow), float("nan"), device=dev)
    plan.s2b_unpack(again)
    assert same_bits(again.cpu().numpy(), before)
    part = torch.full((s.N, s.M, oh, ow), float("nan"), device=dev)
    plan.s2b_unpack(part[:1])
    assert same_bits(part[:1].cpu().numpy(), before[:1]) and np.all(np.isnan(part[1:].cpu().numpy()))
    plan.s2b_pack(_up(np.full_like(sk.x, np.nan), dev))         # the scratch is overwritten by the next forward's own pack
    after = plan.forward(xd, bd_).cpu().numpy()
    assert plan.stat("s2b") == 1 and plan.workspace_bytes == ws and same_bits(before, after)
    plan.close()
    for name in ("3x3_d2", "3x3_d1"):                           # the option off, and on an unserved layer
        s2, sk2 = _case(synth, make(synth, name))
        plan = _plan(pkg, s2, sk2.w, s2b=int(name == "3x3_d1"))
        assert plan.stat("s2b") == 0
        top = torch.zeros((s2.N, s2.M) + tuple(synth.out_hw(s2)), device=dev)
        for call, arg in ((plan.s2b_pack, _up(sk2.x, dev)), (plan.s2b_unpack, top)):
            with pytest.raises(pkg.EscoinError) as e:
                call(arg)
            assert "failed (-4)" in str(e.value)                    # ESCOIN_ESTATE
        plan.close()


def test_dilated_bench_runs_at_a_small_batch(tmp_path):
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    md = str(tmp_path / "s2b.md")
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "dilated_bench.py"), "--batch", "2", "--tiny", "--only", "res4,fc6",
                          "--regions", "5", "--reps", "1", "--markdown", md], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr.decode()
    res = json.loads(out.stdout.decode().strip().splitlines()[-1])
    rows = res["layers"]
    assert [r["layer"] for r in rows] == ["tiny_res4_d2", "tiny_fc6_d12"] and res["batches"] == [2]
    for row in rows:
        assert row["N"] == 2 and row["forward"]["s2b"]["kernel"].startswith(PACK) and row["forward"]["s2b"]["kernel"].endswith(UNPACK)
        assert set(row["forward"]) == set(row["backward"]) == {"s2b", "generic", "dense", "auto"}
        for k in ("pack", "unpack", "pack_copy", "unpack_copy"):
            assert row[k]["median_us"] > 0
    # 3x3_d2-sized: 8 -> 8 channels, 9x9, pad 2: X' = 2 * 4 * 8 * 7 * 7 floats, the top 2 * 8 * 9 * 9
    assert rows[0]["pack"]["dst_bytes"] == 4 * 2 * 4 * 8 * 7 * 7 and rows[0]["unpack"]["dst_bytes"] == 4 * 2 * 8 * 9 * 9
    text = open(md).read()
    assert "pack GB/s" in text and "unpack GB/s" in text
