"""Plan option "deconv" on the MI355X: Deconvolution layers through a stride-1 inner plan, escoin_d2s_unpack_kernel and
escoin_d2s_pack_kernel.  Every shape of d2s_common.SHAPES with the inner kernel AUTO, JIT, TILED, DENSE and GENERIC, with and
without bias and ReLU, on the whole batch and on a partial one, forward and the three gradients held per element to
errbound.py's bound evaluated on the inner stride-1 layer (d2s_common.forward_bound / backward_bound); tiling_batch 256; the
GENERIC forward array-equal to the CPU mode; every backward and weight-gradient kernel the inner plan accepts; guard bands and
images past n_images; the two kernels alone against their numpy restatement; in-place updates and a captured training step
against fresh plans, bit for bit; the stats, the kernel name and the refusals."""
import numpy as np
import pytest

import d2s_common as dc
import errbound as eb
from upd_common import same_bits
from wgrad_common import tiled_ok

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
UNPACK = " + escoin_d2s_unpack_kernel"
GUARD = 257
KERNELS = ["AUTO", "JIT", "TILED", "DENSE", "GENERIC"]
COMBOS = [(True, False), (False, False), (True, True), (False, True)]      # (bias, relu)
SKIPPED = set()      # (shape, kernel) pairs whose forced tiled kernel the inner geometry does not have


@pytest.fixture(scope="module")
def dev(pkg):
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        pytest.fail("no HIP device visible (these tests run on the MI355X)")
    return torch.device("cuda:0")


_CASES = {}


def _case(name):
    """(shape, weights, inputs) of a shape: made once, never written."""
    if name not in _CASES:
        s = dc.make(name)
        _CASES[name] = (s, dc.weights(s)) + dc.inputs(s)
    return _CASES[name]


_BOUNDS = {}


def _fwd_bound(synth, name, bias, relu, n):
    key = ("f", name, bias, relu, n)
    if key not in _BOUNDS:
        s, w, x, b, _ = _case(name)
        _BOUNDS[key] = dc.forward_bound(eb, synth, s, w, x[:n], b if bias else None, relu)
    return _BOUNDS[key]


def _up(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def _guarded(shape, dev, fill):
    """A blob of `shape` inside a larger allocation filled with `fill`: (the whole buffer, the blob's view)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, device=dev)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _guards_kept(buf, n, fill):
    g = torch.cat([buf[:GUARD], buf[GUARD + n:]]).cpu().numpy()
    return bool(np.all(g == fill))


def _plan(pkg, s, w, bias=True, relu=False, **opts):
    plan = pkg.Plan(dc.desc(pkg, s, bias, relu), deconv=1, **opts)
    plan.weight_align(w)
    return plan


def _active(plan, s):
    P, _, _, hi, wi = dc.inner_dims(s)
    assert plan.stat("deconv") == 1
    assert plan.stat("deconv_scratch_bytes") == 4 * s.N * s.M * P * hi * wi
    assert plan.kernel_name.endswith(UNPACK) and len(plan.kernel_name) > len(UNPACK)
    assert plan.stat("device_bytes") > plan.stat("deconv_scratch_bytes")
    assert plan.workspace_bytes == (plan.stat("device_bytes") + plan.stat("bwd_device_bytes") + plan.stat("upd_device_bytes") +
                                    plan.stat("dwg_device_bytes"))


def _check(pkg, synth, dev, name, bias, relu, n=None, **opts):
    """Forward and the three gradients of the first n images of one layer: every element within the bound of the float64
    reference; the blobs' guard bands and the images at or past n keep their fill."""
    s, w, x, b, td = _case(name)
    n = s.N if n is None else n
    b = b if bias else None
    oh, ow = dc.out_hw(s)
    plan = _plan(pkg, s, w, bias, relu, **opts)
    _active(plan, s)
    what = (name, "bias", bias, "relu", relu, "n", n, plan.kernel_name)
    want, B = _fwd_bound(synth, name, bias, relu, n)
    tbuf, top = _guarded((s.N, s.M, oh, ow), dev, 7.0)
    xd, bd_, tdd = _up(x, dev), _up(b, dev), _up(td, dev)
    plan.forward(xd[:n], bd_, top[:n])
    torch.cuda.synchronize()
    top_np = top.cpu().numpy()
    assert _guards_kept(tbuf, top.numel(), 7.0) and np.all(top_np[n:] == 7.0), what
    rf = eb.within(top_np[:n], want, B, plan.kernel_name, what=what)
    tp = top_np[:n] if relu else None
    wantb, Bs = dc.backward_bound(eb, synth, s, w, x[:n], td[:n], tp)
    dbuf, bdiff = _guarded((s.N, s.C, s.H, s.W), dev, -3.0)
    got = plan.backward(tdd[:n], bottom=xd[:n], top=top[:n] if relu else None, bottom_diff=bdiff[:n], weight_diff=True, bias_diff=True)
    torch.cuda.synchronize()
    bd_np = bdiff.cpu().numpy()
    assert _guards_kept(dbuf, bdiff.numel(), -3.0) and np.all(bd_np[n:] == -3.0), what
    rb = [eb.within(g, wn, Bn, plan.kernel_name, what=what + (k,)) for g, wn, Bn, k in
          zip((bd_np[:n], got[1].cpu().numpy(), got[2].cpu().numpy()), wantb, Bs, ("bottom_diff", "weight_diff", "bias_diff"))]
    assert not got[1].cpu().numpy()[w == 0].any(), what
    _active(plan, s)
    print("errbound deconv %-15s bias=%d relu=%d n=%d %-70s forward %.3g, gradients %s" %
          (name, bias, relu, n, plan.kernel_name, rf, " ".join("%.3g" % r for r in rb)))
    plan.close()


# ---- 1. every shape, every inner kernel, against the float64 reference ---------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", list(dc.SHAPES))
def test_every_element_within_the_float64_error_bound(pkg, synth, dev, name, kernel):
    s = dc.make(name)
    opts = {} if kernel == "AUTO" else dict(kernel=getattr(pkg, "KERNEL_" + kernel))
    if kernel in ("JIT", "TILED") and not tiled_ok(dc.inner_shape(synth, s)):
        # the inner geometry has no tiled kernel: the align refuses, naming it
        with pytest.raises(pkg.EscoinError) as e:
            _plan(pkg, s, _case(name)[1], **opts)
        assert "failed (-1)" in str(e.value)
        SKIPPED.add((name, kernel))
        return
    for bias, relu in COMBOS:
        _check(pkg, synth, dev, name, bias, relu, **opts)
        if s.N > 1:
            _check(pkg, synth, dev, name, bias, relu, n=s.N - 1, **opts)
    if kernel != "AUTO":
        plan = _plan(pkg, s, _case(name)[1], **opts)
        assert plan.stat("kernel_choice") == opts["kernel"], plan.kernel_name
        plan.close()


def test_only_the_wide_shape_was_refused_a_tiled_kernel(pkg, synth):
    """A blanket refusal cannot pass: of all (shape, forced kernel) pairs only the inner layers wider than 256 or with KW' > 5
    have no tiled kernel."""
    for name in dc.SHAPES:
        s = dc.make(name)
        fits = tiled_ok(dc.inner_shape(synth, s))
        assert fits == (name != "wide" and dc.inner_dims(s)[2] <= 5), name
    assert SKIPPED <= {("wide", "JIT"), ("wide", "TILED")}, SKIPPED


@pytest.mark.parametrize("name", ["k4s2p1", "k5s3p2_g2", "k2s2"])
def test_under_tiling_batch_256(pkg, synth, dev, name):
    s = dc.make(name)
    for bias, relu in ((True, True), (False, False)):
        _check(pkg, synth, dev, name, bias, relu, tiling_batch=256)
        _check(pkg, synth, dev, name, bias, relu, n=s.N - 1, tiling_batch=256)


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("name", list(dc.SHAPES))
def test_the_generic_kernel_inside_equals_the_cpu_mode(pkg, dev, name, relu):
    s, w, x, b, _ = _case(name)
    plan = _plan(pkg, s, w, True, relu, kernel=pkg.KERNEL_GENERIC)
    got = plan.forward(_up(x, dev), _up(b, dev)).cpu().numpy()
    host = pkg.Plan(dc.desc(pkg, s, True, relu), deconv=1)
    host.weight_align_cpu(w)
    assert np.array_equal(got, host.forward_cpu(x, b)), name
    assert np.array_equal(got, plan.forward_cpu(x, b)), name                       # (the device plan's own host side)
    plan.close(), host.close()


# ---- 2. the two kernels alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k4s2p1", "k3x2_s2x3", "k2s2p2", "k5s3p2_g2", "wide"])
def test_pack_and_unpack_alone_follow_their_rule(pkg, dev, name):
    s, w, x, b, td = _case(name)
    P, _, _, hi, wi = dc.inner_dims(s)
    rs = np.random.RandomState(3)
    t = rs.uniform(-1, 1, (s.N, s.M * P, hi, wi)).astype(np.float32)
    for relu in (False, True):
        plan = _plan(pkg, s, w, True, relu)
        for bias in (b, None):
            tbuf, top = _guarded((s.N, s.M) + dc.out_hw(s), dev, 5.0)
            plan.d2s_unpack(top, _up(bias, dev), _up(t, dev))
            torch.cuda.synchronize()
            assert same_bits(top.cpu().numpy(), dc.unpack(s, t, bias, relu)) and _guards_kept(tbuf, top.numel(), 5.0)
        n = max(1, s.N - 1)
        gbuf, g = _guarded((s.N, s.M * P, hi, wi), dev, 5.0)
        topv = rs.uniform(-1, 1, td.shape).astype(np.float32)
        tdn = td.copy()
        # a masked NaN becomes +0 -- select, not multiply -- under every masking top: 0, -0.0, a negative and NaN, each set
        # BEFORE top_diff is poisoned there, in the first image's first row, its second row and its last element; without
        # the mask the NaN passes through with its bits
        oh, ow = dc.out_hw(s)
        spots = [(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0), (0, s.M - 1, oh - 1, ow - 1)]
        for spot, value in zip(spots, (0.0, -0.0, -1.0, np.nan)):
            topv[spot] = value
            tdn[spot] = np.nan
        plan.d2s_pack(_up(tdn, dev), _up(topv, dev) if relu else None, g, n_images=n)
        torch.cuda.synchronize()
        g_np = g.cpu().numpy()
        assert same_bits(g_np[:n], dc.pack(s, tdn[:n], topv[:n] if relu else None)), (name, relu)
        assert int(np.isnan(g_np[:n]).sum()) == (0 if relu else len(spots)), (name, relu)
        assert np.all(g_np[n:] == 5.0) and _guards_kept(gbuf, g.numel(), 5.0)
        plan.close()


# ---- 3. the backward's kernels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k4s2p1", "k5s3p2_g2"])
def test_every_backward_and_weight_gradient_kernel_or_a_refusal(pkg, synth, dev, name):
    s, w, x, b, td = _case(name)
    wantb, Bs = dc.backward_bound(eb, synth, s, w, x, td)
    xd, tdd = _up(x, dev), _up(td, dev)
    ran = []
    for bk in ("KERNEL_AUTO", "KERNEL_GENERIC", "KERNEL_TILED", "KERNEL_JIT", "KERNEL_DENSE", "BWD_MFMA"):
        for wk in ("WGRAD_AUTO", "WGRAD_ENTRY", "WGRAD_STAGED", "WGRAD_MFMA"):
            plan = _plan(pkg, s, w, backward_kernel=getattr(pkg, bk), wgrad_kernel=getattr(pkg, wk))
            try:
                got = plan.backward(tdd, bottom=xd, weight_diff=True, bias_diff=True)
            except pkg.EscoinError as e:
                assert "failed (-1)" in str(e) and ("backward_kernel" in str(e) or "wgrad_kernel" in str(e)), str(e)
                plan.close()
                continue
            torch.cuda.synchronize()
            for g, wn, Bn, k in zip(got, wantb, Bs, ("bottom_diff", "weight_diff", "bias_diff")):
                eb.within(g.cpu().numpy(), wn, Bn, "%s/%s" % (bk, wk), what=(name, k))
            _, vd, _ = plan.backward(tdd, bottom=xd, bottom_diff=None, values_diff=True)
            assert same_bits(vd.cpu().numpy(), got[1].cpu().numpy().reshape(-1)[np.flatnonzero(w.reshape(-1))])
            ran.append((bk, wk, plan.stat("bwd_data_kernel"), plan.stat("wgrad_kernel")))
            plan.close()
    print(name, "backward kernels that ran:", ran)
    # a blanket refusal cannot pass: the gather kernel and the entry kernel serve every float plan, and the inner layer
    # (stride 1, pad K' - 1) has a transposed plan for AUTO to pick
    assert {(bk, wk) for bk, wk, _, _ in ran} >= {(bk, wk) for bk in ("KERNEL_AUTO", "KERNEL_GENERIC") for wk in ("WGRAD_AUTO", "WGRAD_ENTRY")}


def test_gradients_accumulate_and_are_deterministic(pkg, dev):
    s, w, x, b, td = _case("k3s2p1")
    plan = _plan(pkg, s, w)
    xd, tdd = _up(x, dev), _up(td, dev)
    bd, wd, bsd = plan.backward(tdd, bottom=xd, weight_diff=True, bias_diff=True)
    pre_w, pre_b = torch.full(w.shape, 3.0, device=dev), torch.full((s.M,), -2.0, device=dev)
    bd2, wd2, bsd2 = plan.backward(tdd, bottom=xd, bottom_diff=torch.full(x.shape, float("nan"), device=dev), weight_diff=pre_w, bias_diff=pre_b)
    torch.cuda.synchronize()
    assert same_bits(bd2.cpu().numpy(), bd.cpu().numpy())
    wd_np, wd2_np = wd.cpu().numpy(), wd2.cpu().numpy()
    assert np.all(wd2_np[w == 0] == 3.0) and np.array_equal(wd2_np[w != 0], (np.float32(3.0) + wd_np)[w != 0])
    assert np.array_equal(bsd2.cpu().numpy(), np.float32(-2.0) + bsd.cpu().numpy())
    plan.close()


# ---- 4. updates in place ------------------------------------------------------------------------------------------------------
def _fresh_equals(pkg, dev, s, plan, x, b, td, what, **opts):
    """Forward and the gradients of `plan` equal those of a fresh plan aligned on its current CSR, bit for bit."""
    rp, ci, vals, ng = plan.get_csr()
    fresh = pkg.Plan(dc.desc(pkg, s), deconv=1, **opts)
    fresh.set_csr(rp, ci, vals, ng)
    out = []
    for p in (plan, fresh):
        top = p.forward(_up(x, dev), _up(b, dev))
        bd, vd, _ = p.backward(_up(td, dev), bottom=_up(x, dev), values_diff=True)
        torch.cuda.synchronize()
        out.append((top.cpu().numpy(), bd.cpu().numpy(), vd.cpu().numpy()))
    fresh.close()
    for a, c in zip(*out):
        assert same_bits(a, c) and np.all(np.isfinite(a)), what
    return out[0]


@pytest.mark.parametrize("kernel", ["AUTO", "DENSE", "GENERIC"])
@pytest.mark.parametrize("name", ["k4s2p1", "k5s3p2_g2"])
def test_updates_reach_the_inner_plan_in_place(pkg, dev, name, kernel):
    s, w, x, b, td = _case(name)
    opts = {} if kernel == "AUTO" else dict(kernel=getattr(pkg, "KERNEL_" + kernel))
    plan = _plan(pkg, s, w, **opts)
    nnz = plan.nnz()
    rs = np.random.RandomState(41)
    v1 = rs.uniform(-1, 1, nnz).astype(np.float32)
    plan.set_values(_up(v1, dev))                       # before the inner backward state exists
    assert plan.stat("update_fast") == 1 and plan.stat("deconv") == 1
    before = plan.stat("update_destinations")
    assert before >= 2 * nnz                            # the value array and the inner plan's copies
    assert same_bits(plan.get_csr()[2], v1)
    g0 = _fresh_equals(pkg, dev, s, plan, x, b, td, "set_values before the first backward", **opts)
    v2 = rs.uniform(-1, 1, nnz).astype(np.float32)
    plan.set_values(_up(v2, dev))
    assert plan.stat("update_fast") == 1 and plan.stat("update_destinations") > before     # the inner backward state's copies joined
    g1 = _fresh_equals(pkg, dev, s, plan, x, b, td, "set_values", **opts)
    assert not np.array_equal(g0[0], g1[0]) and not np.array_equal(g0[1], g1[1])
    w3 = np.where(w != 0, rs.uniform(-1, 1, w.shape), np.nan).astype(np.float32)
    plan.update_values(_up(w3, dev))                    # device source, blobs_[0] in C x Mg x KH x KW, NaN outside the pattern
    assert plan.stat("update_fast") == 1
    assert same_bits(plan.get_csr()[2], w3.reshape(-1)[np.flatnonzero(w.reshape(-1))])
    g2 = _fresh_equals(pkg, dev, s, plan, x, b, td, "update_values", **opts)
    assert not np.array_equal(g1[0], g2[0])
    after = plan.stat("update_destinations")
    vd, h = _up(rs.uniform(-1, 1, nnz), dev), torch.zeros(nnz, device=dev)
    plan.solver_step(vd, h, type="sgd", rate=0.05, momentum=0.9)
    assert plan.stat("update_fast") == 1 and plan.stat("update_destinations") == after
    g3 = _fresh_equals(pkg, dev, s, plan, x, b, td, "solver_step", **opts)
    assert not np.array_equal(g2[0], g3[0])
    plan.set_values(v1)                                 # host source
    g4 = _fresh_equals(pkg, dev, s, plan, x, b, td, "set_values from the host", **opts)
    assert same_bits(g4[0], g0[0]) and same_bits(g4[1], g0[1])
    plan.close()


def test_set_csr_and_export_import_rebuild(pkg, synth, dev):
    s, w, x, b, td = _case("k4s2p1")
    plan = _plan(pkg, s, w)
    rp, ci, vals, ng = plan.get_csr()
    erp, eci, _, eng = dc.csr_of(s, w)
    assert rp.tolist() == erp.tolist() and ci.tolist() == eci.tolist() and ng.tolist() == eng.tolist()
    plan.set_csr(rp, ci, vals * 2, ng)
    want, B = dc.forward_bound(eb, synth, s, w * 2, x, b)
    eb.within(plan.forward(_up(x, dev), _up(b, dev)).cpu().numpy(), want, B, plan.kernel_name, what="set_csr")
    blob = plan.export_aligned()
    other = pkg.Plan(dc.desc(pkg, s), deconv=1)
    assert other.import_aligned(blob) is False          # the outer CSR and no code section
    _active(other, s)
    assert all(same_bits(a, c) for a, c in zip(plan.get_csr(), other.get_csr()))
    assert same_bits(other.forward(_up(x, dev), _up(b, dev)).cpu().numpy(), plan.forward(_up(x, dev), _up(b, dev)).cpu().numpy())
    plan.close(), other.close()


def test_forward_backward_and_update_captured_into_one_graph(pkg, dev):
    """After one uncaptured pass, forward + backward + solver step captured into one graph and replayed three times on new
    data: nothing is allocated, and each replay equals the same step run eagerly on a twin plan, bit for bit."""
    s, w, _, b, _ = _case("k4s2p1")
    oh, ow = dc.out_hw(s)

    def state():
        plan = _plan(pkg, s, w, True, True)
        nnz = plan.nnz()
        u = dict(x=torch.zeros((s.N, s.C, s.H, s.W), device=dev), td=torch.zeros((s.N, s.M, oh, ow), device=dev),
                 y=torch.zeros((s.N, s.M, oh, ow), device=dev), bd=torch.zeros((s.N, s.C, s.H, s.W), device=dev), b=_up(b, dev),
                 vd=torch.zeros(nnz, device=dev), bsd=torch.zeros(s.M, device=dev), h=torch.zeros(nnz, device=dev))
        return plan, u

    def step(plan, u):
        plan.forward(u["x"], u["b"], u["y"])
        u["vd"].zero_(), u["bsd"].zero_()
        plan.backward(u["td"], bottom=u["x"], top=u["y"], bottom_diff=u["bd"], values_diff=u["vd"], bias_diff=u["bsd"])
        plan.solver_step(u["vd"], u["h"], type="sgd", rate=0.01, momentum=0.9)

    def feed(u, rnd):
        rs = np.random.RandomState(900 + rnd)
        u["x"].copy_(torch.from_numpy(rs.uniform(-1, 1, tuple(u["x"].shape)).astype(np.float32)))
        u["td"].copy_(torch.from_numpy(rs.uniform(-1, 1, tuple(u["td"].shape)).astype(np.float32)))
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
    assert plan.stat("deconv") == 1 and plan.stat("update_fast") == 1
    ws1 = plan.workspace_bytes
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(plan, u)
    assert plan.workspace_bytes == ws1
    for rnd in (1, 2, 3):           # (a capture runs nothing: both plans have taken one step so far)
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


# ---- 5. the facts and the refusals ----------------------------------------------------------------------------------------------
def test_stats_and_kernel_name_report_the_inner_plan(pkg, dev):
    s, w, x, b, td = _case("k4s2p1")
    for kernel, inner in ((pkg.KERNEL_GENERIC, "generic"), (pkg.KERNEL_DENSE, "dense")):
        plan = _plan(pkg, s, w, kernel=kernel)
        _active(plan, s)
        assert plan.stat("kernel_choice") == kernel and inner in plan.kernel_name.lower()
        assert plan.stat("s2d") == 0 and plan.stat("s2b") == 0 and plan.stat("b2s") == 0
        plan.backward(_up(td, dev), bottom=_up(x, dev), weight_diff=True)
        assert plan.stat("bwd_device_bytes") > 0 and plan.stat("wgrad_kernel") in (pkg.WGRAD_ENTRY, pkg.WGRAD_STAGED)
        _active(plan, s)
        plan.close()
    plain = pkg.Plan(dc.desc(pkg, s))
    plain.weight_align(np.ones((s.M, s.C, s.KH, s.KW), np.float32))
    assert plain.stat("deconv") == 0 and plain.stat("deconv_scratch_bytes") == 0 and "d2s" not in plain.kernel_name
    plain.close()


def test_refusals_on_the_device(pkg, dev):
    s, w, x, b, td = _case("k3s2p1")
    plan = _plan(pkg, s, w)

    def refused(fn, *words):
        with pytest.raises(pkg.EscoinError) as e:
            fn()
        assert "failed (-1)" in str(e.value) and all(k in str(e.value) for k in words), str(e.value)

    refused(lambda: plan.prune(keep=3), "deconv", "escoin_plan_prune")
    refused(lambda: plan.rewire(1, torch.ones(plan._dense_size(), device=dev)), "deconv", "escoin_plan_rewire")
    refused(lambda: plan.dense_wgrad(_up(td, dev), _up(x, dev)), "deconv", "escoin_dense_wgrad")
    eb_top = plan.forward(_up(x, dev), _up(b, dev))      # the plan still works
    assert np.all(np.isfinite(eb_top.cpu().numpy()))
    plan.close()
    refused(lambda: _plan(pkg, s, w.astype(np.float64)), "deconv", "double")
    for other in ("s2d", "s2b", "b2s"):
        refused(lambda: _plan(pkg, s, w, **{other: 1}), "deconv", other)
    wide = dc.make("wide")
    refused(lambda: _plan(pkg, wide, dc.weights(wide), kernel=pkg.KERNEL_TILED))


def test_the_conv_mode_is_the_inner_plans(pkg, synth, dev):
    """A flip of the conv mode goes to the inner plan, which rebuilds itself; the layer stays a "deconv" plan within the bound
    in every mode, takes updates afterwards, and returns to its bits in the mode it came from."""
    s, w, x, b, td = _case("k4s2p1")
    want, B = dc.forward_bound(eb, synth, s, w, x, b)
    plan = _plan(pkg, s, w)
    xd, bd_ = _up(x, dev), _up(b, dev)
    before = plan.forward(xd, bd_).cpu().numpy()
    for mode in (pkg.CONV_MODE_LOWERED_GEMM, pkg.CONV_MODE_LOWERED_SPARSE, pkg.CONV_MODE_SCONV):
        plan.set_option("conv_mode", mode)
        _active(plan, s)
        eb.within(plan.forward(xd, bd_).cpu().numpy(), want, B, plan.kernel_name, what=("conv_mode", mode))
    plan.set_option("conv_mode", pkg.CONV_MODE_SCONV_PAR)
    assert same_bits(plan.forward(xd, bd_).cpu().numpy(), before)
    plan.set_values(_up(plan.get_csr()[2] * np.float32(2), dev))
    want2, B2 = dc.forward_bound(eb, synth, s, w * 2, x, b)
    eb.within(plan.forward(xd, bd_).cpu().numpy(), want2, B2, plan.kernel_name, what="set_values after the flips")
    plan.close()
    lowered = _plan(pkg, s, w, conv_mode=pkg.CONV_MODE_LOWERED_GEMM)      # the mode set before the align
    _active(lowered, s)
    eb.within(lowered.forward(xd, bd_).cpu().numpy(), want, B, lowered.kernel_name, what="aligned in LOWERED_GEMM")
    lowered.close()
