"""The weight / bias gradient on the MI355X under plan option "wgrad_pointwise" (escoin_sconv_wgrad_pointwise_kernel): the
shapes of wgrad_pointwise_common.py against torch float64 autograd and the per-element bound of errbound.py; the pattern is
all that is written; compact == dense gathered bit for bit; accumulation, partial batches, explicit zeros, a non-finite
bottom; bits that do not depend on how entries are dealt to tiles (the two test options), on the call or on the stream;
plans the rule does not serve and a forced kernel; the "b2s" and "deconv" wrappers; the state's lifetime; a captured
training loop.  Every served case asserts that the pointwise kernel ran (stat "wgrad_kernel" == 4)."""
import numpy as np
import pytest

import b2s_common
import d2s_common as dc
import errbound as eb
import wgrad_pointwise_common as pc
from conftest import rel_err

torch = pytest.importorskip("torch")

from wgrad_common import csr_positions, seeded, torch_backward  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4
CONV = list(pc.CONV)


@pytest.fixture(scope="module")
def dev(pkg):
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        pytest.fail("no HIP device visible (these tests run on the MI355X)")
    return torch.device("cuda:0")


_INPUTS = {}
_REFS = {}


def _inputs(synth, name):
    """(shape, weights, activations, bias, top_diff) of a named shape: made once, never written."""
    if name not in _INPUTS:
        s = pc.make(synth, name)
        oh, ow = synth.out_hw(s)
        w = synth.pruned_weights(s, 11)
        if name == "pw_g3":
            w = pc.emptied(w, s)
        _INPUTS[name] = (s, w, synth.activations(s, 12), synth.bias_vector(s, 13), seeded((s.N, s.M, oh, ow), 21))
    return _INPUTS[name]


def _ref(synth, name, n=None):
    """torch float64 (bottom_diff, weight_diff, bias_diff) of the first n images without ReLU: computed once."""
    if (name, n) not in _REFS:
        s, w, x, b, td = _inputs(synth, name)
        _REFS[(name, n)] = torch_backward(x[:n], w, b, s, td[:n])
    return _REFS[(name, n)]


def _plan(pkg, s, w, relu=False, on=1, **opts):
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu), wgrad_pointwise=on, **opts)
    plan.weight_align(w)
    return plan


def _up(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _ran(pkg, plan):
    assert plan.stat("wgrad_kernel") == pkg.WGRAD_POINTWISE == 4
    assert 0 < plan.stat("wgrad_lds_bytes") <= pc.LDS_BUDGET and plan.stat("wgrad_lds_bytes") % (4 * pc.PITCH) == 0


# ---- 1. correctness --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("name", CONV)
def test_matches_torch_writes_the_pattern_only_and_compact_equals_dense(pkg, dev, synth, name, relu):
    s, w, x, b, td = _inputs(synth, name)
    xt, tdt, bt = _up(x, dev), _up(td, dev), _up(b, dev)
    plan = _plan(pkg, s, w, relu)
    with pytest.raises(pkg.EscoinError):
        plan.stat("wgrad_kernel")               # nothing has run yet
    top = plan.forward(xt, bt) if relu else None
    torch.cuda.synchronize()
    want = torch_backward(x, w, b, s, td, top.cpu().numpy()) if relu else _ref(synth, name)
    pos = csr_positions(plan)
    for with_bias in (True, False):
        what = (name, relu, with_bias)
        # NaN outside the pattern: it must come back NaN -- nothing there is read or written
        fill = torch.from_numpy(np.where(w == 0, np.float32(np.nan), np.float32(0))).to(dev)
        _, wd, bsd = plan.backward(tdt, bottom=xt, top=top, bottom_diff=None, weight_diff=fill,
                                   bias_diff=True if with_bias else None)
        _, vd, bsd2 = plan.backward(tdt, bottom=xt, top=top, bottom_diff=None, values_diff=True,
                                    bias_diff=True if with_bias else None)
        torch.cuda.synchronize()
        _ran(pkg, plan)
        wd, vd = wd.cpu().numpy(), vd.cpu().numpy()
        assert np.all(np.isnan(wd[w == 0])), what
        assert np.all(np.isfinite(wd[w != 0])), what
        wd0 = np.where(w == 0, np.float32(0), wd)
        print(what, "weight_diff rel_err", rel_err(wd0, want[1]),
              "bias_diff rel_err", None if not with_bias else rel_err(bsd.cpu().numpy(), want[2]))
        assert rel_err(wd0, want[1]) <= TOL, what
        if with_bias:
            assert rel_err(bsd.cpu().numpy(), want[2]) <= TOL, what
            assert _bytes(bsd) == _bytes(bsd2), what
        else:
            assert bsd is None and bsd2 is None
        assert vd.shape == (plan.nnz(),) and len(pos) == plan.nnz()
        assert vd.tobytes() == wd.reshape(-1)[pos].tobytes(), what
        assert rel_err(vd, want[1].reshape(-1)[pos]) <= TOL, what
        assert plan.stat("bwd_chunks") == pc.chunks(s, synth), what
    plan.close()


def test_an_empty_pattern_still_gives_the_bias(pkg, dev, synth):
    s, w, x, b, td = _inputs(synth, "pw_g3")
    w0 = np.zeros_like(w)
    plan = _plan(pkg, s, w0)
    fill = torch.full(w.shape, float("nan"), device=dev)
    _, wd, bsd = plan.backward(_up(td, dev), bottom=_up(x, dev), bottom_diff=None, weight_diff=fill, bias_diff=True)
    torch.cuda.synchronize()
    _ran(pkg, plan)
    assert np.all(np.isnan(wd.cpu().numpy()))
    assert rel_err(bsd.cpu().numpy(), _ref(synth, "pw_g3")[2]) <= TOL
    plan.close()


# ---- 2. error bound ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("name", ["pw_straddle", "pw_g3", "pw_s2"])
def test_every_element_within_the_float64_error_bound(pkg, synth, dev, name, relu):
    """Inputs whose rows, channels and images differ in scale by up to 2^48 (errbound.skew): every element of the weight
    and bias gradient within errbound.backward_bound, in dense and in compact form."""
    s = pc.make(synth, name)
    w, x, b = synth.pruned_weights(s, 91), synth.activations(s, 92), synth.bias_vector(s, 93)
    if name == "pw_g3":
        w = pc.emptied(w, s)
    td = seeded((s.N, s.M) + synth.out_hw(s), 94)
    sk = eb.skew(s, w, x, b, 95, top_diff=td)
    xd, bd_, tdd = _up(sk.x, dev), _up(sk.b, dev), _up(sk.top_diff, dev)
    plan = _plan(pkg, s, sk.w, relu, backward_kernel=pkg.KERNEL_GENERIC)
    top_np = topd = None
    if relu:
        topd = plan.forward(xd, bd_)
        torch.cuda.synchronize()
        top_np = topd.cpu().numpy()
    want, Bs = eb.backward_bound(s, sk.w, sk.x, sk.b, sk.top_diff, top_np)
    _, wd, bsd = plan.backward(tdd, bottom=xd, top=topd, bottom_diff=None, weight_diff=True, bias_diff=True)
    _, vd, bsd2 = plan.backward(tdd, bottom=xd, top=topd, bottom_diff=None, values_diff=True, bias_diff=True)
    torch.cuda.synchronize()
    _ran(pkg, plan)
    what = (name, "relu", relu)
    wdn = wd.cpu().numpy()
    r = eb.within(wdn, want[1], Bs[1], "wgrad_pointwise", sk.td_row_exp, axis=0, what=what)
    rb = eb.within(bsd.cpu().numpy(), want[2], Bs[2], "wgrad_pointwise bias", sk.td_row_exp, axis=0, what=what)
    assert np.all(wdn[sk.w == 0] == 0), what
    pos = csr_positions(plan)
    rv = eb.within(vd.cpu().numpy(), want[1].reshape(-1)[pos], Bs[1].reshape(-1)[pos], "wgrad_pointwise compact", what=what)
    eb.within(bsd2.cpu().numpy(), want[2], Bs[2], "wgrad_pointwise compact bias", sk.td_row_exp, axis=0, what=what)
    print("errbound backward weight pointwise %-12s relu=%d: %.3g, bias %.3g, values %.3g" % (name, relu, r, rb, rv))
    assert r <= 1.0 and rb <= 1.0 and rv <= 1.0
    plan.close()


# ---- 3. accumulation, partial batches, explicit zeros, a non-finite bottom ----------------------------------------------
@pytest.mark.parametrize("name", ["pw_straddle", "pw_g3"])
def test_accumulates_into_prefilled_blobs(pkg, dev, synth, name):
    s, w, x, b, td = _inputs(synth, name)
    xt, tdt = _up(x, dev), _up(td, dev)
    want = _ref(synth, name)
    plan = _plan(pkg, s, w)
    pre_w, pre_b = seeded(w.shape, 31), seeded((s.M,), 32)
    pre_v = seeded((plan.nnz(),), 33)
    _, wd, bsd = plan.backward(tdt, bottom=xt, bottom_diff=None, weight_diff=_up(pre_w, dev), bias_diff=_up(pre_b, dev))
    _, vd, _ = plan.backward(tdt, bottom=xt, bottom_diff=None, values_diff=_up(pre_v, dev))
    _, vd0, bs0 = plan.backward(tdt, bottom=xt, bottom_diff=None, values_diff=True, bias_diff=True)
    torch.cuda.synchronize()
    _ran(pkg, plan)
    wd, vd, vd0 = wd.cpu().numpy(), vd.cpu().numpy(), vd0.cpu().numpy()
    pos = csr_positions(plan)
    assert wd[w == 0].tobytes() == pre_w[w == 0].tobytes()          # outside the pattern: the prefill, untouched
    assert rel_err(wd, want[1] + pre_w) <= TOL
    assert rel_err(bsd.cpu().numpy(), want[2] + pre_b) <= TOL
    # one rounded addition of the gradient to the prefill
    assert vd.tobytes() == (pre_v + vd0).tobytes()
    assert wd.reshape(-1)[pos].tobytes() == (pre_w.reshape(-1)[pos] + vd0).tobytes()
    assert bsd.cpu().numpy().tobytes() == (pre_b + bs0.cpu().numpy()).tobytes()
    plan.close()


# 2 x 361 = 722 px ends mid-step (722 = 22 x 32 + 18); 3 x 64 = 192 px of pw_s2
PARTIAL = [("pw_straddle", 1), ("pw_straddle", 2), ("pw_s2", 3), ("pw_g3", 1), ("pw_g3", 3)]


@pytest.mark.parametrize("name,n", PARTIAL, ids=["%s-%d" % p for p in PARTIAL])
def test_partial_batch_is_the_gradient_of_the_first_images(pkg, dev, synth, name, n):
    s, w, x, b, td = _inputs(synth, name)
    assert 0 < n < s.N
    # the images past n hold NaN: they are not read
    x2, td2 = x.copy(), td.copy()
    x2[n:] = np.nan
    td2[n:] = np.nan
    xt, tdt = _up(x2, dev), _up(td2, dev)
    want = _ref(synth, name, n)
    plan = _plan(pkg, s, w)
    _, wd, bsd = plan.backward(tdt[:n], bottom=xt[:n], bottom_diff=None, weight_diff=True, bias_diff=True)
    _, vd, _ = plan.backward(tdt[:n], bottom=xt[:n], bottom_diff=None, values_diff=True)
    torch.cuda.synchronize()
    _ran(pkg, plan)
    wd, vd = wd.cpu().numpy(), vd.cpu().numpy()
    print(name, n, "weight_diff rel_err", rel_err(wd, want[1]), "bias_diff rel_err", rel_err(bsd.cpu().numpy(), want[2]))
    assert rel_err(wd, want[1]) <= TOL and rel_err(bsd.cpu().numpy(), want[2]) <= TOL
    assert np.all(wd[w == 0] == 0)
    assert vd.tobytes() == wd.reshape(-1)[csr_positions(plan)].tobytes()
    assert plan.stat("bwd_chunks") == pc.chunks(s, synth, n)
    plan.close()


def test_explicit_zeros_receive_their_gradient(pkg, dev, synth):
    s, w, x, b, td = _inputs(synth, "pw_straddle")
    ref = _plan(pkg, s, w)
    rp, ci, vals, ng = ref.get_csr()
    _, vd_ref, _ = ref.backward(_up(td, dev), bottom=_up(x, dev), bottom_diff=None, values_diff=True)
    vals = vals.copy()
    vals[::3] = 0.0
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s), wgrad_pointwise=1)
    plan.set_csr(rp, ci, vals, ng)
    assert plan.nnz() == ref.nnz()
    _, vd, _ = plan.backward(_up(td, dev), bottom=_up(x, dev), bottom_diff=None, values_diff=True)
    torch.cuda.synchronize()
    _ran(pkg, plan)
    # the weight gradient does not read the values: the same bits, at the explicit zeros too
    assert _bytes(vd) == _bytes(vd_ref) and np.all(vd.cpu().numpy()[::3] != 0)
    assert rel_err(vd.cpu().numpy(), _ref(synth, "pw_straddle")[1].reshape(-1)[csr_positions(ref)]) <= TOL
    plan.close()
    ref.close()


def test_non_finite_bottom_reaches_only_the_entries_of_its_channel(pkg, dev, synth):
    s, w, x, b, td = _inputs(synth, "pw_straddle")
    c = 7
    x_inf = x.copy()
    x_inf[1, c, 3, 5] = np.inf
    tdt = _up(td, dev)
    plan = _plan(pkg, s, w)
    _, clean, bc_ = plan.backward(tdt, bottom=_up(x, dev), bottom_diff=None, values_diff=True, bias_diff=True)
    _, dirty, bd_ = plan.backward(tdt, bottom=_up(x_inf, dev), bottom_diff=None, values_diff=True, bias_diff=True)
    torch.cuda.synchronize()
    _ran(pkg, plan)
    clean, dirty = clean.cpu().numpy(), dirty.cpu().numpy()
    hit = plan.get_csr()[1] == c
    assert hit.sum() > 0 and (~hit).sum() > 0
    assert not np.any(np.isfinite(dirty[hit]))
    assert dirty[~hit].tobytes() == clean[~hit].tobytes()
    assert _bytes(bc_) == _bytes(bd_)
    plan.close()


# ---- 4. the bits do not depend on the deal ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pw_straddle", "pw_dense", "pw_g3", "pw_s2"])
def test_bits_do_not_depend_on_tiles_lanes_calls_or_streams(pkg, dev, synth, name):
    s, w, x, b, td = _inputs(synth, name)
    xt, tdt = _up(x, dev), _up(td, dev)

    def call(p):
        return p.backward(tdt, bottom=xt, bottom_diff=None, values_diff=True, bias_diff=True)
    got, lds = {}, {}
    for block in pc.CHANNEL_BLOCKS:
        for te in pc.TILE_ENTRIES:
            plan = _plan(pkg, s, w, wgrad_channel_block=block, wgrad_pointwise_tile_entries=te)
            ws0 = plan.workspace_bytes
            r1 = call(plan)
            ws1 = plan.workspace_bytes
            assert ws1 > ws0 and plan.stat("bwd_device_bytes") >= 8 * plan.nnz()        # the item tables alone
            assert ws1 == plan.stat("device_bytes") + plan.stat("bwd_device_bytes") + plan.stat("upd_device_bytes")
            r2 = call(plan)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                r3 = call(plan)
            _, _, alone = plan.backward(tdt, bottom_diff=None, bias_diff=True)          # the bias alone: no bottom at all
            torch.cuda.synchronize()
            assert plan.workspace_bytes == ws1
            _ran(pkg, plan)
            lds[(block, te)] = plan.stat("wgrad_lds_bytes")
            for a, c, e in zip(r1[1:], r2[1:], r3[1:]):
                assert _bytes(a) == _bytes(c) == _bytes(e), (name, block, te)
            assert _bytes(alone) == _bytes(r1[2]), (name, block, te)
            got[(block, te)] = (_bytes(r1[1]), _bytes(r1[2]))
            plan.close()
    assert len(set(got.values())) == 1, name
    assert len(set(lds.values())) > 1, name              # ... though the tilings differ
    if name == "pw_dense":
        # 1083 products per entry in two different orders: identical weight bits would mean the kernel did not run
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s), wgrad_kernel=pkg.WGRAD_ENTRY)
        plan.weight_align(w)
        r = call(plan)
        torch.cuda.synchronize()
        assert plan.stat("wgrad_kernel") == pkg.WGRAD_ENTRY
        assert _bytes(r[1]) != got[(0, 0)][0]
        assert rel_err(r[1].cpu().numpy(), np.frombuffer(got[(0, 0)][0], np.float32)) <= TOL
        plan.close()


# ---- 5. not served, or overridden ---------------------------------------------------------------------------------------------
def _both(pkg, dev, s, w, x, td, dt=np.float32, **opts):
    out = []
    for on in (0, 1):
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s), wgrad_pointwise=on, **opts)
        plan.weight_align(w.astype(dt))
        xt, tdt = torch.from_numpy(x.astype(dt)).to(dev), torch.from_numpy(td.astype(dt)).to(dev)
        _, wd, bsd = plan.backward(tdt, bottom=xt, bottom_diff=None, weight_diff=True, bias_diff=True)
        torch.cuda.synchronize()
        out.append((plan.stat("wgrad_kernel"), plan.stat("wgrad_lds_bytes"), _bytes(wd), _bytes(bsd)))
        plan.close()
    return out


@pytest.mark.parametrize("name", list(pc.NOT_PW))
def test_a_plan_the_rule_does_not_serve_runs_as_without_the_option(pkg, dev, synth, name):
    s, w, x, b, td = _inputs(synth, name)
    off, on = _both(pkg, dev, s, w, x, td)
    assert off == on and off[0] in (pkg.WGRAD_ENTRY, pkg.WGRAD_STAGED)


def test_a_double_plan_runs_as_without_the_option(pkg, dev, synth):
    s, w, x, b, td = _inputs(synth, "pw_g3")
    off, on = _both(pkg, dev, s, w, x, td, dt=np.float64)
    assert off == on and off[0] == pkg.WGRAD_ENTRY


def test_a_forced_kernel_wins_over_the_option(pkg, dev, synth):
    s, w, x, b, td = _inputs(synth, "pw_straddle")
    for kernel in (pkg.WGRAD_ENTRY, pkg.WGRAD_STAGED, pkg.WGRAD_MFMA):
        off, on = _both(pkg, dev, s, w, x, td, wgrad_kernel=kernel)
        assert off == on and off[0] == kernel
    # the option set on an aligned plan is read when the next backward state is built
    plan = _plan(pkg, s, w, on=0)
    xt, tdt = _up(x, dev), _up(td, dev)
    plan.backward(tdt, bottom=xt, bottom_diff=None, values_diff=True)
    assert plan.stat("wgrad_kernel") != pkg.WGRAD_POINTWISE
    plan.set_option("wgrad_pointwise", 1)
    plan.backward(tdt, bottom=xt, bottom_diff=None, values_diff=True)
    assert plan.stat("wgrad_kernel") != pkg.WGRAD_POINTWISE       # a state that exists keeps its kernel
    plan.weight_align(w)
    plan.backward(tdt, bottom=xt, bottom_diff=None, values_diff=True)
    torch.cuda.synchronize()
    _ran(pkg, plan)
    plan.close()


# ---- 6. the wrappers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
def test_b2s_hands_the_option_to_its_inner_plan(pkg, synth, dev, relu):
    s = pc.make(synth, "pw_fc")
    w, x, b = synth.pruned_weights(s, 11), synth.activations(s, 12), synth.bias_vector(s, 13)
    sk = eb.skew(s, w, x, b, 95, top_diff=seeded((s.N, s.M, 1, 1), 21))
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu), b2s=1, wgrad_pointwise=1)
    plan.weight_align(sk.w)
    assert plan.stat("b2s") == 1 and plan.stat("b2s_block") == b2s_common.rule_block(s.N)
    xd, tdd = _up(sk.x, dev), _up(sk.top_diff, dev)
    topd = plan.forward(xd, _up(sk.b, dev)) if relu else None
    torch.cuda.synchronize()
    top_np = topd.cpu().numpy() if relu else None
    want, Bs = eb.backward_bound(s, sk.w, sk.x, sk.b, sk.top_diff, top_np)
    _, wd, bsd = plan.backward(tdd, bottom=xd, top=topd, bottom_diff=None, weight_diff=True, bias_diff=True)
    _, vd, _ = plan.backward(tdd, bottom=xd, top=topd, bottom_diff=None, values_diff=True)
    torch.cuda.synchronize()
    _ran(pkg, plan)
    what = ("pw_fc", relu)
    r = eb.within(wd.cpu().numpy(), want[1], Bs[1], "b2s wgrad_pointwise", what=what)
    rb = eb.within(bsd.cpu().numpy(), want[2], Bs[2], "b2s wgrad_pointwise bias", what=what)
    pos = csr_positions(plan)
    rv = eb.within(vd.cpu().numpy(), want[1].reshape(-1)[pos], Bs[1].reshape(-1)[pos], "b2s wgrad_pointwise compact", what=what)
    print("errbound b2s wgrad_pointwise relu=%d: %.3g, bias %.3g, values %.3g" % (relu, r, rb, rv))
    assert r <= 1.0 and rb <= 1.0 and rv <= 1.0
    assert vd.cpu().numpy().tobytes() == wd.cpu().numpy().reshape(-1)[pos].tobytes()
    plan.close()


def test_b2s_and_deconv_hand_the_option_on_when_it_is_set_on_an_aligned_plan(pkg, synth, dev):
    s = pc.make(synth, "pw_fc")
    w, x = synth.pruned_weights(s, 11), synth.activations(s, 12)
    td = seeded((s.N, s.M, 1, 1), 21)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s), b2s=1)
    plan.weight_align(w)
    plan.set_option("wgrad_pointwise", 1)
    _, vd, _ = plan.backward(_up(td, dev), bottom=_up(x, dev), bottom_diff=None, values_diff=True)
    torch.cuda.synchronize()
    _ran(pkg, plan)
    assert rel_err(vd.cpu().numpy(), torch_backward(x, w, None, s, td)[1].reshape(-1)[csr_positions(plan)]) <= TOL
    plan.close()
    d = pc.DECONV
    wdc = dc.weights(d)
    xdc, _, tdc = dc.inputs(d)
    plan = pkg.Plan(dc.desc(pkg, d), deconv=1)
    plan.weight_align(wdc)
    plan.set_option("wgrad_pointwise", 1)
    plan.backward(_up(tdc, dev), bottom=_up(xdc, dev), weight_diff=True)
    torch.cuda.synchronize()
    _ran(pkg, plan)
    plan.close()


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
def test_deconv_hands_the_option_to_its_pointwise_inner_plan(pkg, synth, dev, relu):
    d = pc.DECONV
    w = dc.weights(d)
    x, b, td = dc.inputs(d)
    plan = pkg.Plan(dc.desc(pkg, d, True, relu), deconv=1, wgrad_pointwise=1)
    plan.weight_align(w)
    xd, tdd = _up(x, dev), _up(td, dev)
    topd = plan.forward(xd, _up(b, dev)) if relu else None
    torch.cuda.synchronize()
    tp = topd.cpu().numpy() if relu else None
    wantb, Bs = dc.backward_bound(eb, synth, d, w, x, td, tp)
    got = plan.backward(tdd, bottom=xd, top=topd, weight_diff=True, bias_diff=True)
    _, vd, _ = plan.backward(tdd, bottom=xd, top=topd, bottom_diff=None, values_diff=True)
    torch.cuda.synchronize()
    _ran(pkg, plan)
    r = [eb.within(g.cpu().numpy(), wn, Bn, "deconv wgrad_pointwise", what=("pw_deconv", relu, k)) for g, wn, Bn, k in
         zip(got, wantb, Bs, ("bottom_diff", "weight_diff", "bias_diff"))]
    print("errbound deconv wgrad_pointwise relu=%d: %s" % (relu, r))
    assert max(r) <= 1.0
    wd = got[1].cpu().numpy()
    assert not wd[w == 0].any()
    assert vd.cpu().numpy().tobytes() == wd.reshape(-1)[np.flatnonzero(w.reshape(-1))].tobytes()
    plan.close()


# ---- 7. the state's lifetime -----------------------------------------------------------------------------------------------------
def _fresh_equals(pkg, dev, s, plan, xt, tdt, what):
    """The plan's next backward equals a fresh plan's on the same CSR, bit for bit."""
    rp, ci, vals, ng = plan.get_csr()
    fresh = pkg.Plan(pkg.ConvDesc.from_shape(s), wgrad_pointwise=1)
    fresh.set_csr(rp, ci, vals, ng)
    a = plan.backward(tdt, bottom=xt, bottom_diff=None, values_diff=True, bias_diff=True)
    b = fresh.backward(tdt, bottom=xt, bottom_diff=None, values_diff=True, bias_diff=True)
    torch.cuda.synchronize()
    _ran(pkg, plan)
    _ran(pkg, fresh)
    assert a[1].shape == (plan.nnz(),) and _bytes(a[1]) == _bytes(b[1]) and _bytes(a[2]) == _bytes(b[2]), what
    fresh.close()
    return a


def test_prune_rewire_set_csr_and_import_rebuild_the_state(pkg, dev, synth):
    s, w, x, b, td = _inputs(synth, "pw_straddle")
    xt, tdt = _up(x, dev), _up(td, dev)
    plan = _plan(pkg, s, w)
    first = _fresh_equals(pkg, dev, s, plan, xt, tdt, "align")
    # set_values and solver_step keep the state and do not change the gradient
    plan.set_values(_up(seeded((plan.nnz(),), 55), dev))
    assert plan.stat("update_fast") == 1
    again = plan.backward(tdt, bottom=xt, bottom_diff=None, values_diff=True, bias_diff=True)
    vd = again[1].clone()
    plan.solver_step(vd, torch.zeros(plan.nnz(), device=dev), type="sgd", rate=1e-3, momentum=0.9)
    third = plan.backward(tdt, bottom=xt, bottom_diff=None, values_diff=True, bias_diff=True)
    torch.cuda.synchronize()
    assert _bytes(first[1]) == _bytes(again[1]) == _bytes(third[1]) and _bytes(first[2]) == _bytes(third[2])
    n = plan.nnz()
    plan.prune(keep=n - n // 3)
    assert plan.nnz() == n - n // 3
    _fresh_equals(pkg, dev, s, plan, xt, tdt, "prune")
    score = plan.dense_wgrad(tdt, xt)
    n1 = plan.nnz()
    plan.rewire(n // 4, score.reshape(-1), drop_keep=n1 - n // 8)
    assert plan.nnz() == n1 - n // 8 + n // 4
    _fresh_equals(pkg, dev, s, plan, xt, tdt, "rewire")
    rp, ci, vals, ng = plan.get_csr()
    keep = np.ones(len(ci), bool)
    keep[::2] = False                                     # another pattern through set_csr
    mg = s.M // s.group
    rows = np.repeat(np.arange(mg), np.diff(rp[:mg + 1]))
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=mg))]).astype(np.int32)
    plan.set_csr(rp2, ci[keep], vals[keep], np.array([keep.sum()], np.int32))
    _fresh_equals(pkg, dev, s, plan, xt, tdt, "set_csr")
    blob = plan.export_aligned()
    other = pkg.Plan(pkg.ConvDesc.from_shape(s), wgrad_pointwise=1)
    other.import_aligned(blob)
    a = _fresh_equals(pkg, dev, s, other, xt, tdt, "import")
    bb = plan.backward(tdt, bottom=xt, bottom_diff=None, values_diff=True, bias_diff=True)
    torch.cuda.synchronize()
    assert _bytes(a[1]) == _bytes(bb[1])
    other.close()
    plan.close()


# ---- 8. captured training loop ---------------------------------------------------------------------------------------------
def test_captured_training_loop_equals_eager_steps(pkg, dev, synth):
    """forward -> backward(values_diff) -> solver_step(SGD with momentum, clear_diff) on pw_straddle: after one eager step
    the loop is captured on one stream, replayed three times and compared with three eager steps of a second plan: values
    and histories bit for bit."""
    s, w0, x, b, td = _inputs(synth, "pw_straddle")
    xt, tdt, bt = _up(x, dev), _up(td, dev), _up(b, dev)
    hyper = dict(type="sgd", rate=1e-3, momentum=0.9, clear_diff=1)

    def make_plan():
        plan = _plan(pkg, s, w0)
        oh, ow = plan.out_hw
        n = plan.nnz()
        return plan, dict(y=torch.zeros((s.N, s.M, oh, ow), device=dev), vd=torch.zeros(n, device=dev), h=torch.zeros(n, device=dev))

    def step(plan, u):
        plan.forward(xt, bt, u["y"])
        plan.backward(tdt, bottom=xt, bottom_diff=None, values_diff=u["vd"])
        plan.solver_step(u["vd"], u["h"], **hyper)

    def warm(plan, u):
        v0 = plan.get_csr()[2].copy()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step(plan, u)           # builds the backward and update states outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        _ran(pkg, plan)
        assert plan.stat("update_fast") == 1
        plan.set_values(torch.from_numpy(v0).to(dev))
        u["h"].zero_()
        torch.cuda.synchronize()
        return v0

    ref, ru = make_plan()
    v0 = warm(ref, ru)
    for _ in range(3):
        step(ref, ru)
    torch.cuda.synchronize()

    plan, u = make_plan()
    warm(plan, u)
    ws1 = plan.workspace_bytes
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(plan, u)
    assert plan.workspace_bytes == ws1
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert plan.workspace_bytes == ws1
    _ran(pkg, plan)
    va, vr = plan.get_csr()[2], ref.get_csr()[2]
    assert va.tobytes() == vr.tobytes() and not np.array_equal(va, v0)
    assert _bytes(u["h"]) == _bytes(ru["h"]) and float(u["h"].abs().max()) > 0
    assert _bytes(u["y"]) == _bytes(ru["y"])
    assert np.all(u["vd"].cpu().numpy() == 0)
    plan.close()
    ref.close()
