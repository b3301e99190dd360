"""The edges of the number formats without a GPU: subnormal inputs, weights and results, sums next to the largest finite
number, non-finite reach and the solver rule on special values.

First the inputs check themselves: a model that flushes subnormal inputs or results, and a ReLU mask that flushes the top,
must leave the bound on the very arrays the kernels get, while a plain fp32 model stays inside it -- conditions on the
inputs, not measurements.  Then the CPU twins run on the same rows (test_fp32_edges_gpu.py runs the device on them)."""
import numpy as np
import pytest

import edges_common as ec
import errbound as eb
import solver_common as sc
from wgrad_common import csr_positions, torch_backward

NAMES = ["L3X3", "PW_B", "G5X5", "STR2", "DIL"]
DTYPES = [pytest.param(False, id="float"), pytest.param(True, id="double")]


def _dt(f64):
    return np.float64 if f64 else np.float32


# ---- the inputs check themselves ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_the_inputs_are_where_their_kind_says(synth, name, f64):
    tiny, top = ec.NORMAL[f64], (2.0 ** 1022 if f64 else 2.0 ** 126)
    for backward in (False, True):
        e = {k: ec.edge(synth, name, k, backward, f64)[1] for k in ec.KINDS}
        s = ec.edge(synth, name, "sub_in", backward, f64)[0]
        assert all(a.dtype == _dt(f64) for k in e for a in e[k] if a is not None)
        assert np.all(np.abs(e["sub_in"].x) < tiny) and np.count_nonzero(e["sub_in"].x) > 0.9 * e["sub_in"].x.size
        assert np.all(np.abs(e["sub_w"].w) < tiny) and np.count_nonzero(e["sub_w"].w) > 0
        bits = np.abs(e["sub_w"].w).view(np.uint64 if f64 else np.uint32)
        assert set(eb.SUB_W_PATTERNS) <= set(int(v) for v in bits.ravel())
        so = e["sub_out"]
        for a in (so.w, so.x, so.top_diff):      # (the bias is a result's term: it has to be subnormal itself)
            assert a is None or np.all(np.abs(a[a != 0]) >= tiny)
        if backward:
            mag = torch_backward(np.abs(so.x), np.abs(so.w), None, s, np.abs(so.top_diff))
            assert mag[0].max() < tiny and mag[1].max() < tiny and mag[0].max() > 0 and mag[1].max() > 0
            nm = e["near_max"]
            mag = torch_backward(np.abs(nm.x), np.abs(nm.w), None, s, np.abs(nm.top_diff), mask=np.ones(nm.w.shape, bool))
            S = max(mag[0].max(), mag[1].max(), np.abs(nm.top_diff.astype(np.float64)).sum(axis=(0, 2, 3)).max())
        else:
            assert eb.conv64(np.abs(so.x), np.abs(so.w), np.abs(so.b), s).max() < tiny
            nm = e["near_max"]
            S = eb.conv64(np.abs(nm.x), np.abs(nm.w), np.abs(nm.b), s).max()
        assert top <= S < 2 * top, (name, backward, S)


@pytest.mark.parametrize("name", NAMES)
def test_a_flushing_model_leaves_the_bound_and_a_plain_fp32_model_stays_inside(synth, name):
    """flush_inputs on sub_in and sub_w, flush_results on sub_out: at least half of the output elements are beyond their
    bound.  The plain fp32 model (unfused products added in CSR order) is within it on all four kinds."""
    for kind in ec.KINDS:
        s, e = ec.edge(synth, name, kind)
        want, B = ec.forward_ref(synth, name, kind, True, False)
        plain = ec.plain_fp32_forward(s, e.w, e.x, e.b)
        r = eb.within(plain, want, B, "the plain fp32 model", what=(name, kind))
        share = None
        if kind in ("sub_in", "sub_w"):
            flushed = eb.forward_bound(s, eb.flush_inputs(e.w), eb.flush_inputs(e.x), eb.flush_inputs(e.b))[0]
            share = ec.beyond(flushed, want, B)
        elif kind == "sub_out":
            share = ec.beyond(eb.flush_results(want), want, B)
        else:
            assert np.all(np.isfinite(plain))
        print("edges self-check %-5s %-8s plain fp32 model %.3g of the bound; flushed: %s of the elements beyond it" % (name, kind, r, share))
        assert share is None or share >= 0.5, (name, kind, share)


@pytest.mark.parametrize("name", NAMES)
def test_a_mask_that_flushes_the_top_leaves_the_data_gradient_bound(pkg, synth, name):
    """The tops of the sub_out forward hold positive subnormals; a mask computed from the flushed top drops their
    gradients, and the data gradient leaves its bound on every kind."""
    s, so = ec.edge(synth, name, "sub_out")
    top = np.maximum(ec.plain_fp32_forward(s, so.w, so.x, so.b), 0)
    assert ec.positive_subnormal(top).sum() > 0.25 * top.size
    for kind in ec.KINDS:
        e = ec.edge(synth, name, kind, backward=True)[1]
        want, Bs = eb.backward_bound(s, e.w, e.x, e.b, e.top_diff, top)
        flushed = torch_backward(e.x, e.w, e.b, s, e.top_diff, eb.flush_inputs(top))
        r = eb.check(flushed[0], want[0], Bs[0])[0]
        print("edges self-check %-5s %-8s data gradient under a flushed mask: %.3g x the bound" % (name, kind, r))
        assert r > 1.0, (name, kind, r)


# ---- the CPU twins on the same rows -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("kind", ec.KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_forward_cpu_within_the_bound(pkg, synth, name, kind, f64):
    s, e = ec.edge(synth, name, kind, f64=f64)
    for relu in (False, True):
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu))
        plan.weight_align_cpu(e.w)
        for bias in (False, True):
            got = plan.forward_cpu(e.x, e.b if bias else None, n_threads=3)
            want, B = ec.forward_ref(synth, name, kind, bias, relu, f64)
            r = eb.within(got, want, B, "forward_cpu", what=(name, kind, f64, bias, relu))
            print("edges forward_cpu %-5s %-8s f64=%d bias=%d relu=%d: %.3g" % (name, kind, f64, bias, relu, r))
            if kind == "near_max":
                assert np.all(np.isfinite(got))
        plan.close()


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("kind", ec.KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_backward_cpu_and_dense_wgrad_cpu_within_the_bound(pkg, synth, name, kind, f64):
    """Data, dense and compact weight and bias gradient, with and without ReLU; the ReLU runs under the top of the same
    plan's forward on the sub_out inputs: a mask of positive subnormal tops."""
    s, e = ec.edge(synth, name, kind, backward=True, f64=f64)
    so = ec.edge(synth, name, "sub_out", f64=f64)[1]
    for relu in (False, True):
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu))
        top = None
        if relu:
            plan.weight_align_cpu(so.w)
            top = plan.forward_cpu(so.x, so.b)
            assert ec.positive_subnormal(top, f64).sum() > 0.25 * top.size
        plan.weight_align_cpu(e.w)
        bd, wd, bsd = plan.backward_cpu(e.top_diff, bottom=e.x, top=top, weight_diff=True, bias_diff=True)
        _, vd, _ = plan.backward_cpu(e.top_diff, bottom=e.x, top=top, bottom_diff=None, values_diff=True)
        dw = plan.dense_wgrad_cpu(e.top_diff, e.x, top)
        pos = csr_positions(plan)
        plan.close()
        want, Bs = eb.backward_bound(s, e.w, e.x, e.b, e.top_diff, top, f64=f64)
        dwant, dB = eb.backward_bound(s, e.w, e.x, None, e.top_diff, top, f64=f64, mask=np.ones(e.w.shape, bool))
        what = (name, kind, f64, relu)
        rs = [eb.within(bd, want[0], Bs[0], "backward_cpu bottom_diff", what=what),
              eb.within(wd, want[1], Bs[1], "backward_cpu weight_diff", what=what),
              eb.within(bsd, want[2], Bs[2], "backward_cpu bias_diff", what=what),
              eb.within(vd, want[1].reshape(-1)[pos], Bs[1].reshape(-1)[pos], "backward_values_cpu", what=what),
              eb.within(dw, dwant[1], dB[1], "dense_wgrad_cpu", what=what)]
        print("edges backward_cpu %-5s %-8s f64=%d relu=%d: data %.3g weights %.3g bias %.3g compact %.3g dense_wgrad %.3g" %
              ((name, kind, f64, relu) + tuple(rs)))
        assert np.all(wd[e.w == 0] == 0)
        if kind == "near_max":
            assert all(np.all(np.isfinite(a)) for a in (bd, wd, bsd, vd, dw))


# ---- non-finite reach on the twins ----------------------------------------------------------------------------------------------
def _skewed(synth, name):
    return ec.skewed(synth, name)


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_forward_cpu_nan_reaches_exactly_the_outputs_whose_nonzeros_read_it(pkg, synth, name, f64):
    s, sk = _skewed(synth, name)
    dt = _dt(f64)
    pos = eb.poison_positions(s, sk.w)
    bad, clean = ec.poisoned_bottom(sk.x.astype(dt), pos, np.nan)
    reach = eb.reach_forward(s, sk.w, eb.poisoned(bad.shape, pos))
    assert 0 < reach.sum() < reach.size
    want, B = eb.forward_bound(s, sk.w, clean, sk.b, f64=f64)
    for relu in (False, True):
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu))
        plan.weight_align_cpu(sk.w.astype(dt))
        got = plan.forward_cpu(bad, sk.b.astype(dt), n_threads=3)
        plan.close()
        if relu:        # a NaN becomes +0 under ReLU
            assert np.all(np.isfinite(got)) and np.all(got[reach] == 0) and not np.any(np.signbit(got[reach]))
            eb.within(np.where(reach, 0, got), np.where(reach, 0, np.maximum(want, 0)), B, "forward_cpu", what=(name, "relu"))
        else:
            assert np.array_equal(~np.isfinite(got), reach) and np.all(np.isnan(got[reach])), (name, (~np.isfinite(got)).sum(), reach.sum())
            eb.within(np.where(reach, 0, got), np.where(reach, 0, want), B, "forward_cpu", sk.row_exp, what=(name, "beside the reach"))


@pytest.mark.parametrize("name", NAMES)
def test_forward_cpu_one_infinity_arrives_with_the_sign_of_the_weight_that_reads_it(pkg, synth, name):
    s, sk = _skewed(synth, name)
    pos = eb.poison_positions(s, sk.w)[-1]
    bad, _ = ec.poisoned_bottom(sk.x, [pos], np.inf)
    hit, sg = ec.reader_sign(s, sk.w, pos, bad.shape)
    assert hit.sum() > 0 and (sg < 0).sum() > 0 and (sg > 0).sum() > 0, (name, "the interior element needs readers of both signs")
    for relu in (False, True):
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu))
        plan.weight_align_cpu(sk.w)
        got = plan.forward_cpu(bad, sk.b)
        plan.close()
        assert np.all(np.isfinite(got[~hit]))
        assert np.all(got[sg > 0] == np.inf)
        if relu:        # -inf becomes +0
            assert np.all(got[sg < 0] == 0) and not np.any(np.signbit(got[sg < 0]))
        else:
            assert np.all(got[sg < 0] == -np.inf)


def masked_top_case(s, sk, top, pattern, out_hw):
    """A poisoned top_diff whose every poisoned element lies under a masked top: (top_diff with NaN, the same with 0, the top
    with 0, -1, NaN and -0.0 in turn at those positions)."""
    pos = eb.poison_positions_top(s, pattern, out_hw)
    bad, clean, t = sk.top_diff.copy(), sk.top_diff.copy(), top.copy()
    for i, p in enumerate(pos):
        bad[p], clean[p] = np.nan, 0
        t[p] = (0.0, -1.0, np.nan, -0.0)[i % 4]
    return bad, clean, t


@pytest.mark.parametrize("f64", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_backward_cpu_nan_in_top_diff_reaches_exactly_its_readers_and_nothing_under_a_masked_top(pkg, synth, name, f64):
    s, sk = _skewed(synth, name)
    dt = _dt(f64)
    oh_ow = ec.out_hw(s)
    pos = eb.poison_positions_top(s, sk.w, oh_ow)
    bad, clean = ec.poisoned_bottom(sk.top_diff.astype(dt), pos, np.nan)
    reach = eb.reach_data(s, sk.w, eb.poisoned(bad.shape, pos))
    assert 0 < reach.sum() < reach.size
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
    plan.weight_align_cpu(sk.w.astype(dt))
    got = plan.backward_cpu(bad, bottom=sk.x.astype(dt))[0]
    plan.close()
    want, Bs = eb.backward_bound(s, sk.w, sk.x, sk.b, clean, f64=f64)
    assert np.array_equal(~np.isfinite(got), reach), (name, (~np.isfinite(got)).sum(), reach.sum())
    eb.within(np.where(reach, 0, got), np.where(reach, 0, want[0]), Bs[0], "backward_cpu bottom_diff", what=(name, "beside the reach"))
    # fuse_relu: top <= 0, NaN or -0.0 masks the element, on every gradient
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=True))
    plan.weight_align_cpu(sk.w.astype(dt))
    top = plan.forward_cpu(sk.x.astype(dt), sk.b.astype(dt))
    bad, clean, t = masked_top_case(s, sk, top, sk.w, oh_ow)
    bd, wd, bsd = plan.backward_cpu(bad.astype(dt), bottom=sk.x.astype(dt), top=t, weight_diff=True, bias_diff=True)
    _, vd, _ = plan.backward_cpu(bad.astype(dt), bottom=sk.x.astype(dt), top=t, bottom_diff=None, values_diff=True)
    dw = plan.dense_wgrad_cpu(bad.astype(dt), sk.x.astype(dt), t)
    plan.close()
    want, Bs = eb.backward_bound(s, sk.w, sk.x, sk.b, clean, t, f64=f64)
    eb.within(bd, want[0], Bs[0], "backward_cpu bottom_diff", what=(name, "masked"))
    eb.within(wd, want[1], Bs[1], "backward_cpu weight_diff", what=(name, "masked"))
    eb.within(bsd, want[2], Bs[2], "backward_cpu bias_diff", what=(name, "masked"))
    assert np.all(np.isfinite(vd)) and np.all(np.isfinite(dw))


# ---- the solver rule on special values ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["float", "double"])
@pytest.mark.parametrize("rule,reg", ec.RULE_REG, ids=["%s-%s" % p for p in ec.RULE_REG])
def test_array_step_cpu_on_the_grid_of_special_values(pkg, rule, reg, dt):
    w, g, h, h2 = ec.solver_grid(dt)
    for i in range(len(ec.HYPERS)):
        hy = ec.hyper(i, rule, reg)
        want = sc.step(w, g, h, h2 if rule == "adam" else None, **hy)
        data, diff, hh, hh2 = w.copy(), g.copy(), h.copy(), (h2.copy() if rule == "adam" else None)
        pkg.solver_array_step_cpu(data, diff, hh, hh2, **hy)
        for what, a, b in (("data", data, want[0]), ("history", hh, want[1]), ("history2", hh2, want[2])):
            if b is not None:
                assert sc.equal_up_to_nan_payload(a, b), (rule, reg, i, what, _first_difference(a, b, w, g, h, h2))


def _first_difference(a, b, *inputs):
    na, nb = np.isnan(a), np.isnan(b)
    bad = np.flatnonzero((na != nb) | (~na & ~nb & (a.view(np.uint8).reshape(a.size, -1) != b.view(np.uint8).reshape(b.size, -1)).any(axis=1)))
    i = int(bad[0])
    return dict(index=i, n_bad=bad.size, got=a[i], want=b[i], inputs=[v[i] for v in inputs])


def finite_specials(n, dt, roll=0):
    sp = ec.specials(dt)
    return np.resize(np.roll(sp[np.isfinite(sp)], roll), n).astype(dt)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["float", "double"])
@pytest.mark.parametrize("rule", ["sgd", "nesterov", "adam"])
def test_plan_solver_step_cpu_on_the_finite_special_values(pkg, synth, rule, dt):
    """A plan whose values, gradient and histories are the finite specials: the step equals the restatement, and the
    plan's forward afterwards a fresh plan's on the same values, bit for bit."""
    s, w0, x, b, _ = ec.base(synth, "L3X3")
    plan, fresh = pkg.Plan(pkg.ConvDesc.from_shape(s)), pkg.Plan(pkg.ConvDesc.from_shape(s))
    plan.weight_align_cpu(w0.astype(dt))
    pos = csr_positions(plan)
    n = pos.size
    w, g, h = finite_specials(n, dt), finite_specials(n, dt, 5), finite_specials(n, dt, 11)
    h2 = np.abs(finite_specials(n, dt, 3)) if rule == "adam" else None
    dense = np.full(w0.size, np.nan, dt)
    dense[pos] = w
    plan.update_values_cpu(dense.reshape(w0.shape))
    hy = ec.hyper(1, rule, "L1")
    want = sc.step(w, g, h, h2, **hy)
    hh, hh2 = h.copy(), (None if h2 is None else h2.copy())
    plan.solver_step_cpu(g.copy(), hh, hh2, **hy)
    assert sc.equal_up_to_nan_payload(plan.get_csr()[2], want[0]) and sc.equal_up_to_nan_payload(hh, want[1])
    assert h2 is None or sc.equal_up_to_nan_payload(hh2, want[2])
    fresh.weight_align_cpu(w0.astype(dt))
    dense[pos] = plan.get_csr()[2]
    fresh.update_values_cpu(dense.reshape(w0.shape))
    a, c = plan.forward_cpu(x.astype(dt), b.astype(dt)), fresh.forward_cpu(x.astype(dt), b.astype(dt))
    assert sc.equal_up_to_nan_payload(a, c)
    plan.close()
    fresh.close()
