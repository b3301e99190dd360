"""Plan option "deconv" at the edges of fp32 without a GPU (d2s_edges_common.py has the layers and the inputs).

First the inputs check themselves: the mapping from the inner layer's edge inputs back to the caller's arrays is proved
against torch's float64 conv_transpose2d; every array is where its kind says; a model that flushes subnormal inputs or
results leaves the bound on these very arrays while a plain fp32 model of the decomposition stays inside; and the tops the
ReLU runs mask with hold positive subnormals by the float64 reference alone.  Then the _cpu twin runs on the same rows
(test_d2s_edges_gpu.py runs the device on them)."""
import numpy as np
import pytest

import d2s_common as dc
import d2s_edges_common as de
import errbound as eb
from wgrad_common import torch_backward

pytest.importorskip("torch")

NAMES = list(de.LAYERS)


def _plan(pkg, s, w, relu=False):
    plan = pkg.Plan(dc.desc(pkg, s, True, relu), deconv=1)
    plan.weight_align_cpu(w)
    return plan


# ---- the inputs check themselves ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", de.KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_the_mapping_back_from_the_inner_layer(synth, name, kind):
    """The bias is equal over a channel's P phases; torch's float64 conv_transpose2d and its autograd on the mapped-back
    arrays equal the inner layer's float64 reference read through unpack / the entry map, to float64 rounding (both are sums
    of the same products in another order: gamma(terms) in double on the sum of magnitudes)."""
    s, e, si, inner = de.edge(synth, name, kind, backward=True)
    P = dc.inner_dims(s)[0]
    assert np.array_equal(inner.b, np.repeat(e.b, P)) and e.w.shape == (s.C, s.M // s.group, s.KH, s.KW)
    wi, at = dc.inner_weights(s, e.w)
    assert np.array_equal(wi, inner.w) and np.array_equal(dc.pack(s, e.top_diff), inner.top_diff)
    assert not np.any((e.w != 0) & (de.base(name)[1] == 0))      # (sub_w rounds a few of the smallest weights to 0: none appears)
    want, B = eb.forward_bound(si, inner.w, inner.x, inner.b)
    u = eb.U64 / eb.U32
    got = dc.ref_forward(s, e.w, e.x, e.b)
    assert np.all(np.abs(got - dc.unpack(s, want)) <= dc.unpack(s, B) * u), (name, kind, "forward")
    gwant, gB = eb.backward_bound(si, inner.w, inner.x, inner.b, inner.top_diff)
    bd, wd, bsd = dc.ref_backward(s, e.w, e.x, e.b, e.top_diff)
    assert np.all(np.abs(bd - gwant[0]) <= gB[0] * u), (name, kind, "bottom_diff")
    assert np.all(np.abs(wd - gwant[1].reshape(-1)[at] * (e.w != 0)) <= gB[1].reshape(-1)[at] * u), (name, kind, "weight_diff")
    assert np.all(np.abs(bsd - gwant[2].reshape(s.M, P).sum(axis=1)) <= gB[2].reshape(s.M, P).sum(axis=1) * u), (name, kind, "bias_diff")
    # ... and d2s_common's bounds are those numbers
    w2, B2 = dc.forward_bound(eb, synth, s, e.w, e.x, e.b)
    assert np.array_equal(w2, dc.unpack(s, want)) and np.array_equal(B2, dc.unpack(s, B))


@pytest.mark.parametrize("name", NAMES)
def test_the_inputs_are_where_their_kind_says(synth, name):
    tiny, top = de.NORMAL, 2.0 ** 126
    for backward in (False, True):
        e = {k: de.edge(synth, name, k, backward)[1] for k in de.KINDS}
        s, _, si, _ = de.edge(synth, name, "sub_in", backward)
        assert all(a.dtype == np.float32 for k in e for a in e[k] if a is not None)
        assert np.all(np.abs(e["sub_in"].x) < tiny) and np.count_nonzero(e["sub_in"].x) > 0.9 * e["sub_in"].x.size
        assert np.all(np.abs(e["sub_w"].w) < tiny) and np.count_nonzero(e["sub_w"].w) > 0
        bits = np.abs(e["sub_w"].w).view(np.uint32)
        assert set(eb.SUB_W_PATTERNS) <= set(int(v) for v in bits.ravel())
        so = e["sub_out"]
        for a in (so.w, so.x, so.top_diff):
            assert a is None or np.all(np.abs(a[a != 0]) >= tiny)
        wi = lambda w: dc.inner_weights(s, w)[0]  # noqa: E731
        bi = lambda b: np.repeat(b, dc.inner_dims(s)[0])  # noqa: E731
        if backward:
            assert np.count_nonzero(so.top_diff) > 0.9 * so.top_diff.size
            mag = torch_backward(np.abs(so.x), np.abs(wi(so.w)), None, si, np.abs(dc.pack(s, so.top_diff)))
            assert mag[0].max() < tiny and mag[1].max() < tiny and mag[0].max() > 0 and mag[1].max() > 0
            nm = e["near_max"]
            g = np.abs(dc.pack(s, nm.top_diff))
            mag = torch_backward(np.abs(nm.x), np.abs(wi(nm.w)), None, si, g, mask=np.ones(wi(nm.w).shape, bool))
            # (a bias gradient sums a channel's whole top, P inner rows: far below the weight gradient's sums, which carry
            # the bottom's 2^60 as well)
            S = max(mag[0].max(), mag[1].max(), np.abs(nm.top_diff.astype(np.float64)).sum(axis=(0, 2, 3)).max())
        else:
            assert dc.unpack(s, eb.conv64(np.abs(so.x), np.abs(wi(so.w)), np.abs(bi(so.b)), si)).max() < tiny
            nm = e["near_max"]
            S = eb.conv64(np.abs(nm.x), np.abs(wi(nm.w)), np.abs(bi(nm.b)), si).max()
        assert top <= S < 2 * top, (name, backward, S)


@pytest.mark.parametrize("name", NAMES)
def test_a_flushing_model_leaves_the_bound_and_a_plain_fp32_model_stays_inside(synth, name):
    """flush_inputs on sub_in and sub_w, flush_results on sub_out: more than a quarter of the top elements are beyond their
    bound, the worst by more than 100 x (k2s2p2's outputs are sums of at most three products next to a bias 2^6 larger: where
    all three are small the flushed result is inside).  The plain fp32 model of the decomposition is within the bound on
    all four kinds."""
    for kind in de.KINDS:
        s, e = de.edge(synth, name, kind)[:2]
        want, B = de.forward_ref(synth, name, kind, True, False)
        plain = de.plain_fp32_forward(synth, s, e.w, e.x, e.b)
        r = eb.within(plain, want, B, "the plain fp32 model", what=(name, kind))
        share = flushed = None
        if kind in ("sub_in", "sub_w"):
            flushed = dc.forward_bound(eb, synth, s, eb.flush_inputs(e.w), eb.flush_inputs(e.x), eb.flush_inputs(e.b))[0]
        elif kind == "sub_out":
            flushed = eb.flush_results(want)
        else:
            assert np.all(np.isfinite(plain))
        if flushed is not None:
            share = float((~(np.abs(flushed - want) <= B)).mean())
            assert eb.check(flushed, want, B)[0] > 100, (name, kind)
        print("deconv edges self-check %-10s %-8s plain fp32 model %.3g of the bound; flushed: %s of the elements beyond it" % (name, kind, r, share))
        assert share is None or share > 0.25, (name, kind, share)


@pytest.mark.parametrize("name", NAMES)
def test_the_masking_tops_hold_positive_subnormals_by_the_reference_alone(synth, name):
    """The ReLU runs of the backward take the top of the sub_out forward as their mask and require more than a quarter of it
    to be positive subnormals.  From the float64 reference alone: every element with 0 < want - B and want + B < 2^-126 is
    one on any kernel within the bound, and those are more than a quarter."""
    want, B = de.forward_ref(synth, name, "sub_out", True, True)
    sure = (want - B > 0) & (want + B < de.NORMAL)
    print("deconv edges %-10s: %.3f of the sub_out tops are positive subnormals whatever the rounding" % (name, sure.mean()))
    assert sure.sum() > 0.25 * want.size, (name, sure.mean())


@pytest.mark.parametrize("name", NAMES)
def test_a_mask_that_flushes_the_top_leaves_the_data_gradient_bound(synth, name):
    s, so = de.edge(synth, name, "sub_out")[:2]
    top = np.maximum(de.plain_fp32_forward(synth, s, so.w, so.x, so.b), 0)
    assert de.positive_subnormal(top).sum() > 0.25 * top.size
    for kind in de.KINDS:
        e = de.edge(synth, name, kind, backward=True)[1]
        want, Bs = dc.backward_bound(eb, synth, s, e.w, e.x, e.top_diff, top)
        flushed = dc.ref_backward(s, e.w, e.x, e.b, e.top_diff, eb.flush_inputs(top))
        r = eb.check(flushed[0], want[0], Bs[0])[0]
        print("deconv edges self-check %-10s %-8s data gradient under a flushed mask: %.3g x the bound" % (name, kind, r))
        assert r > 1.0, (name, kind, r)


# ---- the CPU twin on the same rows -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", de.KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_forward_cpu_within_the_bound(pkg, synth, name, kind):
    s, e = de.edge(synth, name, kind)[:2]
    for relu in (False, True):
        plan = _plan(pkg, s, e.w, relu)
        for bias in (False, True):
            got = plan.forward_cpu(e.x, e.b if bias else None)
            want, B = de.forward_ref(synth, name, kind, bias, relu)
            r = eb.within(got, want, B, "forward_cpu", what=(name, kind, bias, relu))
            print("deconv edges forward_cpu %-10s %-8s bias=%d relu=%d: %.3g" % (name, kind, bias, relu, r))
            if kind == "near_max":
                assert np.all(np.isfinite(got))
        plan.close()


@pytest.mark.parametrize("kind", de.KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_backward_cpu_within_the_bound(pkg, synth, name, kind):
    """Data, dense and compact weight and bias gradient, linear and under the top of the same plan's forward on the sub_out
    inputs; then the same gradients accumulated onto prefilled blobs at the kind's own scale."""
    s, e = de.edge(synth, name, kind, backward=True)[:2]
    so = de.edge(synth, name, "sub_out")[1]
    pos = np.flatnonzero(e.w.reshape(-1))
    for relu in (False, True):
        top = None
        if relu:
            plan = _plan(pkg, s, so.w, True)
            top = plan.forward_cpu(so.x, so.b)
            plan.close()
            assert de.positive_subnormal(top).sum() > 0.25 * top.size
        plan = _plan(pkg, s, e.w, relu)
        bd, wd, bsd = plan.backward_cpu(e.top_diff, bottom=e.x, top=top, weight_diff=True, bias_diff=True)
        _, vd, _ = plan.backward_cpu(e.top_diff, bottom=e.x, top=top, bottom_diff=None, values_diff=True)
        want, Bs = dc.backward_bound(eb, synth, s, e.w, e.x, e.top_diff, top)
        what = (name, kind, relu)
        rs = [eb.within(bd, want[0], Bs[0], "backward_cpu bottom_diff", what=what), eb.within(wd, want[1], Bs[1], "backward_cpu weight_diff", what=what),
              eb.within(bsd, want[2], Bs[2], "backward_cpu bias_diff", what=what),
              eb.within(vd, want[1].reshape(-1)[pos], Bs[1].reshape(-1)[pos], "backward_values_cpu", what=what)]
        assert np.all(wd[e.w == 0] == 0)
        if kind == "near_max":
            assert all(np.all(np.isfinite(a)) for a in (bd, wd, bsd, vd))
        if kind in ("sub_out", "near_max"):
            pre_w, pre_b = prefill(want[1], kind, 1), prefill(want[2], kind, 2)
            kw, kb = de.accumulate_terms(s, e.x.shape[0])
            _, wd2, bsd2 = plan.backward_cpu(e.top_diff, bottom=e.x, top=top, bottom_diff=None, weight_diff=pre_w.copy(), bias_diff=pre_b.copy())
            on = e.w != 0
            rs.append(eb.within(wd2[on], (want[1] + pre_w)[on], eb.accumulated_bound(Bs[1], pre_w, kw)[on], "backward_cpu weight_diff +=", what=what))
            rs.append(eb.within(bsd2, want[2] + pre_b, eb.accumulated_bound(Bs[2], pre_b, kb), "backward_cpu bias_diff +=", what=what))
            assert np.array_equal(wd2[~on], pre_w[~on])
        plan.close()
        print("deconv edges backward_cpu %-10s %-8s relu=%d: %s" % (name, kind, relu, " ".join("%.3g" % r for r in rs)))


def prefill(want, kind, seed):
    """A blob to accumulate onto, at the scale of the gradient it receives: subnormals of both signs under sub_out; under
    near_max 2^-6 of the largest finite magnitude, so that prefill + sum (below 2^127 by construction) stays finite."""
    u = np.random.RandomState(seed).uniform(-1, 1, want.shape)
    return (np.ldexp(u, -130) if kind == "sub_out" else np.ldexp(u, 121)).astype(np.float32)


# ---- non-finite reach on the twin -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_forward_cpu_nan_reaches_exactly_the_outputs_whose_nonzeros_read_it(pkg, synth, name):
    s, sk = de.skewed(name)
    pos = de.bottom_positions(synth, s, sk.w)
    bad = sk.x.copy()
    for p in pos:
        bad[p] = np.nan
    reach = de.reach_forward(synth, s, sk.w, eb.poisoned(bad.shape, pos))
    assert 0 < reach.sum() < reach.size
    for relu in (False, True):
        plan = _plan(pkg, s, sk.w, relu)
        got = plan.forward_cpu(bad, sk.b)
        plan.close()
        want, B = de.skewed_forward_ref(synth, name, relu)
        if relu:
            assert np.all(np.isfinite(got)) and np.all(got[reach] == 0) and not np.any(np.signbit(got[reach]))
        else:
            assert np.array_equal(~np.isfinite(got), reach) and np.all(np.isnan(got[reach])), (name, (~np.isfinite(got)).sum(), reach.sum())
        eb.within(np.where(reach, 0, got), np.where(reach, 0, want), B, "forward_cpu", what=(name, relu, "beside the reach"))


@pytest.mark.parametrize("name", ["k4s2p1"])
def test_forward_cpu_one_infinity_arrives_with_the_sign_of_the_weight_that_reads_it(pkg, synth, name):
    s, sk = de.skewed(name)
    pos = de.bottom_positions(synth, s, sk.w)[-1]
    bad = sk.x.copy()
    bad[pos] = np.inf
    hit, sg = de.reader_sign(synth, s, sk.w, pos, bad.shape[0])
    assert (sg < 0).sum() > 0 and (sg > 0).sum() > 0, (name, "the interior element needs readers of both signs")
    for relu in (False, True):
        plan = _plan(pkg, s, sk.w, relu)
        got = plan.forward_cpu(bad, sk.b)
        plan.close()
        assert np.all(np.isfinite(got[~hit])) and np.all(got[sg > 0] == np.inf)
        if relu:
            assert np.all(got[sg < 0] == 0) and not np.any(np.signbit(got[sg < 0]))
        else:
            assert np.all(got[sg < 0] == -np.inf)


@pytest.mark.parametrize("name", NAMES)
def test_backward_cpu_nan_in_top_diff_reaches_exactly_its_readers_and_nothing_under_a_masked_top(pkg, synth, name):
    s, sk = de.skewed(name)
    pos = de.top_positions(s, sk.w)
    bad, clean = sk.top_diff.copy(), sk.top_diff.copy()
    for p in pos:
        bad[p], clean[p] = np.nan, 0
    reach = de.reach_data(synth, s, sk.w, eb.poisoned(bad.shape, pos))
    assert 0 < reach.sum() < reach.size
    plan = _plan(pkg, s, sk.w)
    got = plan.backward_cpu(bad, bottom=sk.x)[0]
    plan.close()
    want, Bs = dc.backward_bound(eb, synth, s, sk.w, sk.x, clean)
    assert np.array_equal(~np.isfinite(got), reach), (name, (~np.isfinite(got)).sum(), reach.sum())
    eb.within(np.where(reach, 0, got), np.where(reach, 0, want[0]), Bs[0], "backward_cpu bottom_diff", what=(name, "beside the reach"))
    plan = _plan(pkg, s, sk.w, True)
    top = plan.forward_cpu(sk.x, sk.b)
    bad, clean, t = de.masked_top_case(s, sk, top)
    bd, wd, bsd = plan.backward_cpu(bad, bottom=sk.x, top=t, weight_diff=True, bias_diff=True)
    _, vd, _ = plan.backward_cpu(bad, bottom=sk.x, top=t, bottom_diff=None, values_diff=True)
    plan.close()
    want, Bs = dc.backward_bound(eb, synth, s, sk.w, sk.x, clean, t)
    eb.within(bd, want[0], Bs[0], "backward_cpu bottom_diff", what=(name, "masked"))
    eb.within(wd, want[1], Bs[1], "backward_cpu weight_diff", what=(name, "masked"))
    eb.within(bsd, want[2], Bs[2], "backward_cpu bias_diff", what=(name, "masked"))
    assert np.all(np.isfinite(vd))
