"""Plan option "wgrad_depthwise" on the MI355X: weight_diff, bias_diff and the compact values of escoin_depthwise_wgrad_kernel on
the cases of wgrad_depthwise_common.py -- every shape of depthwise_common.py under ("depthwise_band_rows", "wgrad_depthwise_slices")
in ((0, 0), (1, 1), (2, 3)), and the shapes that run the px = 2 and px = 4 instantiations, with and without fuse_relu -- element by
element within errbound's bound of the float64 reference (gamma(N x OH x OW + 4) on the sum of magnitudes: it holds for any
summation order); a partial batch, accumulation, a bias-only call; unserved plans; an in-place update."""
import numpy as np
import pytest

import depthwise_common as dc
import wgrad_depthwise_common as wc
import errbound as eb
from upd_common import new_weights, values_at

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

KERNEL = "escoin_depthwise_wgrad_kernel"
_REFS = {}


@pytest.fixture(scope="module")
def dev(pkg):
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        pytest.fail("no HIP device visible (these tests run on the MI355X)")
    return torch.device("cuda:0")


def _up(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _plan(pkg, s, w, relu=False, **opts):
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu), **opts)
    plan.weight_align(w)
    return plan


def _ref(synth, name, relu, top, n):
    """(want, bounds) of the first n images, computed once; top: the forward's, the mask of a fuse_relu plan."""
    if (name, relu, n) not in _REFS:
        s, w, x, b, td = wc.case(synth, name)
        _REFS[name, relu, n] = eb.backward_bound(s._replace(N=n), w, x[:n], b, td[:n], None if top is None else top[:n])
    return _REFS[name, relu, n]


def _grads(plan, s, x, td, dev, top=None, n=None, **out):
    """[weight_diff or values_diff, bias_diff] of the first n images as numpy"""
    got = plan.backward(_up(td, dev)[:n], bottom=_up(x, dev)[:n], top=None if top is None else _up(top, dev)[:n], bottom_diff=None, **out)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in got[1:]]


@pytest.mark.parametrize("name,relu,opts,px,slices", wc.CASES)
def test_gradients_are_within_the_bound(pkg, synth, dev, name, relu, opts, px, slices):
    s, w, x, b, td = wc.case(synth, name)
    plan = _plan(pkg, s, w, relu, wgrad_depthwise=1, depthwise_band_rows=opts[0], wgrad_depthwise_slices=opts[1])
    top = plan.forward(_up(x, dev), _up(b, dev)).cpu().numpy() if relu else None
    want, Bs = _ref(synth, name, relu, top, s.N)
    wd, bd = _grads(plan, s, x, td, dev, top, weight_diff=True, bias_diff=True)
    assert plan.stat("wgrad_kernel") == pkg.WGRAD_DEPTHWISE == 5 and plan.stat("wgrad_depthwise_slices") == slices
    assert plan.stat("wgrad_depthwise_px") == px                    # the instantiation the case is there for
    eb.within(wd, want[1], Bs[1], KERNEL, what=(name, relu, opts))
    eb.within(bd, want[2], Bs[2], KERNEL + " bias", what=(name, relu, opts))
    assert np.all(wd[w == 0] == 0)
    vd, bd2 = _grads(plan, s, x, td, dev, top, values_diff=True, bias_diff=True)
    assert vd.tobytes() == values_at(plan, wd)[2].tobytes() and bd2.tobytes() == bd.tobytes()     # one kernel, two layouts
    eb.within(vd, values_at(plan, want[1])[2], values_at(plan, Bs[1])[2], KERNEL + " compact", what=(name, relu, opts))
    plan.close()


@pytest.mark.parametrize("name,opts", [("3x3_s2", (2, 3)), ("pruned", (1, 4))])
def test_partial_batch_accumulation_and_bias_only(pkg, synth, dev, name, opts):
    s, w, x, b, td = wc.case(synth, name)
    plan = _plan(pkg, s, w, wgrad_depthwise=1, depthwise_band_rows=opts[0], wgrad_depthwise_slices=opts[1])
    n, x2, td2 = s.N - 1, x.copy(), td.copy()       # a partial batch: the images at and past n are not read
    x2[n:], td2[n:] = np.nan, np.nan
    want, Bs = _ref(synth, name, False, None, n)
    wd, bd = _grads(plan, s, x2, td2, dev, n=n, weight_diff=True, bias_diff=True)
    eb.within(wd, want[1], Bs[1], KERNEL, what=(name, "partial"))
    eb.within(bd, want[2], Bs[2], KERNEL + " bias", what=(name, "partial"))
    # accumulation onto prefilled blobs; outside the pattern the prefill stays
    want, Bs = _ref(synth, name, False, None, s.N)
    rs, on, terms = np.random.RandomState(5), w != 0, s.N * int(np.prod(synth.out_hw(s)))
    pre_w, pre_b = rs.uniform(-1, 1, w.shape).astype(np.float32), rs.uniform(-1, 1, s.M).astype(np.float32)
    wd, bd = _grads(plan, s, x, td, dev, weight_diff=_up(pre_w, dev), bias_diff=_up(pre_b, dev))
    assert wd[~on].tobytes() == pre_w[~on].tobytes()
    eb.within(wd[on], (want[1] + pre_w)[on], eb.accumulated_bound(Bs[1], pre_w, terms)[on], KERNEL + " +=", what=name)
    eb.within(bd, want[2] + pre_b, eb.accumulated_bound(Bs[2], pre_b, terms), KERNEL + " bias +=", what=name)
    # the bias alone: within the bound, and the bits of the call that computes both
    alone = _grads(plan, s, x, td, dev, bias_diff=True)[1]
    assert plan.stat("wgrad_kernel") == 5 and alone.tobytes() == _grads(plan, s, x, td, dev, weight_diff=True, bias_diff=True)[1].tobytes()
    eb.within(alone, want[2], Bs[2], KERNEL + " bias alone", what=name)
    plan.close()


@pytest.mark.parametrize("what", ["cg2", "double", "forced"])
def test_unserved_plans_run_as_without_the_option(pkg, synth, dev, what):
    s, w, x, b, td = dc.case(synth, "cg2" if what == "cg2" else "3x3_s1")
    opts = dict(wgrad_kernel=pkg.WGRAD_ENTRY) if what == "forced" else {}
    if what == "double":
        w, x, td = (a.astype(np.float64) for a in (w, x, td))
    on, off = _plan(pkg, s, w, wgrad_depthwise=1, **opts), _plan(pkg, s, w, **opts)
    got, want = (_grads(p, s, x, td, dev, weight_diff=True, bias_diff=True) for p in (on, off))
    assert on.stat("wgrad_kernel") == off.stat("wgrad_kernel") != 5 and on.stat("wgrad_depthwise_slices") == 0
    assert all(g.tobytes() == v.tobytes() for g, v in zip(got, want))
    on.close(), off.close()


def test_update_in_place_equals_a_fresh_plan(pkg, synth, dev):
    s, w, x, b, td = dc.case(synth, "mult2")
    opts = dict(wgrad_depthwise=1, depthwise_band_rows=2, wgrad_depthwise_slices=3)
    plan = _plan(pkg, s, w, **opts)
    _grads(plan, s, x, td, dev, weight_diff=True)                   # (the backward state exists before the update)
    w_new, w_nan = new_weights(w, 31)
    plan.update_values(w_nan)
    fresh = pkg.Plan(pkg.ConvDesc.from_shape(s), **opts)
    fresh.set_csr(*values_at(plan, w_new))
    got, want = (_grads(p, s, x, td, dev, weight_diff=True, bias_diff=True) for p in (plan, fresh))
    assert all(g.tobytes() == v.tobytes() for g, v in zip(got, want)) and plan.stat("wgrad_kernel") == fresh.stat("wgrad_kernel") == 5
    plan.close(), fresh.close()
