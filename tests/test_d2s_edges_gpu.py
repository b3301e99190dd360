"""Plan option "deconv" on the MI355X at the edges of fp32 (d2s_edges_common.py has the layers and the inputs;
test_d2s_edges_cpu.py proves the inputs right): subnormal inputs, weights and results and sums next to the largest finite
number through the unpack kernel's bias add and ReLU, the pack kernel's mask, the carry kernel and the bias-sum kernel, every
element within errbound's bound on the inner stride-1 layer carried through d2s_common's pack / unpack; the reach of a
non-finite bottom or top_diff element, as a set, read off the inner layer through unpack.

Every case asserts the kernels that ran.  The worst err / bound per family and kind is printed when the module ends
(pytest -s; profiles/errbound.md, "The edges of fp32")."""
import numpy as np
import pytest

import d2s_common as dc
import d2s_edges_common as de
import errbound as eb
from test_d2s_edges_cpu import prefill

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

WORST = {}
UNPACK = "escoin_d2s_unpack_kernel"
DENSE_NAME = "escoin_dense_mfma_kernel"


@pytest.fixture(scope="module")
def dev(pkg):
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        pytest.fail("no HIP device visible (these tests run on the MI355X)")
    yield torch.device("cuda:0")
    for k in sorted(WORST):
        print("edges worst %-28s %-9s %.3g" % (k[0], k[1], WORST[k]))


def _up(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _within(got, want, B, family, kind, what):
    r = eb.within(got, want, B, family, what=what)
    WORST[(family, kind)] = max(WORST.get((family, kind), 0.0), r)
    return r


class Family(object):
    """(id, layer, Plan options -- a string names a constant of the package --, what must have run: the inner kernel's
    substrings of kernel_name, the backward's stats)."""

    def __init__(self, id, layer, name=(), stats=None, **options):
        self.id, self.layer, self.name, self.stats, self.options = id, layer, name, stats or {}, options

    def plan(self, pkg, s, relu, w):
        o = {k: getattr(pkg, v) if isinstance(v, str) else v for k, v in self.options.items()}
        plan = pkg.Plan(dc.desc(pkg, s, True, relu), deconv=1, **o)
        plan.weight_align(w)
        return plan

    def ran(self, pkg, plan, backward=False):
        name = plan.kernel_name
        assert name.endswith(" + " + UNPACK) and all(t in name.lower() for t in self.name), (self.id, name)
        assert plan.stat("deconv") == 1 and plan.stat("s2d") == 0 and plan.stat("s2b") == 0 and plan.stat("b2s") == 0, (self.id, name)
        if backward:
            for k, v in self.stats.items():
                assert plan.stat(k) == getattr(pkg, v), (self.id, k, plan.stat(k), name)

    def dense_forward(self, plan):
        return DENSE_NAME in plan.kernel_name

    def dense_backward(self, pkg, plan):
        return plan.stat("bwd_data_kernel") in (pkg.KERNEL_DENSE, pkg.BWD_MFMA)

    def __repr__(self):
        return self.id


FAMILIES = [
    Family("deconv_auto", "k4s2p1"),
    Family("deconv_jit", "k4s2p1", kernel="KERNEL_JIT", backward_kernel="KERNEL_JIT", tiling_batch=256, name=("jit",),
           stats=dict(bwd_data_kernel="KERNEL_JIT")),
    Family("deconv_dense", "k4s2p1", kernel="KERNEL_DENSE", wgrad_kernel="WGRAD_MFMA", name=(DENSE_NAME,), stats=dict(wgrad_kernel="WGRAD_MFMA")),
    Family("deconv_generic", "k4s2p1", kernel="KERNEL_GENERIC", backward_kernel="KERNEL_GENERIC", wgrad_kernel="WGRAD_ENTRY", name=("generic",),
           stats=dict(bwd_data_kernel="KERNEL_GENERIC", wgrad_kernel="WGRAD_ENTRY")),
    Family("deconv_empty_phases", "k3x2_s2x3"),
    Family("deconv_cropped_rows", "k2s2p2"),
]
IDS = [f.id for f in FAMILIES]


# ---- forward: four kinds x (bias, ReLU) ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", de.KINDS)
@pytest.mark.parametrize("fam", FAMILIES, ids=IDS)
def test_forward_at_the_edges_within_the_bound(pkg, synth, dev, fam, kind):
    s, e = de.edge(synth, fam.layer, kind)[:2]
    xd, bd = _up(e.x, dev), _up(e.b, dev)
    for relu in (False, True):
        plan = fam.plan(pkg, s, relu, e.w)
        for bias in (False, True):
            got = plan.forward(xd, bd if bias else None)
            torch.cuda.synchronize()
            fam.ran(pkg, plan)
            got = got.cpu().numpy()
            want, B = de.forward_ref(synth, fam.layer, kind, bias, relu)
            r = _within(got, want, B, fam.id, kind, (fam.id, kind, "bias", bias, "relu", relu, plan.kernel_name))
            print("edges forward %-20s %-8s bias=%d relu=%d %s: %.3g" % (fam.id, kind, bias, relu, plan.kernel_name, r))
            if kind == "near_max":
                assert np.all(np.isfinite(got)), (fam.id, "a sum bounded by 2^127 overflowed")
        plan.close()


# ---- backward -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("kind", de.KINDS)
@pytest.mark.parametrize("fam", FAMILIES, ids=IDS)
def test_backward_at_the_edges_within_the_bound(pkg, synth, dev, fam, kind, relu):
    """Data gradient, dense and compact weight gradient and bias gradient.  The ReLU runs use the top of the same plan's
    forward on the sub_out inputs: the pack kernel's mask sees positive subnormal tops.  Under sub_out and near_max the
    carry and bias-sum kernels also accumulate onto prefilled blobs of that scale (errbound.accumulated_bound)."""
    s, e = de.edge(synth, fam.layer, kind, backward=True)[:2]
    topd = top = None
    if relu:
        so = de.edge(synth, fam.layer, "sub_out")[1]
        plan = fam.plan(pkg, s, True, so.w)
        topd = plan.forward(_up(so.x, dev), _up(so.b, dev)).clone()
        torch.cuda.synchronize()
        plan.close()
        top = topd.cpu().numpy()
        assert de.positive_subnormal(top).sum() > 0.25 * top.size, (fam.id, "the mask needs positive subnormal tops")
    plan = fam.plan(pkg, s, relu, e.w)
    xd, tdd = _up(e.x, dev), _up(e.top_diff, dev)
    bd, wd, bsd = plan.backward(tdd, bottom=xd, top=topd, bottom_diff=True, weight_diff=True, bias_diff=True)
    _, vd, _ = plan.backward(tdd, bottom=xd, top=topd, bottom_diff=None, values_diff=True)
    torch.cuda.synchronize()
    fam.ran(pkg, plan, backward=True)
    want, Bs = dc.backward_bound(eb, synth, s, e.w, e.x, e.top_diff, top)
    pos = np.flatnonzero(e.w.reshape(-1))
    what = (fam.id, kind, "relu", relu, plan.kernel_name, plan.stat("bwd_data_kernel"), plan.stat("wgrad_kernel"))
    got = [a.cpu().numpy() for a in (bd, wd, bsd, vd)]
    rs = [_within(got[0], want[0], Bs[0], fam.id + " data", kind, what), _within(got[1], want[1], Bs[1], fam.id + " weights", kind, what),
          _within(got[2], want[2], Bs[2], fam.id + " bias", kind, what),
          _within(got[3], want[1].reshape(-1)[pos], Bs[1].reshape(-1)[pos], fam.id + " compact", kind, what)]
    assert np.all(got[1][e.w == 0] == 0), what
    if kind == "near_max":
        assert all(np.all(np.isfinite(a)) for a in got), what
    if kind in ("sub_out", "near_max"):
        pre_w, pre_b = prefill(want[1], kind, 1), prefill(want[2], kind, 2)
        kw, kb = de.accumulate_terms(s, e.x.shape[0])
        _, wd2, bsd2 = plan.backward(tdd, bottom=xd, top=topd, bottom_diff=None, weight_diff=_up(pre_w, dev), bias_diff=_up(pre_b, dev))
        torch.cuda.synchronize()
        wd2, bsd2, on = wd2.cpu().numpy(), bsd2.cpu().numpy(), e.w != 0
        assert np.array_equal(wd2[~on], pre_w[~on]), what
        rs.append(_within(wd2[on], (want[1] + pre_w)[on], eb.accumulated_bound(Bs[1], pre_w, kw)[on], fam.id + " weights +=", kind, what))
        rs.append(_within(bsd2, want[2] + pre_b, eb.accumulated_bound(Bs[2], pre_b, kb), fam.id + " bias +=", kind, what))
        assert np.all(np.isfinite(wd2)) and np.all(np.isfinite(bsd2)), what
    print("edges backward %-20s %-8s relu=%d kernels %d/%d: data, weights, bias, compact%s %s" %
          (fam.id, kind, relu, plan.stat("bwd_data_kernel"), plan.stat("wgrad_kernel"), ", weights +=, bias +=" if len(rs) > 4 else "",
           " ".join("%.3g" % r for r in rs)))
    plan.close()


# ---- reach, forward -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES, ids=IDS)
def test_nan_in_the_bottom_reaches_exactly_the_outputs_whose_nonzeros_read_it(pkg, synth, dev, fam):
    """The reach is the inner layer's, read through unpack (the dense reach where the inner kernel is the dense one): exactly
    those top elements are NaN -- through the unpack kernel's bias add -- and +0, not -0, under its ReLU; every other element
    is within the bound."""
    s, sk = de.skewed(fam.layer)
    pos = de.bottom_positions(synth, s, sk.w)
    bad = sk.x.copy()
    for p in pos:
        bad[p] = np.nan
    xd, bd = _up(bad, dev), _up(sk.b, dev)
    for relu in (False, True):
        plan = fam.plan(pkg, s, relu, sk.w)
        got = plan.forward(xd, bd)
        torch.cuda.synchronize()
        fam.ran(pkg, plan)
        reach = de.reach_forward(synth, s, sk.w, eb.poisoned(bad.shape, pos), dense=fam.dense_forward(plan))
        assert 0 < reach.sum() < reach.size, (fam.id, reach.sum())
        got = got.cpu().numpy()
        what = (fam.id, "relu", relu, plan.kernel_name)
        plan.close()
        want, B = de.skewed_forward_ref(synth, fam.layer, relu)
        nonfinite = ~np.isfinite(got)
        if relu:
            assert not nonfinite.any(), (what, "a NaN survived the ReLU at", np.argwhere(nonfinite)[:4].tolist())
            assert np.all(got[reach] == 0) and not np.any(np.signbit(got[reach])), (what, "a reached NaN is +0 under ReLU")
        else:
            leaked, missed = nonfinite & ~reach, reach & ~nonfinite
            assert not leaked.any() and not missed.any(), \
                (what, "reach %d, leaked to %d elements %s, missed %d %s; poisoned %s" %
                 (reach.sum(), leaked.sum(), np.argwhere(leaked)[:6].tolist(), missed.sum(), np.argwhere(missed)[:6].tolist(), pos))
            assert np.all(np.isnan(got[reach]))
        _within(np.where(reach, 0, got), np.where(reach, 0, want), B, fam.id, "reach", what)


@pytest.mark.parametrize("fam", [f for f in FAMILIES if f.id in ("deconv_auto", "deconv_jit", "deconv_generic")], ids=lambda f: f.id)
def test_one_infinity_arrives_with_the_sign_of_the_weight_that_reads_it(pkg, synth, dev, fam):
    s, sk = de.skewed(fam.layer)
    pos = de.bottom_positions(synth, s, sk.w)[-1]
    bad = sk.x.copy()
    bad[pos] = np.inf
    hit, sg = de.reader_sign(synth, s, sk.w, pos, bad.shape[0])
    assert (sg > 0).sum() > 0 and (sg < 0).sum() > 0, (fam.id, "the interior element needs readers of both signs")
    for relu in (False, True):
        plan = fam.plan(pkg, s, relu, sk.w)
        got = plan.forward(_up(bad, dev), _up(sk.b, dev))
        torch.cuda.synchronize()
        fam.ran(pkg, plan)
        assert not fam.dense_forward(plan), (fam.id, plan.kernel_name)
        got = got.cpu().numpy()
        plan.close()
        what = (fam.id, "relu", relu)
        assert np.all(got[sg > 0] == np.inf), what
        if relu:
            assert np.all(got[sg < 0] == 0) and not np.any(np.signbit(got[sg < 0])), what
        else:
            assert np.all(got[sg < 0] == -np.inf), what
        assert np.all(np.isfinite(got[~hit])), what


@pytest.mark.parametrize("fam", FAMILIES, ids=IDS)
def test_a_poisoned_image_past_the_call_s_batch_reaches_nothing(pkg, synth, dev, fam):
    """The first images of the plan's batch; every element of the images behind them in the bottom blob is NaN, and the top
    images past the call's keep their fill (k2s2p2 has one image: the call is the whole batch, behind a NaN guard)."""
    s, sk = de.skewed(fam.layer)
    n = max(1, s.N // 2)
    bad = np.concatenate([sk.x, np.full((1,) + sk.x.shape[1:], np.nan, np.float32)])
    bad[n:] = np.nan
    plan = fam.plan(pkg, s, False, sk.w)
    xd = _up(bad, dev)
    top = torch.full((s.N + 1, s.M) + dc.out_hw(s), -7.5, device=dev)
    plan.forward(xd[:n], _up(sk.b, dev), top[:n])
    torch.cuda.synchronize()
    fam.ran(pkg, plan)
    plan.close()
    want, B = de.skewed_forward_ref(synth, fam.layer, False)
    _within(top[:n].cpu().numpy(), want[:n], B[:n], fam.id, "partial", (fam.id, "first images", n))
    assert bool((top[n:] == -7.5).all()), (fam.id, "images past the call's were written")


# ---- reach, data gradient ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES, ids=IDS)
def test_nan_in_top_diff_reaches_its_readers_in_bottom_diff(pkg, synth, dev, fam):
    """Through the pack kernel without a mask.  On the exact inner backward kernels the non-finite set is the sparse reach
    exactly; on the dense ones (0 x G inside a live step, include/escoin.h) at least the sparse reach and at most the dense."""
    s, sk = de.skewed(fam.layer)
    pos = de.top_positions(s, sk.w)
    bad, clean = sk.top_diff.copy(), sk.top_diff.copy()
    for p in pos:
        bad[p], clean[p] = np.nan, 0
    plan = fam.plan(pkg, s, False, sk.w)
    got = plan.backward(_up(bad, dev), bottom_diff=True)[0]
    torch.cuda.synchronize()
    fam.ran(pkg, plan)
    for k in ("bwd_data_kernel",):
        assert k not in fam.stats or plan.stat(k) == getattr(pkg, fam.stats[k]), (fam.id, plan.stat(k))
    dense = fam.dense_backward(pkg, plan)
    what = (fam.id, plan.kernel_name, plan.stat("bwd_data_kernel"))
    plan.close()
    got = got.cpu().numpy()
    ind = eb.poisoned(clean.shape, pos)
    lo = de.reach_data(synth, s, sk.w, ind)
    hi = de.reach_data(synth, s, sk.w, ind, dense=True) if dense else lo
    assert 0 < lo.sum() < lo.size
    nonfinite = ~np.isfinite(got)
    print("edges reach %-20s: %d non-finite elements; sparse reach %d, dense reach %d (%s)" %
          (fam.id, nonfinite.sum(), lo.sum(), hi.sum(), "dense kernel" if dense else "exact kernel"))
    assert not (lo & ~nonfinite).any() and not (nonfinite & ~hi).any(), (what, (lo & ~nonfinite).sum(), (nonfinite & ~hi).sum())
    want, Bs = dc.backward_bound(eb, synth, s, sk.w, sk.x, clean)
    _within(np.where(nonfinite, 0, got), np.where(nonfinite, 0, want[0]), Bs[0], fam.id + " data", "reach", what)


@pytest.mark.parametrize("fam", FAMILIES, ids=IDS)
def test_nan_in_top_diff_under_a_masked_top_reaches_nothing(pkg, synth, dev, fam):
    """fuse_relu: a top of 0, -1, NaN or -0.0 masks its top_diff element in the pack kernel, which every gradient reads: each
    is finite and within the bound of the reference without the poison."""
    s, sk = de.skewed(fam.layer)
    plan = fam.plan(pkg, s, True, sk.w)
    xd = _up(sk.x, dev)
    top = plan.forward(xd, _up(sk.b, dev)).cpu().numpy()
    bad, clean, t = de.masked_top_case(s, sk, top)
    tdd, topd = _up(bad, dev), _up(t, dev)
    bd, wd, bsd = plan.backward(tdd, bottom=xd, top=topd, bottom_diff=True, weight_diff=True, bias_diff=True)
    _, vd, _ = plan.backward(tdd, bottom=xd, top=topd, bottom_diff=None, values_diff=True)
    torch.cuda.synchronize()
    fam.ran(pkg, plan, backward=True)
    plan.close()
    pos = np.flatnonzero(sk.w.reshape(-1))
    want, Bs = dc.backward_bound(eb, synth, s, sk.w, sk.x, clean, t)
    _within(bd.cpu().numpy(), want[0], Bs[0], fam.id + " data", "masked", fam.id)
    _within(wd.cpu().numpy(), want[1], Bs[1], fam.id + " weights", "masked", fam.id)
    _within(bsd.cpu().numpy(), want[2], Bs[2], fam.id + " bias", "masked", fam.id)
    _within(vd.cpu().numpy(), want[1].reshape(-1)[pos], Bs[1].reshape(-1)[pos], fam.id + " compact", "masked", fam.id)
