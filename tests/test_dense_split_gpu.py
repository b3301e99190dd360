"""Plan option "dense_split" on the MI355X: escoin_dense_bf16x3_kernel under KERNEL_DENSE on the cases of dense_bf16_common.py
and the two off-boundary runs of layout_cases.py.  The reference is the float64 convolution of the UNROUNDED operands; the
bound is include/escoin.h's, unscaled: 2^-16 * sum |w||x| for the dropped and rounded terms plus the fp32 accumulation bound of
the 3 K products summed, three times errbound.forward_bound's.  The worst ratio measured: profiles/dense_split_mi355x.md."""
import numpy as np
import pytest

import dense_bf16_common as bc
import errbound as eb
import layout_cases as lc
from test_dense_bf16_gpu import _plan
from test_errbound_gpu import _up, dev  # noqa: F401
from test_errbound_layouts_gpu import _window

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
_REFS = {}


def _ref(c, s, sk, b):
    """want, bound without ReLU (1-Lipschitz: it keeps the bound), once per (case, bias)."""
    if (c.name, b is not None) not in _REFS:
        want, B = eb.forward_bound(s, sk.w, sk.x, b)
        _REFS[c.name, b is not None] = (want, 2.0 ** -16 * eb.forward_bound(s, np.abs(sk.w), np.abs(sk.x), None)[0] + 3.0 * B)
    return _REFS[c.name, b is not None]


def _bound_holds(plan, c, s, sk, xd, bias, relu, dev, top=None):
    want, B = _ref(c, s, sk, sk.b if bias else None)
    n = c.n_images
    got = plan.forward(xd[:n], _up(sk.b, dev) if bias else None, top).cpu().numpy()
    want = np.maximum(want[:n], 0.0) if relu else want[:n]
    r = eb.within(got, want, B[:n], "escoin_dense_bf16x3_kernel", sk.row_exp, what=(c.name, "bias", bias, "relu", relu))
    print("dense_split %-9s bias=%d relu=%d: worst err / bound %.3g" % (c.name, bias, relu, r))


@pytest.mark.parametrize("c", bc.CASES, ids=bc.IDS)
def test_bound_stats_cross_terms_and_the_way_back_to_fp32(pkg, synth, dev, c):
    """Per element within the bound, with and without bias and ReLU (b16_part: two of three images, the third untouched);
    the stats; with the option back at 0 the same plan gives a fresh fp32 plan's bits.  Then one run per cross term on
    integers, one operand in [-3, 3] (bf16 exactly) and the other in [-4095, 4095] (hi + lo exactly): with K <= 288 every
    partial sum stays below 288 * 3 * 4095 + 8 < 2^24, so the result is the fp32 kernel's to the bit -- a wrong k-mapping,
    swapped half, lost cross term or tail changes bits -- while dense_math = 1, which drops lo, must differ."""
    s, sk, _, _ = bc.layer(synth, eb, c)
    xd, n = _up(sk.x, dev), c.n_images
    for bias, relu in [(False, True)] if c.name == "b16_part" else [(False, False), (True, True)]:
        plan = _plan(pkg, s, sk.w, relu, dense_split=1)
        assert plan.stat("dense_split") == 0 and plan.stat("dense_variant") == 0            # no launch yet
        top = torch.full((s.N,) + tuple(_ref(c, s, sk, None)[0].shape[1:]), -7.5, device=dev)
        _bound_holds(plan, c, s, sk, xd, bias, relu, dev, top[:n])
        assert bool((top[n:] == -7.5).all()), "images past the call's were written"
        assert [plan.stat(k) for k in ("dense_split", "dense_math", "dense_variant", "streamk")] == [1, 1, c.variant + 128, 0]
        plan.set_option("dense_split", 0)
        bd = _up(sk.b, dev) if bias else None
        back = plan.forward(xd[:n], bd).clone()
        assert [plan.stat(k) for k in ("dense_split", "dense_math", "dense_variant")] == [0, 0, c.variant]
        fresh = _plan(pkg, s, sk.w, relu)
        assert torch.equal(back, fresh.forward(xd[:n], bd))
        fresh.close()
        plan.close()
    assert s.C // s.group * s.KH * s.KW <= 288
    rs = np.random.RandomState(sum(map(ord, c.name)))
    b = _up(rs.randint(-8, 9, s.M).astype(np.float32), dev)
    for wmax, xmax in ((3, 4095), (4095, 3)):
        x = _up(rs.randint(-xmax, xmax + 1, (n, s.C, s.H, s.W)).astype(np.float32), dev)
        plan = _plan(pkg, s, rs.randint(-wmax, wmax + 1, sk.w.shape).astype(np.float32), dense_split=1)
        got = plan.forward(x, b).clone()
        plan.set_option("dense_split", 0)
        want = plan.forward(x, b).clone()
        plan.set_option("dense_math", 1)
        assert not torch.equal(plan.forward(x, b), want), "bf16 rounding lost nothing: the inputs do not exercise lo"
        assert torch.equal(got, want), (c.name, wmax, (got != want).nonzero()[:1].tolist())
        plan.close()


@pytest.mark.parametrize("run,bottom_off,top_off,variant", lc.OFF_BOUNDARY, ids=["dn_pw64-" + o[0] for o in lc.OFF_BOUNDARY])
def test_blobs_off_a_16_byte_boundary(pkg, synth, dev, run, bottom_off, top_off, variant):
    """dn_pw64 with the bottom, then the top, 4 bytes off a 16-byte boundary inside a larger allocation: the gathered operand
    path, then scalar stores.  Around the bottom lie NaNs, of which none may reach the top; the top's surroundings stay."""
    c = next(k for k in bc.CASES if k.name == "dn_pw64")
    s, sk, _, _ = bc.layer(synth, eb, c)
    _, xw, _ = _window(sk.x.size, int(bottom_off), float("nan"), dev)
    xw.copy_(_up(sk.x, dev).reshape(-1))
    want = _ref(c, s, sk, sk.b)[0]
    tbuf, tw, around = _window(want.size, int(top_off), -7.5, dev)
    plan = _plan(pkg, s, sk.w, True, dense_split=1)
    _bound_holds(plan, c, s, sk, xw.view(sk.x.shape), True, True, dev, tw.view(want.shape))
    assert plan.stat("dense_variant") == variant + 128
    assert bool((tbuf[around] == -7.5).all()), (run, "the top's surroundings were written")
    plan.close()


def test_set_values_reaches_the_next_forward(pkg, synth, dev):
    """No stale weight copy: after set_values with no re-align the split forward is the new weights'."""
    c = next(k for k in bc.CASES if k.name == "dn_g128v")
    s, sk, _, _ = bc.layer(synth, eb, c)
    plan = _plan(pkg, s, (sk.w * np.float32(0.5) + np.float32(1.0)) * (sk.w != 0), dense_split=1)
    plan.forward(_up(sk.x, dev), None)
    plan.set_values(sk.w[sk.w != 0])
    _bound_holds(plan, c, s, sk, _up(sk.x, dev), True, False, dev)
    plan.close()


def test_inner_plan_of_b2s_runs_the_split_kernel(pkg, synth, dev):
    """Option "b2s" with a dense inner plan: the option is handed on, the inner plan's stats show the split kernel."""
    c = bc.Case("b16_ip", (130, 40, 1, 1, 24, 1), dict(sparsity=0.0), 130, 0, "an inner-product layer: the batch is the inner pixel axis")
    s, sk, _, _ = bc.layer(synth, eb, c)
    plan = _plan(pkg, s, sk.w, b2s=1, dense_split=1)
    assert plan.stat("b2s") == 1
    _bound_holds(plan, c, s, sk, _up(sk.x, dev), True, False, dev)
    assert plan.stat("dense_split") == 1 and plan.stat("dense_variant") >= 128
    plan.close()
