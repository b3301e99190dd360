"""Plan option "dense_math" = bf16 on the MI355X: escoin_dense_bf16_kernel under KERNEL_DENSE on the cases of
dense_bf16_common.py and the two off-boundary runs of layout_cases.py.

The reference is the float64 convolution of the operands rounded to bf16 in numpy.  Products of two bf16 values are exact
in fp32, so the bound is errbound.forward_bound's fp32 accumulation bound on the rounded operands, unscaled: the worst
ratio measured over these cases is in profiles/dense_bf16_mi355x.md."""
import numpy as np
import pytest

import dense_bf16_common as bc
import errbound as eb
import layout_cases as lc
from test_errbound_gpu import _up, dev  # noqa: F401
from test_errbound_layouts_gpu import _window

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
_REFS = {}


def _ref(c, s, w_r, x_r, b):
    """want, B of the rounded operands without ReLU, once per (case, bias); ReLU is 1-Lipschitz and keeps the bound."""
    key = (c.name, b is not None)
    if key not in _REFS:
        _REFS[key] = eb.forward_bound(s, w_r, x_r, b)
    return _REFS[key]


def _plan(pkg, s, w, relu=False, **opts):
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu), kernel=pkg.KERNEL_DENSE, **opts)
    plan.weight_align(w)
    return plan


def _bound_holds(plan, c, s, sk, w_r, x_r, xd, bias, relu, dev, top=None):
    want, B = _ref(c, s, w_r, x_r, sk.b if bias else None)
    n = c.n_images
    got = plan.forward(xd[:n], _up(sk.b, dev) if bias else None, top)
    torch.cuda.synchronize()
    want = np.maximum(want[:n], 0.0) if relu else want[:n]
    r = eb.within(got.cpu().numpy(), want, B[:n], "escoin_dense_bf16_kernel", sk.row_exp, what=(c.name, "bias", bias, "relu", relu))
    print("dense_bf16 %-9s bias=%d relu=%d: worst err / bound %.3g" % (c.name, bias, relu, r))
    return got


@pytest.mark.parametrize("c", bc.CASES, ids=bc.IDS)
def test_bound_variant_exactness_and_the_way_back_to_fp32(pkg, synth, dev, c):
    """Per element within the fp32 accumulation bound of the rounded operands, with and without bias and ReLU (b16_part:
    ReLU, no bias, two of three images, the third untouched); stats "dense_math" 1 and "dense_variant" + 32; with the option
    back at 0 the same plan reports the fp32 variant and gives a fresh fp32 plan's bits."""
    s, sk, w_r, x_r = bc.layer(synth, eb, c)
    xd, n = _up(sk.x, dev), c.n_images
    runs = [(False, True)] if c.name == "b16_part" else [(False, False), (True, True)]
    for bias, relu in runs:
        plan = _plan(pkg, s, sk.w, relu, dense_math=1)
        assert plan.stat("dense_math") == 0 and plan.stat("dense_variant") == 0            # no launch yet
        top = torch.full((s.N,) + tuple(_ref(c, s, w_r, x_r, None)[0].shape[1:]), -7.5, device=dev)
        _bound_holds(plan, c, s, sk, w_r, x_r, xd, bias, relu, dev, top[:n])
        assert bool((top[n:] == -7.5).all()), "images past the call's were written"
        assert (plan.stat("dense_math"), plan.stat("dense_variant"), plan.stat("streamk")) == (1, c.variant + 32, 0)
        plan.set_option("dense_math", 0)
        bd = _up(sk.b, dev) if bias else None
        back = plan.forward(xd[:n], bd).clone()
        assert (plan.stat("dense_math"), plan.stat("dense_variant")) == (0, c.variant)
        fresh = _plan(pkg, s, sk.w, relu)
        assert torch.equal(back, fresh.forward(xd[:n], bd))
        fresh.close()
        plan.close()
    # small integers (weights in [-3, 3], activations in [-4, 4]: bf16 exactly, every partial sum below 2^24): both math modes
    # compute the same exact sums, so any wrong k-mapping, swizzle or tail changes bits
    rs = np.random.RandomState(sum(map(ord, c.name)))
    x = _up(rs.randint(-4, 5, (n, s.C, s.H, s.W)).astype(np.float32), dev)
    b = _up(rs.randint(-8, 9, s.M).astype(np.float32), dev)
    plan = _plan(pkg, s, rs.randint(-3, 4, sk.w.shape).astype(np.float32), dense_math=1)
    got = plan.forward(x, b).clone()
    plan.set_option("dense_math", 0)
    want = plan.forward(x, b)
    assert float(want.abs().max()) > 8 and torch.equal(got, want), (c.name, (got != want).nonzero()[:1].tolist())
    plan.close()


@pytest.mark.parametrize("run,bottom_off,top_off,variant", lc.OFF_BOUNDARY, ids=["dn_pw64-" + o[0] for o in lc.OFF_BOUNDARY])
def test_blobs_off_a_16_byte_boundary(pkg, synth, dev, run, bottom_off, top_off, variant):
    """dn_pw64 with the bottom, then the top, 4 bytes off a 16-byte boundary inside a larger allocation: the gathered operand
    path, then scalar stores.  Around the bottom lie NaNs, of which none may reach the top; the top's surroundings stay."""
    c = next(k for k in bc.CASES if k.name == "dn_pw64")
    s, sk, w_r, x_r = bc.layer(synth, eb, c)
    _, xw, _ = _window(sk.x.size, int(bottom_off), float("nan"), dev)
    xw.copy_(_up(sk.x, dev).reshape(-1))
    want = _ref(c, s, w_r, x_r, sk.b)[0]
    tbuf, tw, around = _window(want.size, int(top_off), -7.5, dev)
    plan = _plan(pkg, s, sk.w, True, dense_math=1)
    _bound_holds(plan, c, s, sk, w_r, x_r, xw.view(sk.x.shape), True, True, dev, tw.view(want.shape))
    assert plan.stat("dense_variant") == variant + 32
    assert bool((tbuf[around] == -7.5).all()), (run, "the top's surroundings were written")
    plan.close()


def test_set_values_reaches_the_next_forward(pkg, synth, dev):
    """No stale weight copy: after set_values with no re-align the bf16 forward is the new weights'."""
    c = next(k for k in bc.CASES if k.name == "dn_g128v")
    s, sk, w_r, x_r = bc.layer(synth, eb, c)
    plan = _plan(pkg, s, (sk.w * np.float32(0.5) + np.float32(1.0)) * (sk.w != 0), dense_math=1)
    plan.forward(_up(sk.x, dev), None)
    plan.set_values(sk.w[sk.w != 0])
    _bound_holds(plan, c, s, sk, w_r, x_r, _up(sk.x, dev), True, False, dev)
    plan.close()


def test_inner_plan_of_b2s_runs_the_bf16_kernel(pkg, synth, dev):
    """Option "b2s" with a dense inner plan: the option is handed on, the inner plan's stats show the bf16 kernel."""
    c = bc.Case("b16_ip", (130, 40, 1, 1, 24, 1), dict(sparsity=0.0), 130, 0, "an inner-product layer: the batch is the inner pixel axis")
    s, sk, w_r, x_r = bc.layer(synth, eb, c)
    plan = _plan(pkg, s, sk.w, b2s=1, dense_math=1)
    assert plan.stat("b2s") == 1
    _bound_holds(plan, c, s, sk, w_r, x_r, _up(sk.x, dev), True, False, dev)
    assert plan.stat("dense_math") == 1 and plan.stat("dense_variant") >= 32
    plan.close()
