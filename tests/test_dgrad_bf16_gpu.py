"""Plan option "dgrad_math" = bf16 on the MI355X: escoin_sconv_dgrad_bf16_kernel under backward_kernel = BWD_MFMA, on the
shapes of test_dgrad_bf16_host.py (emptyblock: live steps {0, 2}, a pair of non-adjacent steps; pw_s2: two steps, two
channel tiles, a pixel tile across image boundaries; the 3x3 cases: one step, a bare tail; steps3: a pair and an odd tail).

The reference is the float64 gradient of the operands rounded to bf16 in numpy (top_diff masked by the real top > 0: zero
rounds to zero).  Products of two bf16 values are exact in fp32, so the bound is errbound.backward_bound's fp32 accumulation
bound on the rounded operands, unscaled.  The worst ratio these cases print is in profiles/dgrad_bf16_mi355x.md."""
import ctypes

import numpy as np
import pytest

import dgrad_mfma_common as dc
import errbound as eb
import test_dgrad_bf16_host as hc
from dense_bf16_common import bf16_rne
from upd_common import new_weights, same_bits

torch = pytest.importorskip("torch")

from wgrad_common import seeded  # noqa: E402

pytestmark = pytest.mark.gpu
LDS = {0: 2 * 2 * 32 * 65 * 4, 1: hc.LDS}


@pytest.fixture(scope="module")
def dev(pkg):
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        pytest.fail("no HIP device visible (these tests run on the MI355X)")
    return torch.device("cuda:0")


_CASES = {}


def _case(synth, name):
    """(shape, skewed inputs) of a shape: made once, never written."""
    if name not in _CASES:
        s = hc.make(synth, name)
        td = seeded((s.N, s.M) + synth.out_hw(s), 21)
        _CASES[name] = (s, eb.skew(s, dc.weights(synth, s), synth.activations(s, 12), synth.bias_vector(s, 13), 95, top_diff=td))
    return _CASES[name]


def _up(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def _window(dev, t):
    """`t` copied to one float past the start of a larger buffer: 4 bytes off a 16-byte boundary."""
    buf = torch.full((t.numel() + 8,), float("nan"), device=dev)
    buf[1:1 + t.numel()].copy_(t.reshape(-1))
    return buf[1:1 + t.numel()].view(t.shape)


def _plan(pkg, s, w, relu=False, **opts):
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu), backward_kernel=pkg.BWD_MFMA, **opts)
    plan.weight_align(w)
    return plan


def _dgrad(pkg, plan, s, tdt, math, top=None, out=None, n=None):
    """bottom_diff of the first n images (default: all) written into `out` (default: a NaN-filled blob) through the C entry
    point, as numpy; asserts which kernel ran."""
    out = torch.full((s.N, s.C, s.H, s.W), float("nan"), device=tdt.device) if out is None else out
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    pkg.check(pkg.lib().escoin_backward(plan._h, None, ptr(top), ptr(tdt), ptr(out), None, None, s.N if n is None else n, stream),
              "escoin_backward")
    torch.cuda.synchronize()
    if n != 0:
        assert plan.stat("bwd_data_kernel") == pkg.BWD_MFMA
        assert (plan.stat("dgrad_math"), plan.stat("dgrad_lds_bytes")) == (math, LDS[math])
    return out.cpu().numpy()


# ---- 1. error bound ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("name", list(hc.SHAPES))
def test_every_element_within_the_bound_of_the_rounded_operands(pkg, synth, dev, name, relu):
    """errbound.skew inputs; every element of bottom_diff, written into a NaN-filled blob, within the bound; the stats; back
    at 0 the same plan gives a never-bf16 plan's bits."""
    s, sk = _case(synth, name)
    tdd = _up(dev, sk.top_diff)
    plan = _plan(pkg, s, sk.w, relu, dgrad_math=pkg.MATH_BF16)
    assert plan.stat("dgrad_math") == 0                     # no launch yet
    top = top_np = None
    if relu:
        top = plan.forward(_up(dev, sk.x), _up(dev, sk.b))
        torch.cuda.synchronize()
        top_np = top.cpu().numpy()
    want, Bs = eb.backward_bound(s, bf16_rne(sk.w), sk.x, sk.b, bf16_rne(sk.top_diff), top_np)
    got = _dgrad(pkg, plan, s, tdd, 1, top)
    r = eb.within(got, want[0], Bs[0], "dgrad_math 1", sk.chan_exp, what=(name, "relu", relu))
    print("errbound dgrad_math bf16 %-12s relu=%d: %.3g" % (name, relu, r))
    plan.set_option("dgrad_math", 0)
    back = _dgrad(pkg, plan, s, tdd, 0, top)
    fresh = _plan(pkg, s, sk.w, relu)
    assert same_bits(back, _dgrad(pkg, fresh, s, tdd, 0, top)), (name, relu)
    fresh.close()
    plan.close()


# ---- 2. small integers: both math modes compute the same exact sums -----------------------------------------------------
@pytest.mark.parametrize("name", ["pw_s2", "3x3_s2x3_g2", "emptyblock", "steps3"])
def test_small_integers_equal_the_fp32_kernel_bit_for_bit(pkg, synth, dev, name):
    """Operands in [-3, 3] are bf16 exactly and every partial sum stays below 2^24: any wrong column pairing, swizzle, tail or
    mask changes bits."""
    s = hc.make(synth, name)
    rs = np.random.RandomState(sum(map(ord, name)))
    w = np.where(dc.weights(synth, s) != 0, rs.randint(-3, 4, (s.M, s.C // s.group, s.KH, s.KW)), 0).astype(np.float32)
    tdt = _up(dev, rs.randint(-3, 4, (s.N, s.M) + synth.out_hw(s)))
    plan = _plan(pkg, s, w, dgrad_math=pkg.MATH_BF16)
    got = _dgrad(pkg, plan, s, tdt, 1)
    plan.set_option("dgrad_math", 0)
    want = _dgrad(pkg, plan, s, tdt, 0)
    assert np.abs(want).max() > 8 and same_bits(got, want), name
    plan.close()


# ---- 3. one sum order ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pw_s2", "3x3_s2x3_g2"])
def test_partial_batches_windows_and_a_side_stream_give_the_same_bits(pkg, synth, dev, name):
    """n_images in (0, N - 1, 1) leaves the other images NaN and gives the first n images of the full-batch call bit for bit;
    so do blobs passed as windows 4 bytes off a 16-byte boundary, and a side stream."""
    s, sk = _case(synth, name)
    tdd = _up(dev, sk.top_diff)
    plan = _plan(pkg, s, sk.w, dgrad_math=pkg.MATH_BF16)
    full = _dgrad(pkg, plan, s, tdd, 1)
    assert np.all(np.isfinite(full)) and np.abs(full).max() > 0
    for n in (0, s.N - 1, 1):
        assert 0 <= n < s.N
        got = _dgrad(pkg, plan, s, tdd, 1, n=n)
        assert np.all(np.isnan(got[n:])) and same_bits(got[:n], full[:n]), (name, n)
    nan = torch.full((s.N, s.C, s.H, s.W), float("nan"), device=dev)
    assert same_bits(_dgrad(pkg, plan, s, _window(dev, tdd), 1, out=_window(dev, nan)), full), name
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert same_bits(_dgrad(pkg, plan, s, tdd, 1), full), name
    plan.close()


# ---- 4. in-place update ------------------------------------------------------------------------------------------------------
def test_update_values_reaches_the_bf16_kernel_without_a_new_align(pkg, synth, dev):
    """The option holds no state: after update_values the bf16 data gradient equals, bit for bit, that of a fresh plan
    aligned on the new weights."""
    s, sk = _case(synth, "pw_s2")
    tdd = _up(dev, sk.top_diff)
    plan = _plan(pkg, s, sk.w, dgrad_math=pkg.MATH_BF16)
    before = _dgrad(pkg, plan, s, tdd, 1)
    w1, w1_nan = new_weights(sk.w, 43, zeros=False)
    plan.update_values(_up(dev, w1_nan))
    assert plan.stat("update_fast") == 1
    got = _dgrad(pkg, plan, s, tdd, 1)
    fresh = _plan(pkg, s, w1, dgrad_math=pkg.MATH_BF16)
    assert same_bits(got, _dgrad(pkg, fresh, s, tdd, 1)) and not same_bits(got, before)
    fresh.close()
    plan.close()
