"""Plan option "wgrad_math" = bf16 on the MI355X: escoin_sconv_wgrad_bf16_kernel under wgrad_kernel = MFMA and
escoin_dense_wgrad_bf16_kernel under dense_wgrad, on the shapes of test_wgrad_bf16_host.py.

The reference is the float64 gradient of the operands rounded to bf16 in numpy (G masked by the real top > 0 first: zero
rounds to zero).  Products of two bf16 values are exact in fp32, so the bound is errbound.backward_bound's fp32 accumulation
bound on the rounded operands, unscaled; its term count N*OH*OW + 4 covers any summation order.  The worst ratio these
cases print is in profiles/wgrad_bf16_mi355x.md."""
import numpy as np
import pytest

import errbound as eb
import test_wgrad_bf16_host as wc
from dense_bf16_common import bf16_rne

torch = pytest.importorskip("torch")

from wgrad_common import csr_positions, seeded  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(pkg):
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        pytest.fail("no HIP device visible (these tests run on the MI355X)")
    return torch.device("cuda:0")


def _up(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def _window(dev, t):
    """`t` copied to one float past the start of a larger buffer: 4 bytes off a 16-byte boundary."""
    buf = torch.full((t.numel() + 8,), float("nan"), device=dev)
    buf[1:1 + t.numel()].copy_(t.reshape(-1))
    return buf[1:1 + t.numel()].view(t.shape)


def _plan(pkg, s, w, relu=False, **opts):
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu), wgrad_kernel=pkg.WGRAD_MFMA, **opts)
    plan.weight_align(w)
    return plan


def _both(plan, tdt, xt, top=None, n=None):
    """(values_diff, bias_diff, dense_wgrad) of the first n images, as bytes-comparable numpy arrays."""
    _, vd, bsd = plan.backward(tdt[:n], bottom=xt[:n], top=None if top is None else top[:n], bottom_diff=None, values_diff=True, bias_diff=True)
    dw = plan.dense_wgrad(tdt[:n], xt[:n], top=None if top is None else top[:n])
    torch.cuda.synchronize()
    return vd.cpu().numpy(), bsd.cpu().numpy(), dw.cpu().numpy()


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _ran(pkg, plan, math, variant=None):
    assert plan.stat("wgrad_kernel") == pkg.WGRAD_MFMA
    assert (plan.stat("wgrad_math"), plan.stat("dwg_math")) == (math, math)
    lds = wc.LDS if math else 2 * 2 * 32 * 65 * 4
    assert (plan.stat("wgrad_lds_bytes"), plan.stat("dwg_lds_bytes")) == (lds, lds)
    if variant is not None:
        assert (plan.stat("wgrad_math_variant"), plan.stat("dwg_math_variant")) == (variant, variant)


# ---- 1. error bound ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("name", list(wc.SHAPES))
def test_every_element_within_the_bound_of_the_rounded_operands(pkg, synth, dev, name, relu):
    """errbound.skew inputs; weight_diff, values_diff and dense_wgrad per element within the bound; NaN prefill outside the
    pattern untouched; compact == dense gathered; the stats; back at 0 the same plan gives a never-bf16 plan's bits; the bias
    gradient keeps its bits throughout."""
    s = wc.make(synth, name)
    w, x, b = synth.pruned_weights(s, 91), synth.activations(s, 92), synth.bias_vector(s, 93)
    sk = eb.skew(s, w, x, b, 95, top_diff=seeded((s.N, s.M) + synth.out_hw(s), 94))
    xd, bd, tdd = _up(dev, sk.x), _up(dev, sk.b), _up(dev, sk.top_diff)
    plan = _plan(pkg, s, sk.w, relu, wgrad_math=pkg.MATH_BF16)
    assert (plan.stat("wgrad_math"), plan.stat("dwg_math")) == (0, 0)          # no launch yet
    top = top_np = None
    if relu:
        top = plan.forward(xd, bd)
        torch.cuda.synchronize()
        top_np = top.cpu().numpy()
    want, Bs = eb.backward_bound(s, sk.w, bf16_rne(sk.x), sk.b, bf16_rne(sk.top_diff), top_np, mask=np.ones_like(sk.w, bool))
    want, B = want[1], Bs[1]
    fill = _up(dev, np.where(sk.w == 0, np.float32(np.nan), np.float32(0)))
    _, wd, _ = plan.backward(tdd, bottom=xd, top=top, bottom_diff=None, weight_diff=fill)
    vd, bsd, dw = _both(plan, tdd, xd, top)
    vec = wc.RULE[name][0] + 2 * wc.RULE[name][1]          # (torch's allocations are 16-byte aligned)
    _ran(pkg, plan, 1, vec)
    wd = wd.cpu().numpy()
    pat, pos, what = sk.w != 0, csr_positions(plan), (name, "relu", relu)
    assert np.all(np.isnan(wd[~pat])), what
    assert vd.tobytes() == wd.reshape(-1)[pos].tobytes(), what
    r = [eb.within(np.where(pat, wd, 0), want * pat, B, "wgrad_math 1", sk.td_row_exp, axis=0, what=what),
         eb.within(vd, want.reshape(-1)[pos], B.reshape(-1)[pos], "wgrad_math 1 compact", what=what),
         eb.within(dw, want, B, "wgrad_math 1 dense_wgrad", sk.td_row_exp, axis=0, what=what)]
    print("errbound wgrad_math bf16 %-10s relu=%d variant %d: weight %.3g, values %.3g, dense_wgrad %.3g" % ((name, relu, vec) + tuple(r)))
    plan.set_option("wgrad_math", 0)
    back = _both(plan, tdd, xd, top)
    _ran(pkg, plan, 0, 0)
    fresh = _plan(pkg, s, sk.w, relu)
    assert _same(back, _both(fresh, tdd, xd, top)), what
    assert back[1].tobytes() == bsd.tobytes(), what         # the bias gradient does not pass through the kernel
    fresh.close()
    plan.close()


# ---- 2. small integers: both math modes compute the same exact sums -----------------------------------------------------
@pytest.mark.parametrize("name", ["b_pw4", "d_3x3", "d_s2pw"])
def test_small_integers_equal_the_fp32_kernel_bit_for_bit(pkg, synth, dev, name):
    """Operands in [-3, 3] are bf16 exactly and every partial sum stays below 2^24: any wrong pixel mapping, swizzle, tail or
    mask changes bits."""
    s = wc.make(synth, name)
    rs = np.random.RandomState(sum(map(ord, name)))
    xt = _up(dev, rs.randint(-3, 4, (s.N, s.C, s.H, s.W)))
    tdt = _up(dev, rs.randint(-3, 4, (s.N, s.M) + synth.out_hw(s)))
    plan = _plan(pkg, s, synth.pruned_weights(s, 11), wgrad_math=pkg.MATH_BF16)
    got = _both(plan, tdt, xt)
    _ran(pkg, plan, 1)
    plan.set_option("wgrad_math", 0)
    want = _both(plan, tdt, xt)
    _ran(pkg, plan, 0)
    assert np.abs(want[2]).max() > 8 and _same(got, want), name
    plan.close()


# ---- 3. one sum order ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("b_pw4", None), ("b_3x3v", None), ("b_pw4x", 8)])
def test_staging_path_tiling_batch_stream_and_partial_batch(pkg, synth, dev, name, n):
    """Blobs passed as windows 4 bytes off a 16-byte boundary take the 4-byte loads: same bits; so do a side stream and
    tiling_batch = 256.  b_pw4x, 8 of 9 images (1152 pixels: the chunk boundary at pixel 16 of image 7, the last chunk 128 live
    pixels): the gradient of the first 8 images."""
    s = wc.make(synth, name)
    w, x, td = synth.pruned_weights(s, 11), synth.activations(s, 12), seeded((s.N, s.M) + synth.out_hw(s), 21)
    xt, tdt = _up(dev, x), _up(dev, td)
    plan = _plan(pkg, s, w, wgrad_math=pkg.MATH_BF16)
    aligned = _both(plan, tdt, xt, n=n)
    _ran(pkg, plan, 1, wc.RULE[name][0] + 2 * wc.RULE[name][1])
    windows = _both(plan, _window(dev, tdt), _window(dev, xt), n=n)
    _ran(pkg, plan, 1, 0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        streamed = _both(plan, tdt, xt, n=n)
    other = _plan(pkg, s, w, wgrad_math=pkg.MATH_BF16, tiling_batch=256)
    assert _same(aligned, windows) and _same(aligned, streamed) and _same(aligned, _both(other, tdt, xt, n=n)), name
    if n is not None:
        want, Bs = eb.backward_bound(s, w, bf16_rne(x[:n]), None, bf16_rne(td[:n]), mask=np.ones_like(w, bool))
        pos = csr_positions(plan)
        eb.within(aligned[2], want[1], Bs[1], "wgrad_math 1 dense_wgrad", what=(name, n))
        eb.within(aligned[0], want[1].reshape(-1)[pos], Bs[1].reshape(-1)[pos], "wgrad_math 1 compact", what=(name, n))
        assert plan.stat("bwd_chunks") == 2
    other.close()
    plan.close()


# ---- 4. non-finite operand ----------------------------------------------------------------------------------------------
def test_non_finite_bottom_reaches_only_the_entries_whose_tap_reads_it(pkg, synth, dev):
    s = wc.make(synth, "d_3x3")
    w, x, td = synth.pruned_weights(s, 11), synth.activations(s, 12), seeded((s.N, s.M) + synth.out_hw(s), 21)
    c = 7
    x_inf = x.copy()
    x_inf[1, c, 0, 0] = np.inf
    plan = _plan(pkg, s, w, wgrad_math=pkg.MATH_BF16)
    clean = _both(plan, _up(dev, td), _up(dev, x))[0]
    dirty = _both(plan, _up(dev, td), _up(dev, x_inf))[0]
    _ran(pkg, plan, 1)
    # pixel (0, 0) is read by output pixel (pad - kr, pad - kc): inside the image for kr, kc <= pad = 1
    col = plan.get_csr()[1]
    hit = (col // 9 == c) & ((col // 3) % 3 <= 1) & (col % 3 <= 1)
    assert hit.sum() > 0 and (~hit).sum() > 0
    assert not np.any(np.isfinite(dirty[hit]))
    assert dirty[~hit].tobytes() == clean[~hit].tobytes()
    plan.close()
