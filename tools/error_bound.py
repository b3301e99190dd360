"""A float64 reference and a derived per-element error bound for the forward and the Backward: the suite has it as
tests/errbound.py (test_errbound_cpu.py, test_errbound_gpu.py); it lives here because tools/fuzz_parity.py and
tools/fuzz_backward.py use it too, and a tool must run whatever the tests directory next to it holds beyond the shared
helpers it already imports (wgrad_common).

conftest.rel_err is a max-norm over the tensor: an output element that is small next to the tensor's largest one is not
checked by it.  Here every element has its own bound, and `skew` gives the rows, input channels and images of a workload
scales that differ by up to 2^48, so that a dropped bias, a value leaked from a neighbouring row or two swapped images
show on the small elements.

The bound is derived, not measured.  An output element of channel m is a sum of n_m products (the nonzeros of row m;
zero weights and padding taps add exact zeros) plus the bias.  In IEEE arithmetic with unit roundoff u, whatever the
order of the additions and whether or not product and add are fused, each term passes through at most n_m roundings, so
    |got - exact| <= gamma(n_m + 4) * S,   gamma(k) = k u / (1 - k u),   S = sum of the magnitudes of the terms
(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).  The extra 4 covers the bias add, the unfused
product and a split-K fix-up add; (n_m + 4) * 2^-149 covers a result in the subnormal range.  u = 2^-24 for a float plan
and 2^-53 for a double plan.  ReLU is 1-Lipschitz: max(want, 0) keeps the bound.  Denormal INPUTS are out of scope: with
synth's values under `skew` no product or partial sum leaves the normal fp32 range.

(For a double plan the float64 reference carries an error of the same order as the bound itself; an IEEE double kernel
can therefore reach a ratio of 2 against it in principle.  Sums of random signs stay near sqrt(n) u, far below.)"""
import os
import sys
from collections import namedtuple

import numpy as np
import torch

_TESTS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests")
if _TESTS not in sys.path:
    sys.path.insert(0, _TESTS)
from wgrad_common import torch_backward  # noqa: E402

F = torch.nn.functional

U32 = 2.0 ** -24
U64 = 2.0 ** -53
TINY = 2.0 ** -149
ROW_EXPONENTS = (-24, -12, 0, 12, 24)
CHANNEL_EXPONENT = 8        # input channels: 2^f, f in [-8, 8]
IMAGE_EXPONENT = 10         # images: 2^g, g in [-10, 10]

Skewed = namedtuple("Skewed", "w x b top_diff row_exp chan_exp img_exp td_row_exp td_img_exp")


def gamma(k, u=U32):
    k = np.asarray(k, np.float64)
    return k * u / (1.0 - k * u)


def _pow2(e, dt):
    return np.ldexp(1.0, np.asarray(e, np.int64)).astype(dt)


def _row_exponents(rs, m):
    """Each of ROW_EXPONENTS on (nearly) the same number of rows, in a seeded order: every skewed layer has rows at
    both ends of the range, whatever the seed."""
    return rs.permutation(np.resize(np.array(ROW_EXPONENTS, np.int64), m))


def _image_exponents(rs, n):
    """n exponents spread evenly over [-IMAGE_EXPONENT, IMAGE_EXPONENT] in a seeded order: a batch of two or more has an
    image at each end, so a bias (which no image scale multiplies) is large next to the sum on one image and small on
    another."""
    if n == 1:
        return rs.randint(-IMAGE_EXPONENT, IMAGE_EXPONENT + 1, 1)
    return rs.permutation(np.rint(np.linspace(-IMAGE_EXPONENT, IMAGE_EXPONENT, n)).astype(np.int64))


def skew(s, w, x, b, seed, top_diff=None):
    """w, x, b (and top_diff) scaled by exact powers of two: weight row m and its bias by 2^e_m, e_m from ROW_EXPONENTS;
    input channel c by 2^f_c, |f_c| <= 8; image n by 2^g_n, |g_n| <= 10; top_diff's channels and images by exponents of
    their own from the same ranges.  The dtypes are kept and every value stays exact.  `s` gives the layer's sizes."""
    rs = np.random.RandomState(seed)
    M, Cc, N = w.shape[0], x.shape[1], x.shape[0]
    assert (M, Cc) == (s.M, s.C) and N <= s.N, "w, x are not this layer's"
    e = _row_exponents(rs, M)
    f = rs.randint(-CHANNEL_EXPONENT, CHANNEL_EXPONENT + 1, Cc)
    g = _image_exponents(rs, N)
    te = _row_exponents(rs, M)
    tg = _image_exponents(rs, N)
    ws = w * _pow2(e, w.dtype)[:, None, None, None]
    xs = x * _pow2(f, x.dtype)[None, :, None, None] * _pow2(g, x.dtype)[:, None, None, None]
    bs = None if b is None else b * _pow2(e, b.dtype)
    tds = None
    if top_diff is not None:
        tds = top_diff * _pow2(te, top_diff.dtype)[None, :, None, None] * _pow2(tg[:top_diff.shape[0]], top_diff.dtype)[:, None, None, None]
    return Skewed(np.ascontiguousarray(ws), np.ascontiguousarray(xs), bs, tds, e, f, g, te, tg)


def _conv64(x, w, b, s):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float64))  # noqa: E731
    return F.conv2d(t(x), t(w), t(b), stride=(s.stride_h, s.stride_w), padding=(s.pad_h, s.pad_w),
                    dilation=(s.dil_h, s.dil_w), groups=s.group).numpy()


def row_nnz(w):
    return (np.asarray(w).reshape(w.shape[0], -1) != 0).sum(axis=1)


def forward_bound(s, w, x, b, relu=False, f64=False):
    """(want, B): the float64 forward and the bound of every output element, both (N, M, OH, OW) float64."""
    want = _conv64(x, w, b, s)
    mag = _conv64(np.abs(x), np.abs(w), None if b is None else np.abs(b), s)
    k = (row_nnz(w) + 4).astype(np.float64)[None, :, None, None]
    B = gamma(k, U64 if f64 else U32) * mag + k * TINY
    if relu:
        want = np.maximum(want, 0.0)
    return want, B


def backward_bound(s, w, x, b, top_diff, top=None, f64=False, mask=None):
    """((bottom_diff, weight_diff, bias_diff), (B_bottom, B_weight, B_bias)) in float64: wgrad_common.torch_backward on
    the inputs and on their magnitudes (top_diff masked by [top > 0] in both).  Terms per element -- data gradient of
    input channel c: the nonzeros of the taps that read c; a weight entry and a bias: n_images * OH * OW.  `mask`: the
    plan's pattern where it holds explicit zeros (default: w != 0)."""
    u = U64 if f64 else U32
    pattern = (np.asarray(w) != 0) if mask is None else mask
    want = torch_backward(x, w, b, s, top_diff, top, mask=pattern)
    mag = torch_backward(np.abs(x), np.abs(w), None if b is None else np.abs(b), s, np.abs(top_diff), top, mask=pattern)
    mg = w.shape[0] // s.group
    taps = np.concatenate([pattern[g * mg:(g + 1) * mg].sum(axis=(0, 2, 3)) for g in range(s.group)])
    kd = (taps + 4).astype(np.float64)[None, :, None, None]
    kw = float(top_diff.shape[0] * top_diff.shape[2] * top_diff.shape[3] + 4)
    Bs = (gamma(kd, u) * mag[0] + kd * TINY, gamma(kw, u) * mag[1] + kw * TINY,
          None if b is None else gamma(kw, u) * mag[2] + kw * TINY)
    return want, Bs


def accumulated_bound(B, base, n_terms, f64=False):
    """The bound of base + gradient where the kernel accumulated into a prefilled blob: the prefill is one more term
    of the sum, gamma(k + 1) * (S + |base|) with k = n_terms + 4, written in terms of B = gamma(k) * S + k * 2^-149."""
    u = U64 if f64 else U32
    k = float(n_terms + 4)
    return B * float(gamma(k + 1, u) / gamma(k, u)) + float(gamma(k + 1, u)) * np.abs(base) + TINY


def check(got, want, B):
    """(worst |got - want| / B, its index).  A NaN or an infinity in `got` counts as an infinite ratio."""
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape == B.shape, (got.shape, want.shape, B.shape)
    if got.size == 0:
        return 0.0, ()
    with np.errstate(invalid="ignore", over="ignore"):
        ratio = np.abs(got - want) / B
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    idx = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[idx]), tuple(int(i) for i in idx)


def within(got, want, B, kernel="", exps=None, axis=1, what="", worst=None):
    """Asserts check() <= 1 and returns the ratio.  The message names the element, the ratio, the kernel and the scale
    exponent of the element's row (`exps` indexed by the element's coordinate on `axis`).  `worst`: a dict that keeps the
    largest ratio seen per kernel name."""
    ratio, idx = check(got, want, B)
    if worst is not None:
        worst[kernel] = max(worst.get(kernel, 0.0), ratio)
    if not ratio <= 1.0:
        e = "" if exps is None or len(idx) <= axis else ", scale exponent %d" % int(exps[idx[axis]])
        raise AssertionError("%s via %s: element %s is off by %.3g x its bound (got %r, want %r, bound %.3g%s)" %
                             (what, kernel, idx, ratio, float(np.asarray(got)[idx]), float(want[idx]), float(B[idx]), e))
    return ratio


# ---- the three corruptions of test_errbound_cpu.py's self-check (also what a reverted kernel line looks like) --------
def low_channels(want):
    """Output channels ordered by magnitude, lowest first; the lowest quarter is the first M // 4 of them."""
    mag = np.abs(want).max(axis=(0, 2, 3))
    return np.argsort(mag, kind="stable"), mag


def corruption_target(want, w, b, gap=2.0 ** 20):
    """(m, src): the channel the self-check corrupts and the neighbour it leaks from.  m is the lowest-magnitude channel
    of the lowest quarter that has nonzeros and a bias, src its neighbour (m - 1 or m + 1: rows that share a wave or a
    quad are adjacent) of the larger magnitude.  Where that neighbour is not `gap` times larger, the pair of the quarter
    with the largest gap -- again among channels with nonzeros and a bias only: an empty row's channel holds its bias on
    every image (swapping two of them changes nothing), and a rule that takes the largest gap alone lands on such rows at
    95 % sparsity.  If the quarter has no such channel, the lowest one that has is taken from the rest."""
    order, mag = low_channels(want)
    M = len(order)
    nnz = row_nnz(w)
    live = [int(m) for m in order if nnz[m] > 0 and b is not None and b[m] != 0]
    assert live, "no output channel has both nonzeros and a bias"
    quarter = set(int(m) for m in order[:max(1, M // 4)])
    cand = [m for m in live if m in quarter] or live[:1]

    def pairs(ms):
        return [(m, n) for m in ms for n in (m - 1, m + 1) if 0 <= n < M]

    m, src = max(pairs(cand[:1]), key=lambda p: mag[p[1]])
    if mag[src] < gap * mag[m]:
        m, src = max(pairs(cand), key=lambda p: mag[p[1]] / max(mag[p[0]], 1e-300))
    return int(m), int(src)


def drop_bias(out, b, m):
    c = out.copy()
    c[:, m] = (c[:, m].astype(np.float64) - float(b[m])).astype(out.dtype)
    return c


def leak_from(out, m, src, exp=-30):
    """Channel m receives 2^exp of channel src (a cross-row leak inside a wave or a quad)."""
    c = out.copy()
    c[:, m] = (c[:, m].astype(np.float64) + np.ldexp(out[:, src].astype(np.float64), exp)).astype(out.dtype)
    return c


def swap_images(out, m, a=0, b=1):
    c = out.copy()
    c[a, m], c[b, m] = out[b, m].copy(), out[a, m].copy()
    return c
