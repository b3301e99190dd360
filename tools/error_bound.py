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
product and a split-K fix-up add.  u = 2^-24 for a float plan and 2^-53 for a double plan.  ReLU is 1-Lipschitz:
max(want, 0) keeps the bound.

Subnormal inputs, weights and results are in scope (`edge_inputs`): no kernel may flush.  With gradual underflow a
product that lands below the smallest normal number is rounded to a multiple of tiny = 2^-149 (2^-1074 for a double
plan) and errs by at most tiny / 2 = 2^-150 instead of u x |product|; a sum of two numbers is exact whenever its result
is subnormal (both are multiples of tiny and so is their sum), and errs by u x |sum| otherwise.  A fused multiply-add
rounds once, by the larger of the two.  So the n products of an element add at most n * 2^-150 to the relative part, the
bias and a fix-up add nothing, and (n + 4) * tiny covers them with room to spare: that is the bound's last term, TINY
per dtype.

(For a double plan the float64 reference carries an error of the same order as the bound itself; an IEEE double kernel
can therefore reach a ratio of 2 against it in principle.  Sums of random signs stay near sqrt(n) u, far below.)

The edges of the number line (tests/test_fp32_edges_cpu.py, tests/test_fp32_edges_gpu.py): `edge_inputs` scales a
layer's inputs into the subnormal range or up to the top of the format, `flush_inputs` / `flush_results` are the two
models of a kernel that flushes (the self-check proves the inputs tell them from a right kernel), and the reach sets
say which outputs a non-finite input element may make non-finite.
"""
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
TINY = 2.0 ** -149          # the smallest subnormal float
TINY64 = 2.0 ** -1074       # ... and double


def tiny(f64=False):
    """The spacing of the subnormal range of the plan's dtype: the unit of the bound's last term."""
    return TINY64 if f64 else TINY

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


conv64 = _conv64       # the float64 convolution itself, for indicator and magnitude blobs


def row_nnz(w):
    return (np.asarray(w).reshape(w.shape[0], -1) != 0).sum(axis=1)


def forward_bound(s, w, x, b, relu=False, f64=False):
    """(want, B): the float64 forward and the bound of every output element, both (N, M, OH, OW) float64."""
    want = _conv64(x, w, b, s)
    mag = _conv64(np.abs(x), np.abs(w), None if b is None else np.abs(b), s)
    k = (row_nnz(w) + 4).astype(np.float64)[None, :, None, None]
    B = gamma(k, U64 if f64 else U32) * mag + k * tiny(f64)
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
    t = tiny(f64)
    Bs = (gamma(kd, u) * mag[0] + kd * t, gamma(kw, u) * mag[1] + kw * t,
          None if b is None else gamma(kw, u) * mag[2] + kw * t)
    return want, Bs


def accumulated_bound(B, base, n_terms, f64=False):
    """The bound of base + gradient where the kernel accumulated into a prefilled blob: the prefill is one more term
    of the sum, gamma(k + 1) * (S + |base|) with k = n_terms + 4, written in terms of B = gamma(k) * S + k * tiny."""
    u = U64 if f64 else U32
    k = float(n_terms + 4)
    return B * float(gamma(k + 1, u) / gamma(k, u)) + float(gamma(k + 1, u)) * np.abs(base) + tiny(f64)


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


# ---- the edges of the format: subnormal inputs, weights and results; sums next to the largest finite number ------------
EDGE_KINDS = ("sub_in", "sub_w", "sub_out", "near_max")
Edge = namedtuple("Edge", "w x b top_diff")
SUB_W_PATTERNS = (0x01, 0x02, 0x03, 0x04, 0x07, 0x08, 0x10, 0x11, 0x20, 0x3F, 0x40, 0x15)      # a dozen in 0x01 .. 0x40


def _ld(a, e):
    """a * 2^e in float64 (np.ldexp rounds once where the result is a subnormal double); e broadcasts against a."""
    return np.ldexp(np.asarray(a, np.float64), np.asarray(e, np.int64))


def _top_exponent(s0):
    """T with max(s0) * 2^T in [2^126, 2^127)."""
    m, e = np.frexp(float(np.max(s0)))      # max = m * 2^e, m in [0.5, 1): floor(log2 max) = e - 1
    assert m > 0, "near_max needs a nonzero sum of magnitudes"
    return 126 - (e - 1)


def edge_inputs(s, w, x, b, kind, seed, top_diff=None, f64=False):
    """Edge(w, x, b, top_diff): a layer's inputs (values of order 1, as synth gives them) scaled to an edge of the
    format; float32 arrays, float64 ones with `f64` -- the arrays handed to the kernel, and the ones the reference is
    computed from.  Every scaling is np.ldexp in float64 followed by one cast.  Exponents for float; a double plan's
    are these moved by E = 896 = 1023 - 127 (a product of two inputs: E / 2 each):
      sub_in    every bottom element x 2^-(127 + r), r seeded in [0, 12): all subnormal (or 0).  Weight row m x 2^8, 2^16 or
                2^24 (seeded per row), bias x 2^-130; top_diff like the bottom
      sub_w     every nonzero weight x 2^-(127 + r); a dozen of them are the bit patterns SUB_W_PATTERNS.  Bottom x 2^100,
                bias x 2^-20; top_diff as it is (of order 1: the data gradient is subnormal, and top_diff x bottom fits)
      sub_out   all inputs normal: bottom (and top_diff) x 2^-70, weight row m x 2^-66, 2^-70 or 2^-74, bias x 2^-136:
                every product, partial sum and result of the forward and of the data and weight gradient is subnormal or 0
      near_max  weights and bottom x 2^60, bias x 2^120; then weights and bias (with top_diff: top_diff, itself x 2^60
                first) by the one power of two that puts the largest sum of magnitudes S over the outputs (the three
                gradients) into [2^126, 2^127): whatever the order of the additions nothing can overflow"""
    assert kind in EDGE_KINDS, kind
    rs = np.random.RandomState(seed)
    E = 896 if f64 else 0
    dt = np.float64 if f64 else np.float32
    M = w.shape[0]
    row3 = rs.randint(0, 3, M)[:, None, None, None]
    rx = rs.randint(0, 12, x.shape)
    rw = rs.randint(0, 12, w.shape)
    rt = rs.randint(0, 12, top_diff.shape) if top_diff is not None else None
    pick = rs.choice(np.flatnonzero(np.asarray(w).ravel() != 0), len(SUB_W_PATTERNS), replace=False)
    td = None
    if kind == "sub_in":
        ws, xs = _ld(w, 8 * (row3 + 1)), _ld(x, -(127 + E + rx))
        bs = None if b is None else _ld(b, -(130 + E))
        td = None if top_diff is None else _ld(top_diff, -(127 + E + rt))
    elif kind == "sub_w":
        ws, xs = _ld(w, -(127 + E + rw)), _ld(x, 100 + E)
        bs = None if b is None else _ld(b, -20)
        td = None if top_diff is None else _ld(top_diff, 0)
    elif kind == "sub_out":
        ws, xs = _ld(w, -(66 + E // 2 + 4 * row3)), _ld(x, -(70 + E // 2))
        bs = None if b is None else _ld(b, -(136 + E))
        td = None if top_diff is None else _ld(top_diff, -(70 + E // 2))
    else:
        h = 60 + E // 2
        if top_diff is None:        # S = 2^T * (conv(|x|, |w|) + |b|): the shift is exact, so S0 of the plain inputs decides
            T = _top_exponent(_conv64(np.abs(x), np.abs(w), None if b is None else np.abs(b), s)) + E
            ws, xs = _ld(w, T - h), _ld(x, h)
            bs = None if b is None else _ld(b, T)
        else:
            # (every position of the weight blob: the dense weight gradient writes the pruned ones as well)
            mag = torch_backward(np.abs(x), np.abs(w), None, s, np.abs(top_diff), mask=np.ones(w.shape, bool))
            s0 = max(float(mag[0].max()), float(mag[1].max()), float(np.ldexp(np.abs(top_diff).sum(axis=(0, 2, 3)).max(), -h)))
            T = _top_exponent(s0) + E
            ws, xs, td = _ld(w, h), _ld(x, h), _ld(top_diff, T - h)
            bs = None if b is None else _ld(b, 2 * h)
    c = lambda a: None if a is None else np.ascontiguousarray(a.astype(dt))  # noqa: E731
    ws = c(ws)
    if kind == "sub_w":
        bits = np.array(SUB_W_PATTERNS, np.uint64 if f64 else np.uint32).view(dt)
        ws.ravel()[pick] = np.where(np.asarray(w).ravel()[pick] < 0, -bits, bits)
    out = Edge(ws, c(xs), c(bs), c(td))
    assert all(a is None or bool(np.isfinite(a).all()) for a in out), kind
    return out


def flush_inputs(a, f64=False):
    """What a kernel that flushes subnormal inputs reads: elements below the smallest normal number are 0."""
    a = np.asarray(a)
    return np.where(np.abs(a) < (2.0 ** -1022 if f64 else 2.0 ** -126), a.dtype.type(0), a)


def flush_results(want, f64=False):
    """What a kernel that flushes subnormal results writes, modelled on the reference."""
    return flush_inputs(np.asarray(want, np.float64), f64)


# ---- reach: the outputs a non-finite input element may make non-finite, from float64 convolutions of indicators ------------
def _ones_pattern(s):
    return np.ones((s.M, s.C // s.group, s.KH, s.KW), np.float64)


def reach_forward(s, pattern, poisoned):
    """The sparse reach: top elements that a nonzero of `pattern` (M x Cg x KH x KW) multiplies by a poisoned bottom
    element (`poisoned`: a boolean bottom blob)."""
    return _conv64(np.asarray(poisoned, np.float64), (np.asarray(pattern) != 0).astype(np.float64), None, s) > 0


def reach_forward_dense(s, poisoned):
    """The dense reach: every tap of every channel of the element's conv group counts."""
    return reach_forward(s, _ones_pattern(s), poisoned)


def reach_data(s, pattern, poisoned_top_diff):
    """bottom_diff elements that a nonzero of `pattern` multiplies by a poisoned top_diff element: the transposed
    convolution of the same indicators."""
    p = (np.asarray(pattern) != 0).astype(np.float64)
    x = np.zeros((poisoned_top_diff.shape[0], s.C, s.H, s.W))
    return torch_backward(x, p, None, s, np.asarray(poisoned_top_diff, np.float64), mask=p != 0)[0] > 0


def reach_data_dense(s, poisoned_top_diff):
    return reach_data(s, _ones_pattern(s), poisoned_top_diff)


def _positions(N, Cn, Hn, Wn, group, live):
    """The fixed list of poison_positions on a blob of N x Cn x Hn x Wn whose channels come in `group` conv groups; each
    moved to the nearest channel of `live` (a boolean per channel) inside its conv group, the lower one on a tie."""
    per = Cn // group
    mid = N // 2
    pos = [(0, 0, 0, 0), (N - 1, Cn - 1, Hn - 1, Wn - 1)]
    if N > 1:
        pos += [(0, Cn - 1, Hn - 1, Wn - 1), (1, 0, 0, 0)]
    if group > 1:
        pos += [(mid, per - 1, Hn // 2, Wn // 3), (mid, per, Hn // 2, Wn // 3)]
    pos += [(mid, Cn // 3, Hn // 2, Wn - 1), (mid, Cn // 2, Hn // 3, Wn // 2)]
    out = []
    for n, c, h, w in pos:
        g = c // per
        cand = [k for k in range(g * per, (g + 1) * per) if live[k]] or [k for k in range(Cn) if live[k]] or [c]
        c = min(cand, key=lambda k: (abs(k - c), k))
        if (n, c, h, w) not in out:
            out.append((n, c, h, w))
    return out


def poison_positions(s, pattern, n_images=None):
    """Where the reach tests poison the bottom blob, as (n, c, h, w): its first and its last element; (0, C-1, H-1, W-1)
    and (1, 0, 0, 0), neighbours in memory across an image boundary; on a grouped layer the last channel of conv group 0
    and the first of group 1; a row end (n, c, h, W-1) in a middle image; an interior element.  Each on the nearest input
    channel that has a nonzero, so that each reaches something."""
    p = np.asarray(pattern) != 0
    mg = p.shape[0] // s.group
    live = np.concatenate([p[g * mg:(g + 1) * mg].any(axis=(0, 2, 3)) for g in range(s.group)])
    return _positions(s.N if n_images is None else n_images, s.C, s.H, s.W, s.group, live)


def poison_positions_top(s, pattern, out_hw, n_images=None):
    """The same list on top_diff's axes (n, m, oh, ow), each on the nearest output channel whose row has a nonzero."""
    live = (np.asarray(pattern) != 0).any(axis=(1, 2, 3))
    return _positions(s.N if n_images is None else n_images, s.M, out_hw[0], out_hw[1], s.group, live)


def poisoned(shape, positions):
    """The boolean blob that is True at `positions`."""
    m = np.zeros(shape, bool)
    for p in positions:
        m[p] = True
    return m
