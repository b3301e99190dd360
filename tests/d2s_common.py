"""Shared by test_d2s_host.py, test_d2s_cpu.py, test_d2s_gpu.py and test_shim_d2s.py -- and, through plan_model.DeconvModel,
d2s_seq_common.py, d2s_edges_common.py and large_common.py, by the sequence, fp32-edge and large-blob suites: the Deconvolution layers plan option
"deconv" is tested on -- the smallest at which each piece (the inner CSR and its entry map, the pack / unpack kernels' phase
arithmetic, the crop, the inner kernels) can still go wrong --, a seeded slice of random geometries, the decomposition of
include/escoin.h "Deconvolution" restated in numpy from the contract's formulas, the torch float64 reference, and the
error bound of errbound.py evaluated on the inner stride-1 layer, which is the layer that runs."""
from collections import namedtuple

import numpy as np

DShape = namedtuple("DShape", "name N C H W M KH KW stride_h stride_w pad_h pad_w group")

# name: (N, C, M, H, W, (KH, KW), (sh, sw), (ph, pw), group)
SHAPES = {
    "k4s2p1": (3, 8, 6, 5, 7, (4, 4), (2, 2), (1, 1), 1),          # the common decoder layer; crop on both sides
    "k3s2p1": (2, 5, 7, 6, 5, (3, 3), (2, 2), (1, 1), 1),          # phases with different tap counts; zero positions in the inner kernel
    "k3x2_s2x3": (2, 4, 4, 5, 4, (3, 2), (2, 3), (0, 1), 1),       # axes differ; sw > KW: phases without taps
    "k2s2": (2, 6, 4, 7, 7, (2, 2), (2, 2), (0, 0), 1),            # KH' = 1: pointwise inner plan
    "k1s2_bias_relu": (2, 4, 4, 4, 4, (1, 1), (2, 2), (0, 0), 1),  # three of four phases are bias only
    "k5s3p2_g2": (2, 6, 8, 4, 5, (5, 5), (3, 3), (2, 2), 2),       # groups; K not a multiple of s
    "k3s1p1": (2, 4, 5, 6, 6, (3, 3), (1, 1), (1, 1), 1),          # P = 1: the flipped convolution
    "k3s1p0": (2, 4, 5, 6, 6, (3, 3), (1, 1), (0, 0), 1),
    "k2s2p2": (1, 3, 3, 5, 5, (2, 2), (2, 2), (2, 2), 1),          # pad above K - 1: the crop removes whole inner rows
    "depthwise": (2, 4, 4, 6, 6, (4, 4), (2, 2), (1, 1), 4),       # FCN bilinear: Cg = Mg = 1
    "wide": (1, 2, 2, 3, 258, (4, 4), (2, 2), (1, 1), 1),          # W' > 256: the inner plan leaves the tiled kernels
}


def make(name):
    N, C, M, H, W, k, st, pd, g = SHAPES[name]
    return DShape(name, N, C, H, W, M, k[0], k[1], st[0], st[1], pd[0], pd[1], g)


def out_hw(s):
    return s.stride_h * (s.H - 1) + s.KH - 2 * s.pad_h, s.stride_w * (s.W - 1) + s.KW - 2 * s.pad_w


def random_shapes(count=200, seed=20262):
    """`count` seeded geometries: stride 1-4 and kernel 1-6 per axis, pad 0-3, groups 1-3; those without a top pixel are
    drawn again."""
    rs = np.random.RandomState(seed)
    out = []
    while len(out) < count:
        g = int(rs.randint(1, 4))
        s = DShape("d2s_rand%03d" % len(out), int(rs.randint(1, 3)), g * int(rs.randint(1, 4)), int(rs.randint(1, 7)), int(rs.randint(1, 7)),
                   g * int(rs.randint(1, 4)), int(rs.randint(1, 7)), int(rs.randint(1, 7)), int(rs.randint(1, 5)), int(rs.randint(1, 5)),
                   int(rs.randint(0, 4)), int(rs.randint(0, 4)), g)
        # (the descriptor is created as a convolution's before the option is set: it needs a convolution output too)
        if min(out_hw(s)) >= 1 and s.H + 2 * s.pad_h >= s.KH and s.W + 2 * s.pad_w >= s.KW:
            out.append(s)
    return out


def desc(pkg, s, bias=True, relu=False, N=None):
    return pkg.ConvDesc.deconvolution(s.N if N is None else N, s.C, s.H, s.W, s.M, (s.KH, s.KW), (s.stride_h, s.stride_w),
                                      (s.pad_h, s.pad_w), s.group, bias, relu)


def weights(s, seed=5, density=0.4):
    """blobs_[0], C x Mg x KH x KW float32, about `density` nonzero; bottom channel 0 has an empty row and the last channel
    a full one (layers of one channel per group keep their random row)."""
    rs = np.random.RandomState(seed)
    mg = s.M // s.group
    w = rs.uniform(-1, 1, (s.C, mg, s.KH, s.KW)).astype(np.float32)
    w[w == 0] = 0.5
    keep = rs.uniform(0, 1, w.shape) < density
    if s.C > 1:
        keep[0] = False
        keep[-1] = True
    return w * keep


def inputs(s, seed=7):
    rs = np.random.RandomState(seed)
    x = rs.uniform(-1, 1, (s.N, s.C, s.H, s.W)).astype(np.float32)
    b = rs.uniform(-0.5, 0.5, s.M).astype(np.float32)
    td = rs.uniform(-1, 1, (s.N, s.M) + out_hw(s)).astype(np.float32)
    return x, b, td


# ---- the decomposition, from the contract's formulas -------------------------------------------------------------------
def inner_dims(s):
    """(P, KH', KW', H', W')"""
    kh, kw = -(-s.KH // s.stride_h), -(-s.KW // s.stride_w)
    return s.stride_h * s.stride_w, kh, kw, s.H + kh - 1, s.W + kw - 1


def inner_shape(synth, s, N=None):
    """The inner stride-1 layer as a synth shape (what errbound.py and torch's conv2d take)."""
    P, kh, kw, _, _ = inner_dims(s)
    return synth.shape(s.name + "_inner", s.N if N is None else N, s.C, s.H, s.W, s.M * P, kh, KW=kw, pad=kh - 1, pad_w=kw - 1, group=s.group)


def inner_position(s, c, ml, kr, kc):
    """(row m', group-local column) of entry (c, ml, kr, kc): m' = (m * sh + kr % sh) * sw + kc % sw with m = g * Mg + ml,
    column cl * KH' * KW' + (KH' - 1 - kr / sh) * KW' + (KW' - 1 - kc / sw)."""
    _, kh, kw, _, _ = inner_dims(s)
    cg, mg = s.C // s.group, s.M // s.group
    g, cl = c // cg, c % cg
    m = g * mg + ml
    return ((m * s.stride_h + kr % s.stride_h) * s.stride_w + kc % s.stride_w,
            cl * kh * kw + (kh - 1 - kr // s.stride_h) * kw + (kw - 1 - kc // s.stride_w))


def inner_weights(s, w):
    """(W', at): the inner dense blobs_[0], M * P x Cg x KH' x KW', and for every element of w its flat position in W'."""
    P, kh, kw, _, _ = inner_dims(s)
    cg = s.C // s.group
    wi = np.zeros((s.M * P, cg * kh * kw), w.dtype)
    at = np.zeros(w.shape, np.int64)
    for c, ml, kr, kc in np.ndindex(*w.shape):
        r, col = inner_position(s, c, ml, kr, kc)
        at[c, ml, kr, kc] = r * cg * kh * kw + col
        wi[r, col] = w[c, ml, kr, kc]
    assert len(np.unique(at)) == at.size, "the entry map is not injective"
    return wi.reshape(s.M * P, cg, kh, kw), at


def unpack(s, t, bias=None, relu=False):
    """top[n][m][oh][ow] = T'[n][m'(m, hp % sh, wp % sw)][hp / sh][wp / sw] + bias[m], then v > 0 ? v : 0."""
    P, _, _, hi, wi = inner_dims(s)
    oh, ow = out_hw(s)
    n = t.shape[0]
    t6 = t.reshape(n, s.M, s.stride_h, s.stride_w, hi, wi)
    hp, wp = np.arange(oh) + s.pad_h, np.arange(ow) + s.pad_w
    top = t6[:, :, (hp % s.stride_h)[:, None], (wp % s.stride_w)[None, :], (hp // s.stride_h)[:, None], (wp // s.stride_w)[None, :]]
    if bias is not None:
        top = top + np.asarray(bias, top.dtype)[None, :, None, None]
    if relu:
        top = np.where(top > 0, top, 0).astype(top.dtype)
    return top


def pack(s, top_diff, top=None):
    """G'[n][m'][i][j] = top_diff[n][m][i * sh + ph - pad_h][j * sw + pw - pad_w] inside OH x OW (top > 0 ? that : 0 where top
    is given), +0 outside."""
    P, _, _, hi, wi = inner_dims(s)
    oh, ow = out_hw(s)
    n = top_diff.shape[0]
    g = top_diff if top is None else np.where(np.asarray(top) > 0, top_diff, 0).astype(top_diff.dtype)
    out = np.zeros((n, s.M, s.stride_h, s.stride_w, hi, wi), top_diff.dtype)
    for ph in range(s.stride_h):
        for pw in range(s.stride_w):
            r = np.arange(hi) * s.stride_h + ph - s.pad_h
            c = np.arange(wi) * s.stride_w + pw - s.pad_w
            ri, ci = np.nonzero((r >= 0) & (r < oh))[0], np.nonzero((c >= 0) & (c < ow))[0]
            if len(ri) and len(ci):
                out[:, :, ph, pw, ri[:, None], ci[None, :]] = g[:, :, r[ri][:, None], c[ci][None, :]]
    return out.reshape(n, s.M * P, hi, wi)


# ---- the float64 reference ------------------------------------------------------------------------------------------------
def ref_forward(s, w, x, b=None, relu=False):
    import torch
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float64))  # noqa: E731
    y = torch.nn.functional.conv_transpose2d(t(x), t(w), t(b), stride=(s.stride_h, s.stride_w), padding=(s.pad_h, s.pad_w),
                                             groups=s.group).numpy()
    return np.maximum(y, 0.0) if relu else y


def ref_backward(s, w, x, b, top_diff, top=None):
    """torch float64 autograd of conv_transpose2d: (bottom_diff, weight_diff masked by the pattern, bias_diff); with `top` the
    gradient is top_diff x [top > 0]."""
    import torch
    X = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    Wt = torch.tensor(np.asarray(w, np.float64), requires_grad=True)
    B = torch.tensor(np.asarray(b, np.float64), requires_grad=True)
    y = torch.nn.functional.conv_transpose2d(X, Wt, B, stride=(s.stride_h, s.stride_w), padding=(s.pad_h, s.pad_w), groups=s.group)
    g = torch.tensor(np.asarray(top_diff, np.float64))
    if top is not None:
        g = g * torch.tensor((np.asarray(top) > 0).astype(np.float64))
    y.backward(g)
    return X.grad.numpy(), Wt.grad.numpy() * (np.asarray(w) != 0), B.grad.numpy()


# ---- the bound: errbound.py on the inner layer, carried through the pack / unpack rules ---------------------------------
def forward_bound(eb, synth, s, w, x, b=None, relu=False):
    """(want, B) per top element: errbound.forward_bound of the inner stride-1 layer -- with bias[m] as the bias of m's P inner
    channels, so that the bias add is the one rounding the bound's "+ 4" already counts -- read through the unpack rule."""
    P = inner_dims(s)[0]
    wi, _ = inner_weights(s, w)
    bi = None if b is None else np.repeat(np.asarray(b), P)
    want, B = eb.forward_bound(inner_shape(synth, s, x.shape[0]), wi, x, bi)
    want, B = unpack(s, want), unpack(s, B)
    return (np.maximum(want, 0.0) if relu else want), B


def backward_bound(eb, synth, s, w, x, top_diff, top=None, mask=None):
    """((bottom_diff, weight_diff, bias_diff), (B_bottom, B_weight, B_bias)): errbound.backward_bound of the inner layer on
    G' = pack(top_diff, top), the weight gradient read back through the entry map into C x Mg x KH x KW, the bias gradient
    summed over a channel's P phases.  That sum is P more additions on top of the inner sum's k = N * H' * W' + 4 roundings,
    so its bound is the inner bounds' sum scaled by gamma(k + P) / gamma(k).  `mask`: the plan's pattern in w's shape where
    it holds explicit zeros (default: w != 0)."""
    P = inner_dims(s)[0]
    wi, at = inner_weights(s, w)
    own = (np.asarray(w) != 0) if mask is None else np.asarray(mask, bool)
    pattern = np.zeros(wi.size, bool)
    pattern[at[own]] = True
    g = pack(s, np.asarray(top_diff, np.float64), top)
    bi = np.zeros(s.M * P, np.float32)
    want, Bs = eb.backward_bound(inner_shape(synth, s, x.shape[0]), wi, x, bi, g, mask=pattern.reshape(wi.shape))
    k = float(g.shape[0] * g.shape[2] * g.shape[3] + 4)
    scale = float(eb.gamma(k + P) / eb.gamma(k))
    wd, Bw = want[1].reshape(-1)[at] * own, Bs[1].reshape(-1)[at]
    bd, Bb = want[2].reshape(s.M, P).sum(axis=1), Bs[2].reshape(s.M, P).sum(axis=1) * scale
    return (want[0], wd, bd), (Bs[0], Bw, Bb)


def csr_of(s, w):
    """The layer's CSR as escoin_plan_get_csr gives it: per conv group, rows = the group's bottom channels, column =
    ml * KH * KW + kr * KW + kc ascending.  (rowptr, colidx, values, nnz_per_group), rowptr group-relative."""
    cg = s.C // s.group
    rp, ci, va, ng = [], [], [], []
    for g in range(s.group):
        rows = np.asarray(w[g * cg:(g + 1) * cg]).reshape(cg, -1)
        rp.append(0)
        n = 0
        for r in rows:
            nz = np.nonzero(r)[0]
            ci.extend(nz.tolist())
            va.extend(r[nz].tolist())
            n += len(nz)
            rp.append(n)
        ng.append(n)
    return np.array(rp, np.int32), np.array(ci, np.int32), np.array(va, np.float32), np.array(ng, np.int32)
