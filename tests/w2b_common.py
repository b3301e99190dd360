"""Plan option "w2b" (include/escoin.h "Width-to-batch"), for test_w2b_host.py and test_w2b_gpu.py: the shapes, the strip rule
and the three rearrangements restated in numpy from the header alone."""
import numpy as np

# name -> (N, C, M, H, W, KH, KW, pad_h, pad_w, group, forced strip): the smallest at which each index rule can go wrong
SHAPES = {
    "k3p1": (3, 4, 6, 5, 19, 3, 3, 1, 1, 1, 8),        # halo on both sides, a short last strip (8, 8, 3)
    "k5p2_g2": (3, 4, 6, 6, 21, 5, 5, 2, 2, 2, 4),     # SW == KW - 1: every interior column in two strips
    "k3p0": (3, 5, 4, 4, 18, 3, 3, 0, 0, 1, 8),        # OW = W - 2, the last strip exactly full
    "k3p3": (3, 3, 5, 4, 13, 3, 3, 3, 3, 1, 8),        # OW > W: strips lying wholly in the padding
    "k1x3": (3, 8, 3, 3, 17, 1, 3, 0, 1, 1, 12),       # one kernel row
    "k3x1": (3, 4, 8, 7, 17, 3, 1, 1, 0, 1, 8),        # KW = 1: no halo, unpack_sum always has one term
    "real": (2, 2, 4, 3, 300, 3, 3, 1, 1, 1, 0),       # the shipped rule: S = 2, SW = 152, Wi = 154
}


def make(synth, name, bias=True, **over):
    N, C, M, H, W, KH, KW, ph, pw, group, _ = SHAPES[name]
    return synth.shape(name, N, C, H, W, M, KH, **dict(dict(KW=KW, pad=ph, pad_w=pw, group=group, bias=bias, sparsity=0.85), **over))


def plan_row(synth, s, strip=0, f64=False):
    """w2b_plan's answer (tests/cpp/w2b_plan_check.cpp): [0] where the option does not serve the layer, else [1, S, SW, Wi,
    x_floats, t_floats, the inner descriptor]."""
    (oh, ow), halo = synth.out_hw(s), s.KW - 1
    if f64 or (s.stride_h, s.stride_w, s.dil_h, s.dil_w) != (1, 1, 1, 1) or (not strip and max(s.W, ow) <= 256):
        return [0]
    cap = (256 - halo) // 4 * 4                        # the widest strip: a multiple of 4 with SW + KW - 1 <= 256
    S = -(-ow // (strip or max(cap, 1)))               # the fewest strips
    SW = strip or -(-(-(-ow // S)) // 4) * 4
    Wi = SW + halo
    x, t = s.N * S * s.C * s.H * Wi, s.N * S * s.M * oh * SW
    if SW % 4 or SW < max(halo, 4) or Wi > 256 or s.N * S > 65535 or max(x, t, s.N * s.C * s.H * s.W, s.N * s.M * oh * ow) >= 2 ** 31:
        return [0]
    return [1, S, SW, Wi, x, t, s.N * S, s.C, s.H, Wi, s.M, s.KH, s.KW, s.pad_h, 0, 1, 1, 1, 1, s.group, int(bool(s.bias)), 0]


def pack(a, S, SW, Wd, off, mask=None):
    """strip[n * S + s][ch][h][x] = a[n][ch][h][s * SW - off + x] inside the row (mask > 0 ? that : 0), +0 outside."""
    n, ch, hr, ws = a.shape
    frame = np.zeros((n, ch, hr, off + max(ws, S * SW) + Wd), a.dtype)
    frame[..., off:off + ws] = a if mask is None else np.where(mask > 0, a, np.float32(0))
    return np.stack([frame[..., s * SW:s * SW + Wd] for s in range(S)], axis=1).reshape(n * S, ch, hr, Wd)


def unpack(t, S, SW, ow, relu=False):
    """top[n][m][oh][w] = t[n * S + w / SW][m][oh][w % SW], through v > 0 ? v : 0 with relu."""
    ns, ch, hr, _ = t.shape
    top = t.reshape(ns // S, S, ch, hr, SW).transpose(0, 2, 3, 1, 4).reshape(ns // S, ch, hr, S * SW)[..., :ow]
    return np.where(top > 0, top, np.float32(0)) if relu else np.ascontiguousarray(top)


def unpack_sum(dx, S, SW, W, off):
    """bottom_diff[n][c][h][w] = the sum over s, ascending, of dx[n * S + s][c][h][w + off - s * SW] where that index is in [0, Wi)."""
    ns, ch, hr, wi = dx.shape
    frame = np.zeros((ns // S, ch, hr, S * SW + wi), dx.dtype)
    for s in range(S):
        frame[..., s * SW:s * SW + wi] += dx.reshape(ns // S, S, ch, hr, wi)[:, s]
    return np.ascontiguousarray(frame[..., off:off + W])
