"""Shared by test_s2d_host.py and test_s2d_gpu.py: the shapes plan option "s2d" is tested on -- the smallest at which each
piece (the pack / unpack kernels' phase arithmetic, the inner CSR, the inner kernels) can still go wrong -- a seeded slice
of random geometries, and the space-to-depth identity of include/escoin.h restated in numpy."""
import numpy as np

# name: (N, C, H, W, M, K, kwargs of synth.shape)
SHAPES = {
    "3x3_s2": (2, 5, 8, 7, 6, 3, dict(pad=1, stride=2)),           # four phases, odd width, 2x2 inner kernel with positions without a preimage
    "3x3_s2x3_g2": (2, 10, 9, 11, 14, 3, dict(pad=1, pad_w=0, stride=2, stride_w=3, group=2)),   # PW = 3, KW' = 1, channel order within groups
    "2x2_s3": (2, 3, 10, 10, 4, 2, dict(stride=3)),                # stride > kernel: PH < stride; bottom rows and columns no window reads
    "7x7_s2": (1, 3, 19, 19, 8, 7, dict(pad=3, stride=2, sparsity=0.5)),     # 4x4 inner kernel
    "5x5_s4": (1, 4, 17, 17, 5, 5, dict(stride=4)),                # PH = 4, 2x2 inner kernel
    "pw_s2_odd": (3, 6, 9, 9, 8, 1, dict(stride=2)),               # odd width: not the strided-pointwise special case
    "res_like": (2, 64, 28, 28, 64, 3, dict(pad=1, stride=2, sparsity=0.9)),  # the inner generated-code kernel with a real tiling
}
# where the option must change nothing: stride 1, and a dilation
UNSERVED = {
    "3x3_s1": (2, 5, 8, 7, 6, 3, dict(pad=1)),
    "3x3_s2_dil2": (1, 4, 9, 9, 4, 3, dict(pad=2, stride=2, dil=2, sparsity=0.0)),
}


def make(synth, name):
    N, C, H, W, M, K, kw = (SHAPES.get(name) or UNSERVED[name])
    return synth.shape(name, N, C, H, W, M, K, **kw)


def random_shapes(synth, count=24, seed=20261):
    """`count` seeded geometries: stride 1-3 per axis (not both 1), kernel 1-5 per axis, pad 0-3, groups 1-2, dilation 1;
    those without an output pixel are drawn again."""
    rs = np.random.RandomState(seed)
    out = []
    while len(out) < count:
        group = int(rs.randint(1, 3))
        cg, mg = int(rs.randint(1, 6)), int(rs.randint(1, 9))
        kh, kw = int(rs.randint(1, 6)), int(rs.randint(1, 6))
        H, W = int(rs.randint(3, 14)), int(rs.randint(3, 14))
        sh, sw = int(rs.randint(1, 4)), int(rs.randint(1, 4))
        kwargs = dict(KW=kw, pad=int(rs.randint(0, 4)), pad_w=int(rs.randint(0, 4)), stride=sh, stride_w=sw, group=group,
                      sparsity=round(float(rs.uniform(0.0, 0.9)), 2))
        s = synth.shape("s2d_rand%02d" % len(out), int(rs.randint(1, 4)), group * cg, H, W, group * mg, kh, **kwargs)
        if (sh, sw) != (1, 1) and min(synth.out_hw(s)) >= 1:
            out.append(s)
    return out


def inner_dims(s, synth):
    """(PH, PW, C', H', W', KH', KW') of the inner stride-1 layer."""
    oh, ow = synth.out_hw(s)
    ph, pw = min(s.stride_h, s.KH), min(s.stride_w, s.KW)
    kh, kw = -(-s.KH // s.stride_h), -(-s.KW // s.stride_w)
    return ph, pw, s.C * ph * pw, oh + kh - 1, ow + kw - 1, kh, kw


def pack(s, synth, x):
    """X' of the identity: X'[n][(c * PH + ph) * PW + pw][i][j] = x[n][c][i * s_h + ph - pad_h][j * s_w + pw - pad_w], 0 outside."""
    ph_n, pw_n, ci, hi, wi, _, _ = inner_dims(s, synth)
    n = x.shape[0]
    xp = np.zeros((n, s.C, max(hi * s.stride_h, s.H + s.pad_h), max(wi * s.stride_w, s.W + s.pad_w)), x.dtype)
    xp[:, :, s.pad_h:s.pad_h + s.H, s.pad_w:s.pad_w + s.W] = x
    out = np.zeros((n, s.C, ph_n, pw_n, hi, wi), x.dtype)
    for ph in range(ph_n):
        for pw in range(pw_n):
            out[:, :, ph, pw] = xp[:, :, ph:ph + hi * s.stride_h:s.stride_h, pw:pw + wi * s.stride_w:s.stride_w][:, :, :hi, :wi]
    return out.reshape(n, ci, hi, wi)


def unpack(s, synth, dxi):
    """bottom_diff of the identity from dX' (NaN where the rule would write nothing: there is no such element)."""
    ph_n, pw_n, ci, hi, wi, _, _ = inner_dims(s, synth)
    n = dxi.shape[0]
    d6 = dxi.reshape(n, s.C, ph_n, pw_n, hi, wi)
    out = np.full((n, s.C, s.H, s.W), np.nan, dxi.dtype)
    for h in range(s.H):
        hp = h + s.pad_h
        for w in range(s.W):
            wp = w + s.pad_w
            ph, i, pw, j = hp % s.stride_h, hp // s.stride_h, wp % s.stride_w, wp // s.stride_w
            out[:, :, h, w] = d6[:, :, ph, pw, i, j] if ph < ph_n and pw < pw_n and i < hi and j < wi else 0.0
    return out
