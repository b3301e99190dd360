"""Shared by test_s2b_host.py and test_s2b_gpu.py: the shapes plan option "s2b" is tested on -- the smallest at which each
piece (the pack / unpack kernels' residue arithmetic, short residue classes, the inner kernels) can still go wrong -- a
seeded slice of random geometries, and the space-to-batch identity of include/escoin.h restated in numpy."""
import numpy as np

# name: (N, C, H, W, M, K, kwargs of synth.shape)
SHAPES = {
    "3x3_d2": (3, 8, 9, 9, 8, 3, dict(pad=2, dil=2, sparsity=0.5)),                   # the plain case
    "3x3_d2x3_g2": (2, 8, 11, 10, 12, 3, dict(pad=2, pad_w=1, dil=2, dil_w=3, group=2, sparsity=0.5)),  # uneven residue classes, Hp = 15
    "d_gt_out": (2, 4, 7, 8, 4, 3, dict(dil=3, dil_w=2, sparsity=0.5)),               # OH = 1 < eh: classes without a top pixel
    "one_tap_axis": (2, 4, 6, 9, 6, 1, dict(KW=3, pad=0, pad_w=2, dil=2, sparsity=0.5)),   # eh = 1
    "pad_gt_span": (2, 4, 6, 6, 4, 2, dict(pad=3, dil=2, sparsity=0.5)),              # pad > dil * (K - 1): the outer plan has no transposed plan
    "5x5_d2": (2, 6, 13, 13, 6, 5, dict(pad=4, dil=2, sparsity=0.7)),                 # the 5x5 kernel
    "res_like": (4, 64, 14, 14, 64, 3, dict(pad=2, dil=2, sparsity=0.9)),             # the only shape JIT / TILED are forced on
    "d12_small": (1, 8, 13, 13, 8, 3, dict(pad=12, dil=12, sparsity=0.5)),            # 144 inner images of 4x4
}
# where the option must change nothing: dilation 1, a 1x1 kernel with a dilation, a stride with a dilation
# (a double plan and the two lowered modes are cases of the tests themselves: they are no geometries)
UNSERVED = {
    "3x3_d1": (2, 5, 8, 7, 6, 3, dict(pad=1, sparsity=0.5)),
    "1x1_d2": (2, 6, 9, 9, 8, 1, dict(dil=2, sparsity=0.5)),
    "3x3_s2_d2": (1, 4, 9, 9, 4, 3, dict(pad=2, stride=2, dil=2, sparsity=0.0)),
}


def make(synth, name):
    N, C, H, W, M, K, kw = (SHAPES.get(name) or UNSERVED[name])
    return synth.shape(name, N, C, H, W, M, K, **kw)


def random_shapes(synth, count=24, seed=20262):
    """`count` seeded geometries the option serves: stride 1, dilation 1-4 per axis, kernel 1-4 per axis, pad 0-4, groups
    1-2; those without an output pixel or with P == 1 are drawn again."""
    rs = np.random.RandomState(seed)
    out = []
    while len(out) < count:
        group = int(rs.randint(1, 3))
        cg, mg = int(rs.randint(1, 5)), int(rs.randint(1, 7))
        kh, kw = int(rs.randint(1, 5)), int(rs.randint(1, 5))
        H, W = int(rs.randint(3, 15)), int(rs.randint(3, 15))
        dh, dw = int(rs.randint(1, 5)), int(rs.randint(1, 5))
        kwargs = dict(KW=kw, pad=int(rs.randint(0, 5)), pad_w=int(rs.randint(0, 5)), dil=dh, dil_w=dw, group=group,
                      sparsity=round(float(rs.uniform(0.0, 0.8)), 2))
        s = synth.shape("s2b_rand%03d" % len(out), int(rs.randint(1, 4)), group * cg, H, W, group * mg, kh, **kwargs)
        if min(synth.out_hw(s)) >= 1 and inner_dims(s, synth)[2] > 1:
            out.append(s)
    return out


def inner_dims(s, synth):
    """(eh, ew, P, H', W', OH', OW') of the inner undilated layer."""
    oh, ow = synth.out_hw(s)
    eh, ew = (s.dil_h if s.KH > 1 else 1), (s.dil_w if s.KW > 1 else 1)
    hi, wi = -(-(s.H + 2 * s.pad_h) // eh), -(-(s.W + 2 * s.pad_w) // ew)
    assert (hi - s.KH + 1, wi - s.KW + 1) == (-(-oh // eh), -(-ow // ew))
    return eh, ew, eh * ew, hi, wi, hi - s.KH + 1, wi - s.KW + 1


def pack(a, eh, ew, off_h, off_w, hd, wd):
    """Residue-class images of `a` (n, ch, Hs, Ws) at offset (off_h, off_w) in the padded frame:
    out[(n * eh + qh) * ew + qw][ch][i][j] = a[n][ch][i * eh + qh - off_h][j * ew + qw - off_w], 0 outside."""
    n, ch, hs, ws = a.shape
    frame = np.zeros((n, ch, max(hd * eh, hs + off_h), max(wd * ew, ws + off_w)), a.dtype)
    frame[:, :, off_h:off_h + hs, off_w:off_w + ws] = a
    assert hd * eh >= hs + off_h and wd * ew >= ws + off_w
    out = np.zeros((n, eh, ew, ch, hd, wd), a.dtype)
    for qh in range(eh):
        for qw in range(ew):
            out[:, qh, qw] = frame[:, :, qh:qh + hd * eh:eh, qw:qw + wd * ew:ew]
    return out.reshape(n * eh * ew, ch, hd, wd)


def unpack(b, eh, ew, off_h, off_w, hs, ws):
    """The inverse on the image: out[n][ch][h][w] = b[n'(n, hp % eh, wp % ew)][ch][hp / eh][wp / ew], (hp, wp) = (h + off_h, w + off_w)."""
    np_, ch, hd, wd = b.shape
    n = np_ // (eh * ew)
    b6 = b.reshape(n, eh, ew, ch, hd, wd)
    out = np.full((n, ch, hs, ws), np.nan, b.dtype)
    for h in range(hs):
        hp = h + off_h
        for w in range(ws):
            wp = w + off_w
            out[:, :, h, w] = b6[:, hp % eh, wp % ew, :, hp // eh, wp // ew]
    return out
