"""Shared by test_dgrad_mfma_host.py and test_dgrad_mfma_gpu.py: the shapes the MFMA data-gradient kernel is tested on -- the
smallest at which it can still go wrong (tiles of 64 input channels x 64 phase pixels, steps of 32 columns, two columns per
matrix instruction, one stride-1 gather-GEMM per stride phase) -- and a seeded slice of random geometries."""
import numpy as np

# name: (N, C, H, W, M, KH, kwargs of synth.shape)
SHAPES = {
    # C one above 64: two channel tiles, the second with 6 of its 64 rows; three empty phases; Kp = 40: two K-steps; 75
    # phase pixels: two pixel tiles, the first crossing two image boundaries
    "pw_s2": (3, 70, 9, 9, 40, 1, dict(stride=2, sparsity=0.3)),
    "3x3_s2": (2, 5, 8, 7, 6, 3, dict(pad=1, stride=2, sparsity=0.0)),              # phases of 1 / 2 / 2 / 4 taps, odd width
    # six phases; Cg = 5, Mg = 7 and Kp = 7 .. 14 are no multiples of the tiles
    "3x3_s2x3_g2": (2, 10, 9, 11, 14, 3, dict(pad=1, pad_w=0, stride=2, stride_w=3, group=2, sparsity=0.4)),
    "3x3_s2_dil2": (1, 4, 9, 9, 4, 3, dict(pad=2, stride=2, dil=2, sparsity=0.0)),  # only one phase has taps
    "2x2_s3": (2, 3, 10, 10, 4, 2, dict(stride=3, sparsity=0.25)),                  # stride > kernel; the bottom's last row and column are read by no window
    "3x3_pad3": (2, 4, 6, 6, 5, 3, dict(pad=3, sparsity=0.5)),                      # stride 1, no transposed plan: a single phase
    "emptyblock": (1, 64, 8, 8, 70, 1, dict(stride=2, sparsity=0.0)),               # rows 32..63 of the weights zeroed: K-step 1 of 3 is not live
    "res3a_branch2a": (2, 256, 56, 56, 128, 1, dict(stride=2, bias=False, sparsity=0.0)),   # a real chain layer at small batch
}


def make(synth, name):
    N, C, H, W, M, K, kw = SHAPES[name]
    return synth.shape(name, N, C, H, W, M, K, **kw)


def weights(synth, s, seed=11):
    w = synth.pruned_weights(s, seed)
    if s.name == "emptyblock":
        w[32:64] = 0
    return w


def random_shapes(synth, count=24, seed=20260):
    """`count` seeded geometries: stride 1-3 per axis, dilation 1-2, pad 0-3, groups 1-2, kernel 1-3 per axis, density
    0.1-1.0; those without an output pixel are drawn again."""
    rs = np.random.RandomState(seed)
    out = []
    while len(out) < count:
        group = int(rs.randint(1, 3))
        cg, mg = int(rs.randint(1, 8)), int(rs.randint(1, 14))
        kh, kw = int(rs.randint(1, 4)), int(rs.randint(1, 4))
        H, W = int(rs.randint(3, 13)), int(rs.randint(3, 13))
        kwargs = dict(KW=kw, pad=int(rs.randint(0, 4)), pad_w=int(rs.randint(0, 4)), stride=int(rs.randint(1, 4)),
                      stride_w=int(rs.randint(1, 4)), dil=int(rs.randint(1, 3)), dil_w=int(rs.randint(1, 3)), group=group,
                      sparsity=round(float(rs.uniform(0.0, 0.9)), 2))
        s = synth.shape("rand%02d" % len(out), int(rs.randint(1, 4)), group * cg, H, W, group * mg, kh, **kwargs)
        if min(synth.out_hw(s)) >= 1:
            out.append(s)
    return out


def phases(s):
    """The stride phases restated: per phase (row residue major) a dict of h0, w0, rows, cols and its taps [(kr, kc, dh,
    dw)], ascending: tap (kr, kc) of phase pixel (hh, ww) reads top pixel (hh + dh, ww + dw)."""
    def axis(r, size, pad, stride, dil, K):
        first = (r - pad) % stride
        count = len(range(first, size, stride))
        taps = [(k, (first + pad - k * dil) // stride) for k in range(K) if (k * dil) % stride == r]
        assert all((first + pad - k * dil) % stride == 0 for k, _ in taps)
        return first, count, taps
    out = []
    for rh in range(s.stride_h):
        for rw in range(s.stride_w):
            h0, rows, th = axis(rh, s.H, s.pad_h, s.stride_h, s.dil_h, s.KH)
            w0, cols, tw = axis(rw, s.W, s.pad_w, s.stride_w, s.dil_w, s.KW)
            out.append(dict(h0=h0, w0=w0, rows=rows, cols=cols, taps=[(kr, kc, dh, dw) for kr, dh in th for kc, dw in tw]))
    return out
