"""The layers of test_errbound_layouts_cpu.py and test_errbound_layouts_gpu.py: every layout class of the tiled kernels
(BODY: test_body_variant_gpu.CASES, imported) and every instantiation and store path of the dense MFMA kernel (DENSE),
each with a bias, on inputs skewed by errbound.skew with seeds derived from the row's name.

The CPU module checks the table itself -- the checker sees three corruptions on every row, the host rules give every BODY
row the tiling it names, dense_variant() gives every DENSE row the variant it names -- so the table cannot rot without
a GPU noticing; the GPU module runs the kernels on it."""
from collections import namedtuple

import errbound as eb
from test_body_variant_gpu import CASES as _BODY_CASES

N_CU = 256              # the device the tilings and the stream-K variants below are named for (MI355X)
TILING_BATCH = 256      # every BODY row is tiled as for a batch of 256 and run on its few images

BodyRow = namedtuple("BodyRow", "name dims kw expect variant options")
DenseRow = namedtuple("DenseRow", "name dims kw expect_variant reaches")

# (N, C, H, W, M, K, pad, sparsity), what the tiling must say, the body variant, further plan options
BODY = [BodyRow(name, d[:6], dict(pad=d[6], sparsity=d[7]), expect, variant, options)
        for name, d, expect, variant, options in _BODY_CASES]


def _dense(name, N, C, H, W, M, K, variant, reaches, pad=0, group=1):
    return DenseRow(name, (N, C, H, W, M, K), dict(pad=pad, group=group, sparsity=0.0), variant, reaches)


# stat "dense_variant" = WROWS + 4 * BMODE + 8 * vec_out + 16 * STREAMK (include/escoin.h), on N_CU compute units
DENSE = [
    _dense("dn_g128v", 3, 8, 10, 10, 72, 3, 10, "WROWS 2 gathered, 16-byte stores (100 pixels), one channel tile of 72 of 128 rows, "
           "pixel tiles 128 + 128 + 44, K = 72 (tail of 8)", pad=1),
    _dense("dn_g128s", 3, 8, 9, 11, 130, 3, 2, "scalar stores (99 pixels), a second channel tile of 2 rows", pad=1),
    _dense("dn_pw64", 5, 40, 6, 6, 33, 1, 13, "pointwise 16-byte operand, K = 40 (rows past K staged as zeros), ragged pixel tile 128 + 52"),
    _dense("dn_pw128", 5, 40, 6, 6, 150, 1, 14, "the same on WROWS 2, a second channel tile of 22 rows"),
    _dense("dn_pwodd", 5, 40, 5, 5, 33, 1, 1, "1x1 with H * W % 4 = 1: the gather path, scalar stores"),
    _dense("dn_pwg", 4, 40, 6, 6, 48, 1, 13, "cg addressing of the pointwise operand and of the 16-byte stores, Cg = 20 < one k-step", group=2),
    _dense("sk_pw64", 160, 1024, 8, 8, 48, 1, 29, "stream-K on WROWS 1, BMODE 1, 16-byte stores: 80 tiles x 32 k-steps over 512 runs of 5"),
    _dense("sk_pw128", 64, 1024, 8, 8, 512, 1, 30, "stream-K on WROWS 2, BMODE 1: 128 tiles, runs of 8 steps"),
]
GK_VARIANT = 18         # test_errbound_gpu.GK: stream-K on WROWS 2, gathered operand, scalar stores (49 pixels)

# dn_pw64 with the bottom, then the top, 4 bytes off a 16-byte boundary: (run, bottom off, top off, dense_variant)
OFF_BOUNDARY = [("bottom_off", True, False, 9), ("top_off", False, True, 5)]

# The data gradient of a BODY row runs a transposed plan (C' = M, M' = C = 8 .. 64, pad' = K - 1 - pad) on the same
# images.  Where the rules refuse backward_kernel = JIT on that geometry the first backward fails: row name -> the text.
BWD_JIT_REFUSALS = {}

_LAYERS = {}


def spec(row):
    """(name, (N, C, H, W, M, K), kwargs of synth.shape) of a row: what test_errbound_gpu._layer takes."""
    return (row.name, row.dims, row.kw)


def layer(synth, row):
    """(shape, skewed inputs, unskewed (w, x, b)) of a row, made once; test_errbound_gpu._layer's seeds."""
    if row.name not in _LAYERS:
        s = synth.shape(row.name, *row.dims, **row.kw)
        k = sum(map(ord, row.name))
        w, x, b = synth.pruned_weights(s, k), synth.activations(s, k + 1), synth.bias_vector(s, k + 2)
        _LAYERS[row.name] = (s, eb.skew(s, w, x, b, k + 3), (w, x, b))
    return _LAYERS[row.name]


def dense_variant(s, n_images, n_cu=N_CU, bottom_aligned=True, top_aligned=True):
    """What launch_dense (csrc/dense_mfma.hip) launches for n_images of shape s on n_cu compute units, as stat
    "dense_variant" reports it: the rule's inputs as that function states them, for a plan that runs the whole layer on
    the dense kernel."""
    oh = (s.H + 2 * s.pad_h - (s.dil_h * (s.KH - 1) + 1)) // s.stride_h + 1
    ow = (s.W + 2 * s.pad_w - (s.dil_w * (s.KW - 1) + 1)) // s.stride_w + 1
    P = n_images * oh * ow
    mg, kdim = s.M // s.group, (s.C // s.group) * s.KH * s.KW
    unit_1x1 = s.KH == 1 and s.KW == 1 and s.stride_h == 1 and s.stride_w == 1
    pointwise = unit_1x1 and s.pad_h == 0 and s.pad_w == 0
    vec_b = pointwise and (s.H * s.W) % 4 == 0 and bottom_aligned and P >= 4
    vec_out = (oh * ow) % 4 == 0 and top_aligned
    bm = 64 if mg <= 64 else 128
    tiles = -(-P // 128) * -(-mg // bm) * s.group
    slots = 2 * n_cu
    nk = -(-kdim // 32)
    rounds = -(-tiles // slots)
    streamk = unit_1x1 and tiles / float(rounds * slots) < 0.85 and nk >= 8 and tiles * nk >= 4 * slots
    return (1 if bm == 64 else 2) + 4 * vec_b + 8 * vec_out + 16 * streamk
