"""Shared by test_dense_bf16_host.py and test_dense_bf16_gpu.py (plan option "dense_math" = bf16): the round-to-nearest-even
of float32 to bfloat16 in numpy, and the cases -- the non-stream-K rows of layout_cases.DENSE plus three of this module's."""
from collections import namedtuple

import numpy as np

import layout_cases as lc


def bf16_rne(a):
    """float32 -> the nearest bfloat16 (ties to even), returned as float32: add 0x7FFF plus the lsb that survives, keep the
    top 16 bits.  A value past bf16's largest finite one carries into the exponent: infinity.  (NaNs are not handled.)"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


# name, (N, C, H, W, M, K), kwargs of synth.shape, images per call, the fp32 kernel's dense_variant, what the case reaches
Case = namedtuple("Case", "name dims kw n_images variant reaches")
CASES = [Case(r.name, r.dims, r.kw, r.dims[0], r.expect_variant, r.reaches) for r in lc.DENSE if not r.name.startswith("sk_")] + [
    Case("b16_s2", (3, 8, 31, 31, 8, 3), dict(pad=1, stride=2, sparsity=0.6), 3, 9, "stride 2, pad 1, 3x3: the gather's window origins"),
    Case("b16_dil", (2, 24, 13, 16, 20, 3), dict(pad=2, dil=2, sparsity=0.0), 2, 9,
         "dilation 2: K = 216, a last k-step whose upper half lies past the decode table's end"),
    Case("b16_part", (3, 8, 9, 11, 130, 3), dict(pad=1, sparsity=0.0), 2, 2, "dn_g128s's geometry, two of three images"),
]
IDS = [c.name for c in CASES]
# K per conv group, the kernel's k-steps of 64 and (bm, pixel tiles, channel tiles, tiles) of a whole batch: align_rules.h db16_plan
PLANS = {"dn_g128v": (72, 2, 128, 3, 1, 3), "dn_g128s": (72, 2, 128, 3, 2, 6), "dn_pw64": (40, 1, 64, 2, 1, 2),
         "dn_pw128": (40, 1, 128, 2, 2, 4), "dn_pwodd": (40, 1, 64, 1, 1, 1), "dn_pwg": (20, 1, 64, 2, 1, 4),
         "b16_s2": (72, 2, 64, 6, 1, 6), "b16_dil": (216, 4, 64, 4, 1, 4), "b16_part": (72, 2, 128, 2, 2, 4)}
_LAYERS = {}


def layer(synth, eb, c):
    """(shape, skewed inputs, the skewed weights and activations rounded to bf16) of a case, made once."""
    if c.name not in _LAYERS:
        s = synth.shape(c.name, *c.dims, **c.kw)
        k = sum(map(ord, c.name))
        sk = eb.skew(s, synth.pruned_weights(s, k), synth.activations(s, k + 1), synth.bias_vector(s, k + 2), k + 3)
        _LAYERS[c.name] = (s, sk, bf16_rne(sk.w), bf16_rne(sk.x))
    return _LAYERS[c.name]
