"""Shared by test_depthwise_host.py and test_depthwise_gpu.py: the shapes plan option "depthwise" is tested on -- the
smallest at which each piece of csrc/depthwise.hip can go wrong -- and the plans the option must leave alone."""
import numpy as np

BAND_ROWS = (0, 1, 2)
BWD_DEPTHWISE = 6
WAVE_LDS = 8 * 1024

# name: (N, C, H, W, M, KH, kwargs of synth.shape); group = C throughout
SHAPES = {
    "3x3_s1": (2, 5, 9, 7, 5, 3, dict(pad=1)),                      # odd width: unaligned rows, no 16-byte path, 5 units on 4 waves
    "3x3_s2": (2, 6, 11, 10, 6, 3, dict(pad=1, stride=2)),          # the phase predicate; bottom rows no window reads
    "mult2": (2, 3, 8, 8, 6, 3, dict(pad=1)),                       # Mg = 2: the ocl loop, the data gradient's sum across ocl
    "5x5_dil2": (1, 4, 12, 12, 4, 5, dict(pad=4, dil=2)),           # dilation; the band's row count
    "3x1_s1x2": (2, 4, 9, 12, 4, 3, dict(KW=1, pad=1, pad_w=0, stride_w=2)),   # asymmetric everything
    "img7": (3, 9, 7, 7, 9, 3, dict(pad=1)),                        # one band per unit, idle lanes, units no multiple of 4
    "wide": (1, 2, 5, 70, 2, 3, dict(pad=1)),                       # a row longer than a wave
    "g130": (1, 130, 6, 6, 130, 3, dict(pad=1)),                    # more than 64 groups
    "pruned": (2, 6, 8, 8, 6, 3, dict(pad=1, sparsity=0.6)),        # pruned taps and an empty row
}
# a plan the option does not serve: two input channels per group (a double plan, a forced kernel and a lowered mode are the tests')
CG2 = (2, 8, 8, 8, 4, 3, dict(pad=1, group=4))


def make(synth, name):
    N, C, H, W, M, K, kw = CG2 if name == "cg2" else SHAPES[name]
    return synth.shape(name, N, C, H, W, M, K, **dict(dict(group=C, sparsity=0.0), **kw))


def case(synth, name):
    """(shape, weights, bottom, bias, top_diff): made once per name, never written.  "pruned": channel 0's row is emptied."""
    if name not in _CASES:
        s = make(synth, name)
        w = synth.pruned_weights(s, 11)
        if name == "pruned":
            w[0] = 0
        td = synth.uniform(21, s.N * s.M * int(np.prod(synth.out_hw(s)))).reshape((s.N, s.M) + tuple(synth.out_hw(s)))
        _CASES[name] = (s, w, synth.activations(s, 12), synth.bias_vector(s, 13), td)
    return _CASES[name]


_CASES = {}
