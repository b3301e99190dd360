"""Plan option "deconv" at the edges of fp32: shared by test_d2s_edges_cpu.py and test_d2s_edges_gpu.py.  The layer that runs is
the inner stride-1 layer, so the edge inputs are errbound.edge_inputs applied to THAT layer (d2s_common.inner_shape,
inner_weights, the bias repeated over a channel's P phases, top_diff packed) and mapped back to the caller's arrays: the
weights through the entry map, top_diff through unpack (pack is a bijection from the top's positions onto the inner positions
it fills; the others are +0 and stay +0 under every scaling), the bias read from one phase -- edge_inputs scales a bias by
one power of two, so it stays equal over the phases, and the per-row exponents of the weights may differ between the inner
rows of one channel since every weight maps back on its own.  Every reference is computed once and never written.  Imports
nothing from the library."""
import numpy as np

import d2s_common as dc
import d2s_seq_common as ds
import errbound as eb

# the sequence suite's decoder layer (forced inner kernels exist), phases without taps (sw > KW: those outputs are the bias
# alone), and a crop that removes whole inner rows
LAYERS = {"k4s2p1": ds.LAYERS["DK4"], "k3x2_s2x3": dc.make("k3x2_s2x3"), "k2s2p2": dc.make("k2s2p2")}
DENSITY = {"k4s2p1": 0.1, "k3x2_s2x3": 0.4, "k2s2p2": 0.5}
KINDS = eb.EDGE_KINDS
ALL4 = [(False, False), (True, False), (False, True), (True, True)]      # (bias, relu)
NORMAL = 2.0 ** -126

_BASE, _EDGE, _FWD, _SKEW, _SKEW_FWD = {}, {}, {}, {}, {}


def base(name):
    """(shape, w, x, b, top_diff) of order 1, made once per layer."""
    if name not in _BASE:
        s = LAYERS[name]
        k = sum(map(ord, name)) + 77
        _BASE[name] = (s, dc.weights(s, k, DENSITY[name])) + dc.inputs(s, k + 1)
    return _BASE[name]


def map_back(s, at, inner):
    """The caller's Edge(w, x, b, top_diff) of an inner layer's."""
    P = dc.inner_dims(s)[0]
    return eb.Edge(np.ascontiguousarray(inner.w.reshape(-1)[at]), inner.x, None if inner.b is None else np.ascontiguousarray(inner.b.reshape(s.M, P)[:, 0]),
                   None if inner.top_diff is None else np.ascontiguousarray(dc.unpack(s, inner.top_diff)))


def edge(synth, name, kind, backward=False):
    """(shape, the layer's Edge, the inner layer's shape, the inner layer's Edge) at an edge, made once."""
    key = (name, kind, backward)
    if key not in _EDGE:
        s, w, x, b, td = base(name)
        P = dc.inner_dims(s)[0]
        wi, at = dc.inner_weights(s, w)
        si = dc.inner_shape(synth, s)
        inner = eb.edge_inputs(si, wi, x, np.repeat(b, P), kind, KINDS.index(kind) + 11, top_diff=dc.pack(s, td) if backward else None)
        _EDGE[key] = (s, map_back(s, at, inner), si, inner)
    return _EDGE[key]


def forward_ref(synth, name, kind, bias, relu):
    key = (name, kind, bias)
    if key not in _FWD:
        s, e = edge(synth, name, kind)[:2]
        _FWD[key] = dc.forward_bound(eb, synth, s, e.w, e.x, e.b if bias else None)
    want, B = _FWD[key]
    return (np.maximum(want, 0.0) if relu else want), B


def skewed(name):
    """(shape, errbound.skew of the layer's inputs and top_diff, weights back in C x Mg x KH x KW): the ordinary values of
    the reach tests; the row exponent is per output channel."""
    if name not in _SKEW:
        s, w, x, b, td = base(name)
        sk = eb.skew(s, ds.to_rows(s, w), x, b, 5, top_diff=td)
        _SKEW[name] = sk._replace(w=ds.from_rows(s, sk.w))
    return base(name)[0], _SKEW[name]


def skewed_forward_ref(synth, name, relu):
    if name not in _SKEW_FWD:
        s, sk = skewed(name)
        _SKEW_FWD[name] = dc.forward_bound(eb, synth, s, sk.w, sk.x, sk.b)
    want, B = _SKEW_FWD[name]
    return (np.maximum(want, 0.0) if relu else want), B


def positive_subnormal(top):
    return (top > 0) & (top < NORMAL)


def plain_fp32_forward(synth, s, w, x, b):
    """The plain fp32 model of the decomposition: edges_common.plain_fp32_forward of the inner layer (bias[m] the bias of m's
    P inner channels), read through unpack."""
    import edges_common as ec
    P = dc.inner_dims(s)[0]
    wi, _ = dc.inner_weights(s, w)
    t = ec.plain_fp32_forward(dc.inner_shape(synth, s, x.shape[0]), wi, x, None if b is None else np.repeat(b, P))
    return dc.unpack(s, t)


# ---- reach: the inner layer's, read through unpack / pack ------------------------------------------------------------------------
def bottom_positions(synth, s, w, n_images=None):
    """errbound.poison_positions on the bottom blob (the inner layer's own bottom)."""
    return eb.poison_positions(dc.inner_shape(synth, s), dc.inner_weights(s, w)[0], n_images)


def top_positions(s, w, n_images=None):
    """errbound.poison_positions_top on the layer's top: each on the nearest output channel that has a weight."""
    return eb.poison_positions_top(s, ds.to_rows(s, w), dc.out_hw(s), n_images)


def reach_forward(synth, s, w, poisoned, dense=False):
    si = dc.inner_shape(synth, s, poisoned.shape[0])
    r = eb.reach_forward_dense(si, poisoned) if dense else eb.reach_forward(si, dc.inner_weights(s, w)[0], poisoned)
    return dc.unpack(s, r)


def reach_data(synth, s, w, poisoned_top_diff, dense=False):
    si = dc.inner_shape(synth, s, poisoned_top_diff.shape[0])
    g = dc.pack(s, np.asarray(poisoned_top_diff, np.float64)) > 0
    return eb.reach_data_dense(si, g) if dense else eb.reach_data(si, dc.inner_weights(s, w)[0], g)


def reader_sign(synth, s, w, pos, n_images):
    """edges_common.reader_sign of the inner layer through unpack: (the outputs that read the bottom element at pos, the
    sign of the weight each reads it through)."""
    import edges_common as ec
    si = dc.inner_shape(synth, s, n_images)
    _, sg = ec.reader_sign(si, dc.inner_weights(s, w)[0], pos, (n_images,))
    sg = dc.unpack(s, sg)
    return sg != 0, sg


def masked_top_case(s, sk, top):
    """test_fp32_edges_cpu.masked_top_case on the layer's own top: NaN in top_diff under tops of 0, -1, NaN and -0.0."""
    from test_fp32_edges_cpu import masked_top_case as case
    return case(s, sk, top, ds.to_rows(s, sk.w), dc.out_hw(s))


def accumulate_terms(s, n):
    """(terms of a weight entry's sum, terms of a bias element's) as errbound.accumulated_bound counts them: the inner
    top's positions; the bias sums its P phases on top of that (d2s_common.backward_bound's gamma(k + P) / gamma(k))."""
    P, _, _, hi, wi = dc.inner_dims(s)
    return n * hi * wi, n * hi * wi + P
