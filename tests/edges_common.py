"""Shared by test_fp32_edges_cpu.py and test_fp32_edges_gpu.py: the layers, their inputs at the edges of the format
(errbound.edge_inputs), the references -- each computed once from the rounded arrays and never written -- the plain fp32
model of the self-check and the solver's grid of special values.  Imports nothing from the library."""
import numpy as np

import errbound as eb
import seq_common
import solver_common as sc

# the smallest layers at which each kernel still runs (seq_common.LAYERS; test_errbound_gpu.py proves it for each)
# MIXED: G5X5 with seq_common.mixed_weights (conv group 0 is 60 % dense, group 1 keeps 8 %): under dense_threshold_pct=30 the
# plan runs group 0 on the dense kernel and group 1 on a sparse one.  GK: test_errbound_gpu.GK, the stream-K layer
LAYERS = dict(seq_common.LAYERS, MIXED=seq_common.LAYERS["G5X5"], GK=("gk", (64, 1024, 7, 7, 512, 1), dict(sparsity=0.0)))
KINDS = eb.EDGE_KINDS
ALL4 = [(False, False), (True, False), (False, True), (True, True)]      # (bias, relu)
NORMAL = {False: 2.0 ** -126, True: 2.0 ** -1022}                        # the smallest normal number, by f64

_BASE, _EDGE, _FWD, _SKEW, _SKEW_FWD = {}, {}, {}, {}, {}


def out_hw(s):
    return ((s.H + 2 * s.pad_h - (s.dil_h * (s.KH - 1) + 1)) // s.stride_h + 1,
            (s.W + 2 * s.pad_w - (s.dil_w * (s.KW - 1) + 1)) // s.stride_w + 1)


def base(synth, name, spec=None):
    """(shape, w, x, b, top_diff) of order 1, made once per layer; `spec` = (synth name, dims, kwargs) for a layer that
    is not in LAYERS (a row of layout_cases)."""
    if name not in _BASE:
        sname, dims, kw = spec or LAYERS[name]
        s = synth.shape(sname, *dims, **kw)
        k = sum(map(ord, sname)) + 77
        td = np.random.RandomState(k + 3).uniform(-1, 1, (s.N, s.M) + out_hw(s)).astype(np.float32)
        w = seq_common.mixed_weights(s, k) if name == "MIXED" else synth.pruned_weights(s, k)
        _BASE[name] = (s, w, synth.activations(s, k + 1), synth.bias_vector(s, k + 2), td)
    return _BASE[name]


def edge(synth, name, kind, backward=False, f64=False, spec=None):
    """(shape, errbound.Edge) of a layer at an edge, made once; `backward`: with a top_diff (near_max then bounds the
    gradients' sums, not the forward's)."""
    key = (name, kind, backward, f64)
    if key not in _EDGE:
        s, w, x, b, td = base(synth, name, spec)
        _EDGE[key] = eb.edge_inputs(s, w, x, b, kind, KINDS.index(kind) + 11, top_diff=td if backward else None, f64=f64)
    return base(synth, name, spec)[0], _EDGE[key]


def forward_ref(synth, name, kind, bias, relu, f64=False, spec=None):
    """(want, B) of the forward at an edge; the float64 convolution runs once per (layer, kind, bias, dtype)."""
    key = (name, kind, bias, f64)
    if key not in _FWD:
        s, e = edge(synth, name, kind, f64=f64, spec=spec)
        _FWD[key] = eb.forward_bound(s, e.w, e.x, e.b if bias else None, f64=f64)
    want, B = _FWD[key]
    return (np.maximum(want, 0.0) if relu else want), B


def skewed(synth, name, spec=None):
    """(shape, errbound.skew of the layer's inputs and top_diff): the ordinary values of the reach tests, made once."""
    if name not in _SKEW:
        s, w, x, b, td = base(synth, name, spec)
        _SKEW[name] = eb.skew(s, w, x, b, 5, top_diff=td)
    return base(synth, name, spec)[0], _SKEW[name]


def skewed_forward_ref(synth, name, relu, f64=False, spec=None):
    """(want, B) of the forward with bias on the skewed inputs.  A poisoned bottom element changes the reference only
    inside its reach, which the reach tests compare as a set: beside it this reference holds."""
    if (name, f64) not in _SKEW_FWD:
        s, sk = skewed(synth, name, spec)
        _SKEW_FWD[(name, f64)] = eb.forward_bound(s, sk.w, sk.x, sk.b, f64=f64)
    want, B = _SKEW_FWD[(name, f64)]
    return (np.maximum(want, 0.0) if relu else want), B


def plain_fp32_forward(s, w, x, b):
    """The plain fp32 model of the self-check: per output channel its nonzeros in CSR order (input channel, kernel row,
    kernel column ascending), each product rounded to float and added to a float accumulator that starts at +0; the bias
    last.  numpy rounds every operation once in float32 and keeps subnormals."""
    oh, ow = out_hw(s)
    N = x.shape[0]
    cg, mg = s.C // s.group, s.M // s.group
    xp = np.zeros((N, s.C, s.H + 2 * s.pad_h, s.W + 2 * s.pad_w), np.float32)
    xp[:, :, s.pad_h:s.pad_h + s.H, s.pad_w:s.pad_w + s.W] = x
    out = np.zeros((N, s.M, oh, ow), np.float32)
    with np.errstate(all="ignore"):
        for m in range(s.M):
            acc = out[:, m]
            for c, kr, kc in zip(*np.nonzero(w[m])):
                patch = xp[:, (m // mg) * cg + c, kr * s.dil_h:kr * s.dil_h + (oh - 1) * s.stride_h + 1:s.stride_h,
                           kc * s.dil_w:kc * s.dil_w + (ow - 1) * s.stride_w + 1:s.stride_w]
                acc += np.float32(w[m, c, kr, kc]) * patch
            if b is not None:
                acc += np.float32(b[m])
    assert out.dtype == np.float32
    return out


def beyond(got, want, B):
    """The share of elements further than their bound from the reference."""
    with np.errstate(invalid="ignore", over="ignore"):
        bad = ~(np.abs(np.asarray(got, np.float64) - want) <= B)
    return float(bad.mean())


def positive_subnormal(top, f64=False):
    return (top > 0) & (top < NORMAL[f64])


# ---- non-finite reach ------------------------------------------------------------------------------------------------------
def poisoned_bottom(x, positions, value):
    """(the poisoned bottom, the bottom with the poison replaced by 0)."""
    bad, clean = x.copy(), x.copy()
    for p in positions:
        bad[p], clean[p] = value, 0
    return bad, clean


def reader_sign(s, w, pos, out_shape):
    """For a single poisoned bottom element read by at most one nonzero per output: (the outputs that read it, the sign of
    the weight each reads it through), from a float64 convolution of the indicator with sign(w)."""
    ind = eb.poisoned((out_shape[0], s.C, s.H, s.W), [pos]).astype(np.float64)
    sg = eb.conv64(ind, np.sign(w.astype(np.float64)), None, s)
    return sg != 0, sg


# ---- the solver's special values ---------------------------------------------------------------------------------------------
def specials(dt):
    """+-0, +-the smallest subnormal, 3 x that, +-tiny / 2, +-tiny (the smallest normal), tiny (1 + eps), 1e-30, +-1, +-max,
    max / 2, +-sqrt(max), +-inf, NaN in dtype dt: 21 values."""
    fi = np.finfo(dt)
    sub = np.nextafter(dt(0), dt(1))
    t, mx = fi.tiny, fi.max
    with np.errstate(all="ignore"):
        v = [0.0, -0.0, sub, -sub, 3 * sub, t / 2, -t / 2, t, -t, t * (1 + fi.eps), 1e-30, 1.0, -1.0, mx, -mx, mx / 2,
             np.sqrt(mx), -np.sqrt(mx), np.inf, -np.inf, np.nan]
        return np.array(v, dt)


def solver_grid(dt):
    """(w, g, h, h2) flat: every triple of specials(dt) for w, g and h, times every non-negative special for h2 (Adam's
    second moment is a sum of squares)."""
    sp = specials(dt)
    nn = sp[~np.signbit(sp) & ~np.isnan(sp)]
    w, g, h, h2 = np.meshgrid(sp, sp, sp, nn, indexing="ij")
    return tuple(np.ascontiguousarray(a.ravel()) for a in (w, g, h, h2))


# the suite's hyper-parameters (test_solver_step_cpu.HYPER) and a set under which nothing shrinks: sums overflow
HYPERS = [dict(rate=0.01, momentum=0.9, momentum2=0.999, delta=1e-8, decay=5e-4),
          dict(rate=1.0, momentum=0.5, momentum2=0.5, delta=0.0, decay=1.0)]
RULE_REG = [(r, g) for r in ("sgd", "nesterov", "adam") for g in ("none", "L2", "L1")]


def hyper(i, rule, reg):
    return dict(HYPERS[i], type=sc.RULES[rule], regularization=sc.REGS[reg])
