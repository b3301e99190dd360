"""Blobs past 2 GiB and 4 GiB (test_large_blobs_host.py, test_large_blobs_gpu.py): the cases, what each claims to exercise,
and the periodic inputs that let a float64 reference of 28 images check every element of a blob of thousands.

Inputs.  A base of BASE = 4 images skewed by errbound.skew for the case's layer, crossed with SCALES = 7 power-of-two image
scales: image n of the large blob is base[n % 4] * 2^SCALE_EXP[n % 7], so the blob has period 28 in n and image n's
float64 forward and bound are those of pattern image n % 28 (reference()).  A kernel that stores an image 2^31 or 2^32
bytes or elements away from its place, or reads one from there, lands on another image of the pattern, because no power
of two is a multiple of 7: test_large_blobs_host.py proves for every case that such a displacement, and a stale
sentinel, violate the bound somewhere.

On the device (torch): fill_pattern builds the blob by gather, never on the host; guarded allocates a blob between two
1 MiB guard zones of the sentinel; worst_ratio compares in float64, CHUNK_ELEMS elements at a time.
"""
from collections import namedtuple

import numpy as np

import d2s_common as dc
import errbound as eb

BASE, SCALES = 4, 7
PERIOD = BASE * SCALES
SCALE_EXP = (-6, 3, -2, 7, 0, -4, 5)
SENTINEL = -7.5
GUARD_FLOATS = (1 << 20) // 4
CHUNK_ELEMS = 1 << 24             # 128 MiB of float64 per temporary, five temporaries alive at most: under 1 GiB
MAX_CASE_BYTES = 12 << 30
N_CU = 256                        # the MI355X, which the claims below are made for

Layer = namedtuple("Layer", "name C H W M K pad stride dil group sparsity")
LAYERS = dict((l.name, l) for l in [
    Layer("pw_quads", 16, 16, 16, 512, 1, 0, 1, 1, 1, 0.75),       # top image 2^19 bytes, rows of whole quads
    Layer("pw_partial", 16, 7, 7, 512, 1, 0, 1, 1, 1, 0.75),       # top image 100352 bytes, rows ending in a partial quad
    # (rows of 14: the 3x3 / 5x5 asm epilogues need a row shorter than its quads' lanes, which 16 columns are not --
    #  align_rules.h body_variant's fast_epi)
    Layer("c3_top", 16, 14, 14, 256, 3, 1, 1, 1, 1, 0.9),          # top image 200704 bytes
    Layer("c5g2_top", 16, 14, 14, 256, 5, 2, 1, 1, 2, 0.9),
    Layer("c3_top16", 16, 16, 16, 256, 3, 1, 1, 1, 1, 0.9),        # top image 2^18 bytes = 2^16 elements
    Layer("c3_bottom", 256, 16, 16, 16, 3, 1, 1, 1, 1, 0.9),       # bottom image 2^18 bytes
    Layer("c3_bottom14", 256, 14, 14, 16, 3, 1, 1, 1, 1, 0.9),     # bottom image 200704 bytes: the asm epilogue and the chained body
    Layer("pw_bottom", 512, 16, 16, 16, 1, 0, 1, 1, 1, 0.9),       # bottom image 2^19 bytes
    Layer("s2d_bottom", 128, 32, 32, 16, 3, 1, 2, 1, 1, 0.9),      # stride 2: bottom image 2^19 bytes, X' image 512 x 17 x 17
    Layer("s2b_bottom", 512, 16, 16, 16, 3, 2, 1, 2, 1, 0.9),      # dilation 2: bottom image 2^19 bytes, X' four images of 512 x 10 x 10
    Layer("ip_bottom", 4096, 1, 1, 16, 1, 0, 1, 1, 1, 0.9),        # inner product: 2^14 bytes per image
    Layer("sp_strided", 8, 32, 32, 1024, 1, 0, 2, 1, 1, 0.5),      # strided pointwise: top image 2^20 bytes
    Layer("sp_mixed", 8, 32, 32, 1024, 1, 0, 2, 1, 2, 0.75),       # ... in two conv groups, of which the test makes the first dense
    Layer("sx_mfma", 1, 256, 256, 1, 3, 1, 2, 1, 1, 0.0),          # stride 2: bottom image 2^16 elements, top image 2^14
    Layer("one", 1, 1, 1, 1, 1, 0, 1, 1, 1, 0.0),
])

# One forward run.  n: the call's images; plan_n: the batch the plan is made for (> n: a partial batch).  What the case
# claims (test_large_blobs_host.py holds the rules to it, test_large_blobs_gpu.py the device): the kernel family that
# runs, `launches` of launch_tiled, whether the (first, last) launch stores through the asm epilogues (`epi`) and which
# compiled body they run (`body`: 1 the chained one); None where the kernel has no such thing.
Case = namedtuple("Case", "layer n plan_n kernel options launches epi body")


def _case(layer, n, kernel, launches=None, epi=None, body=None, plan_n=None, **options):
    return Case(layer, n, n if plan_n is None else plan_n, kernel, options, launches, epi, body)


def _edge(layer, below, at, body_below, kernels=("AUTO", "TILED", "GENERIC", "DENSE"), stream_stores=False):
    """Top blobs just under and at 2^31 bytes: the asm epilogues below, the element-wise one at; generated code runs the
    chained body where the asm epilogue stores (body_below) and the generic body at the edge; the stream kernel always
    the generic one.  The N below the edge once more as a partial batch of the plan for the N at it."""
    out = []
    for k in kernels:
        if k in ("AUTO", "TILED"):
            b = body_below if k == "AUTO" else 0
            out += [_case(layer, below, k, 1, (1, 1), (b, b)), _case(layer, at, k, 1, (0, 0), (0, 0)),
                    _case(layer, below, k, 1, (1, 1), (b, b), plan_n=at)]
        else:
            out += [_case(layer, below, k), _case(layer, at, k), _case(layer, below, k, plan_n=at)]
    if stream_stores:
        out.append(_case(layer, below, "AUTO", 1, (1, 1), (body_below, body_below), stream_stores=1))
    return out


def _bottom(layer, past, whole, two, body_auto, kernels):
    """Bottom blobs past 2^31 bytes in one launch, the last whole launch, and two launches by the real limit (the second
    starts 4 GiB into the blob); the tops are small, so no launch is kept from the asm epilogues by its size (rows of 16
    columns keep the 3x3 layer from them, and from the chained body: body_auto = 0).  DENSE and GENERIC run where they
    accept the size."""
    out = []
    for k in kernels:
        if k in ("AUTO", "TILED"):
            b = body_auto if k == "AUTO" else 0
            out += [_case(layer, past, k, 1, (1, 1), (b, b)), _case(layer, whole, k, 1, (1, 1), (b, b)),
                    _case(layer, two, k, 2, (1, 1), (b, b)), _case(layer, whole, k, 1, (1, 1), (b, b), plan_n=two)]
        elif k == "DENSE":
            out += [_case(layer, past, k), _case(layer, whole, k)]
        else:
            out += [_case(layer, past, k), _case(layer, whole, k), _case(layer, two, k)]
    return out


FORWARD = (_edge("pw_quads", 4095, 4096, 1, ("AUTO", "TILED"), stream_stores=True) +
           _edge("pw_partial", 21399, 21400, 1, ("AUTO", "TILED")) +
           _edge("c3_top", 10699, 10700, 1) +
           _edge("c5g2_top", 10699, 10700, 1, ("AUTO", "TILED")) +
           _bottom("c3_bottom", 8193, 16383, 16385, 0, ("AUTO", "TILED", "DENSE")) +
           _bottom("c3_bottom14", 10700, 21399, 21401, 1, ("AUTO",)) +
           _bottom("pw_bottom", 4097, 8191, 8193, 1, ("AUTO", "TILED", "GENERIC")) +
           # top past 2^31 ELEMENTS (8 GiB)
           [_case("c3_top16", 32769, "AUTO", 1, (0, 0), (0, 0)), _case("c3_top16", 32769, "GENERIC")])


# Plans that run an inner plan on a rearranged bottom (layer, images, option): the bottom and X' both pass 4 GiB under
# "s2d" and "s2b" (under "s2b" with 512 channels at 8193 images: 256 at 16385 would be 65540 inner images, five more than
# s2b_plan takes); under "b2s" they pass 2 GiB -- the plan holds X' twice (X' and dX'), which with the bottom passes the
# 12 GiB a case may hold once each of them passes 4.
INNER = [("s2d_bottom", 8193, "s2d"), ("s2b_bottom", 8193, "s2b"), ("ip_bottom", 32769 * 4, "b2s")]


def case_id(c):
    opts = "".join("-%s%d" % kv for kv in sorted(c.options.items()))
    return "%s-%d%s-%s%s" % (c.layer, c.n, "" if c.plan_n == c.n else "of%d" % c.plan_n, c.kernel, opts)


def shape(synth, layer, n):
    l = LAYERS[layer] if isinstance(layer, str) else layer
    return synth.shape(l.name, n, l.C, l.H, l.W, l.M, l.K, pad=l.pad, stride=l.stride, dil=l.dil, group=l.group, sparsity=l.sparsity)


def top_image_elems(synth, layer):
    s = shape(synth, layer, 1)
    oh, ow = synth.out_hw(s)
    return s.M * oh * ow


_PATTERNS = {}


def _activations(synth, s, seed, layer):
    """synth's activations; of one sign on MFMA_LAYER, whose weight gradient has 5 x 10^8 terms per element: with mixed
    signs what is left after cancellation is smaller than the bound of the sum, and a kernel that lost half the batch
    would pass."""
    x = synth.activations(s, seed)
    return np.abs(x) if layer == MFMA_LAYER else x


def pattern(synth, layer):
    """(shape of PERIOD images, skewed weights, bias, base images (BASE, C, H, W), the PERIOD pattern images) of a layer,
    made once: pattern image k = base[k % BASE] * 2^SCALE_EXP[k % SCALES]."""
    if layer not in _PATTERNS:
        s4 = shape(synth, layer, BASE)
        k = sum(map(ord, layer)) + 77
        w, x, b = synth.pruned_weights(s4, k), _activations(synth, s4, k + 1, layer), synth.bias_vector(s4, k + 2)
        sk = eb.skew(s4, w, x, b, k + 3)
        idx = np.arange(PERIOD)
        x28 = sk.x[idx % BASE] * np.ldexp(np.float32(1.0), np.array(SCALE_EXP)[idx % SCALES]).astype(np.float32)[:, None, None, None]
        _PATTERNS[layer] = (shape(synth, layer, PERIOD), sk.w, sk.b, sk.x, np.ascontiguousarray(x28))
    return _PATTERNS[layer]


_REFS = {}


def reference(synth, layer):
    """(want, B): the float64 forward with bias and ReLU of the PERIOD pattern images and its bound, computed once and
    never written to."""
    if layer not in _REFS:
        s28, w, b, _, x28 = pattern(synth, layer)
        want, B = eb.forward_bound(s28, w, x28, b, relu=True)
        want.setflags(write=False)
        B.setflags(write=False)
        _REFS[layer] = (want, B)
    return _REFS[layer]


# ---- the Backward: top_diff is the large blob (16 -> 256 3x3 on 16 x 16: the bottom of the transposed plan) -----------------
BWD_LAYER = "c3_top16"
BWD_DATA = [(n, k) for n in (8193, 16385) for k in ("AUTO", "JIT", "TILED", "GENERIC")]
# (images, option "wgrad_kernel"): 32769 images put top_diff past 2^31 ELEMENTS.  That is a limit of the STAGED kernel's
# (stg_plan: N*M*OH*OW below 2^31), which refuses the batch (STAGED_REFUSAL); wgm_plan accepts it -- its limits are
# N*OH*OW, M*Cg*KH*KW and Cg*H*W, and its kernel indexes top_diff in 64 bits -- so the MFMA kernel runs there as the
# entry kernel does.
# One image past an edge weighs less than the bound of the whole sum, so each edge has a second batch 512 / 1024 images
# past it: there what lies past the edge, lost or paired with the wrong top_diff, breaks the bound
# (test_large_blobs_host.py proves which faults which batch shows).
BWD_WGRAD = [(n, k) for n in (16385, 16896, 32769, 33792) for k in ("ENTRY", "STAGED", "MFMA")]
BWD_EDGES = (8192, 16384, 32768)      # images of top_diff at 2^31 and 2^32 bytes and at 2^31 elements

# The MFMA data gradient and the dense weight gradient on the matrix cores at the largest batch their plans accept on a
# strided shape: 1 -> 1 channels, 3x3, stride 2, on 256 x 256, N*H*W = 2^31 - 2^16 at 32767 images; 32768 is refused
# (dgm_plan, wgm_plan: N*H*W and N*OH*OW below 2^31 -- the latter only from 131072 images on, so it is dgm_plan's
# limit that one more image passes, and dense_wgrad's at a batch no device holds).
MFMA_LAYER = "sx_mfma"
MFMA_MAX_IMAGES = 32767
DGM_REFUSAL = "backward_kernel: the MFMA data-gradient kernel needs a float plan whose pixel, top and matrix indices fit 31 bits"

# ---- the launch-time refusals (layer, images, which kernel's verdict in launch_limits_check's output, the message) -----
DENSE_RANGE = "dense kernel: bottom blob or weight matrix exceeds the 4 GiB descriptor range"
STRIDED_TOP = "tiled kernel: strided pointwise layer with a top blob of 2 GiB or more"
GENERIC_GRID = "generic kernel: grid dimension exceeds 65535"
REFUSALS = [("c3_bottom", 16384, "dense_error", DENSE_RANGE), ("sp_strided", 2048, "tiled_error", STRIDED_TOP),
            ("one", 65536, "generic_error", GENERIC_GRID)]
STAGED_REFUSAL = "wgrad_kernel: the staged weight-gradient kernel needs a float plan with stride 1"
STAGED_MAX_IMAGES = 32767         # of BWD_LAYER: 32768 x 256 x 16 x 16 is 2^31

_BWD = {}


def bwd_pattern(synth, layer=BWD_LAYER):
    """(top_diff base images (BASE, M, OH, OW), the PERIOD top_diff pattern images): pattern image k of top_diff is
    base[k % BASE] * 2^SCALE_EXP[k % SCALES], as for the bottom."""
    if layer not in _BWD:
        from wgrad_common import seeded
        s4 = shape(synth, layer, BASE)
        k = sum(map(ord, layer)) + 77
        w, x, b = synth.pruned_weights(s4, k), _activations(synth, s4, k + 1, layer), synth.bias_vector(s4, k + 2)
        oh, ow = synth.out_hw(s4)
        # (top_diff of one sign: an image's bias gradient is then the sum of its magnitudes, and a batch that counts other
        #  images than its own moves the bias gradient by whole images, not by what is left of them after cancellation)
        sk = eb.skew(s4, w, x, b, k + 3, top_diff=np.abs(seeded((BASE, s4.M, oh, ow), k + 4)))
        assert np.array_equal(sk.w, pattern(synth, layer)[1]) and np.array_equal(sk.x, pattern(synth, layer)[3])
        idx = np.arange(PERIOD)
        td28 = sk.top_diff[idx % BASE] * np.ldexp(np.float32(1.0), np.array(SCALE_EXP)[idx % SCALES]).astype(np.float32)[:, None, None, None]
        _BWD[layer] = (sk.top_diff, np.ascontiguousarray(td28))
    return _BWD[layer]


_BWD_REFS = {}


def bwd_reference(synth, layer=BWD_LAYER):
    """Without ReLU.  (bottom_diff of the PERIOD pattern images, its bound): image n's data gradient is pattern image
    n % PERIOD's."""
    if layer not in _BWD_REFS:
        s28, w, b, _, x28 = pattern(synth, layer)
        want, Bs = eb.backward_bound(s28, w, x28, b, bwd_pattern(synth, layer)[1])
        _BWD_REFS[layer] = (want[0], Bs[0])
    return _BWD_REFS[layer]


_PAIRS = {}


def pair_gradients(synth, shift=0, layer=BWD_LAYER):
    """Per pattern image k the float64 weight and bias gradient of ONE image whose bottom is pattern image k and whose
    top_diff is pattern image (k - shift) % PERIOD, and the same of the magnitudes: (wd, bd, wmag, bmag), each
    (PERIOD, ...).  shift = 0 is the batch as it is; another shift is what a kernel pairs up whose top_diff offset lost
    `shift` images."""
    key = (layer, shift % PERIOD)
    if key not in _PAIRS:
        from wgrad_common import torch_backward
        s28, w, b, _, x28 = pattern(synth, layer)
        td28 = np.roll(bwd_pattern(synth, layer)[1], shift % PERIOD, axis=0)      # td28[k] = pattern image k - shift
        per = [torch_backward(x28[k:k + 1], w, b, s28, td28[k:k + 1]) for k in range(PERIOD)]
        mag = [torch_backward(np.abs(x28[k:k + 1]), np.abs(w), np.abs(b), s28, np.abs(td28[k:k + 1]), mask=(w != 0)) for k in range(PERIOD)]
        _PAIRS[key] = (np.stack([p[1] for p in per]), np.stack([p[2] for p in per]), np.stack([m[1] for m in mag]), np.stack([m[2] for m in mag]))
    return _PAIRS[key]


def _counts(lo, hi):
    """How often each pattern image occurs among images lo .. hi - 1."""
    return np.array([max(0, (hi - k + PERIOD - 1) // PERIOD) - max(0, (lo - k + PERIOD - 1) // PERIOD) for k in range(PERIOD)], np.float64)


def batch_gradient(synth, n, layer=BWD_LAYER, lost_from=None, displaced=0):
    """(weight_diff, bias_diff, their magnitude sums) in float64 of a batch of n images: the sum of the pattern images'
    gradients, each as often as it occurs.  lost_from: the images from there on contribute nothing (a kernel that loses
    what lies past an offset); displaced = d: images n >= d are paired with top_diff[n - d] (a top_diff offset that lost
    d images)."""
    hi = n if lost_from is None else min(n, lost_from)
    parts = [(0, _counts(0, min(hi, displaced) if displaced else hi))]
    if displaced:
        parts.append((displaced, _counts(min(displaced, hi), hi)))
    out = [0.0, 0.0, 0.0, 0.0]
    for shift, counts in parts:
        for i, g in enumerate(pair_gradients(synth, shift, layer)):
            out[i] = out[i] + (g * counts.reshape((-1,) + (1,) * (g.ndim - 1))).sum(axis=0)
    return tuple(out)


def reduction_depth(synth, n, layer=BWD_LAYER, chunk_span=1):
    """The most additions one term of a weight or bias gradient passes through in the Backward's two-stage reduction
    (sconv_backward.hip, wgrad_mfma.hip, dense_wgrad.hip): stage 1 sums a span of chunk_span chunks of kBwdChunkPixels =
    1024 flattened pixels into one partial, in whatever order; stage 2 sums the partials."""
    oh, ow = synth.out_hw(shape(synth, layer, 1))
    chunks = -(-n * oh * ow // 1024)
    return 1024 * chunk_span + -(-chunks // chunk_span)


def weight_reference(synth, n, layer=BWD_LAYER, chunk_span=1):
    """((weight_diff, bias_diff), (their bounds)) of a batch of n images accumulated into zeroed blobs.  The bound is
    errbound's for a sum, gamma(k + 4) x the sum of the magnitudes, with k = reduction_depth, not the n * OH * OW terms of
    an element: in a sum of any order each term passes through at most as many roundings as the additions it takes part
    in (Higham, section 4.2), which the two-stage reduction keeps at 1024 + chunks.  With k = the number of terms gamma
    passes 1 at these batches and the bound would hold for a kernel that writes nothing.  accumulated_bound adds the zero
    prefill as one more term."""
    wd, bd, wmag, bmag = batch_gradient(synth, n, layer)
    depth = reduction_depth(synth, n, layer, chunk_span)
    kw = float(depth + 4)
    bounds = tuple(eb.accumulated_bound(eb.gamma(kw) * m + kw * eb.TINY, np.zeros_like(m), depth) for m in (wmag, bmag))
    return (wd, bd), bounds


def displaced_violates(want, B, elems):
    """Whether a top blob whose every element comes from `elems` elements further on in the periodic blob -- what a store
    or a load whose offset lost 2^31 or 2^32 shows -- violates the bound on at least one element of EVERY image."""
    flat = want.reshape(-1)
    moved = np.roll(flat, -(elems % flat.size)).reshape(want.shape)
    bad = np.abs(moved - want) > B
    return bool(bad.reshape(want.shape[0], -1).any(axis=1).all())


# ---- on the device ----------------------------------------------------------------------------------------------------
def need_bytes(*elem_counts):
    """Device bytes of a case: its float blobs, their guard zones and 1 GiB for the comparison's temporaries and the plan."""
    return sum(4 * (e + 2 * GUARD_FLOATS) for e in elem_counts) + (1 << 30)


def require_memory(torch, pytest, need, what):
    assert need <= MAX_CASE_BYTES, (what, need)
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.fail("%s needs %.2f GiB of device memory, %.2f GiB are free" % (what, need / 2.0 ** 30, free / 2.0 ** 30))


def guarded(torch, dev, shape_):
    """(the allocation, the blob): a contiguous float blob of `shape_` with GUARD_FLOATS of the sentinel before and after,
    itself filled with the sentinel."""
    numel = int(np.prod(shape_, dtype=np.int64))
    buf = torch.full((numel + 2 * GUARD_FLOATS,), SENTINEL, device=dev, dtype=torch.float32)
    blob = buf[GUARD_FLOATS:GUARD_FLOATS + numel].view(*shape_)
    assert blob.data_ptr() % 16 == 0 and blob.is_contiguous()
    return buf, blob


def guards_intact(buf):
    return bool((buf[:GUARD_FLOATS] == SENTINEL).all()) and bool((buf[-GUARD_FLOATS:] == SENTINEL).all())


def all_sentinel(torch, blob):
    """Every element of `blob` still holds the sentinel (in chunks: no temporary of the blob's size)."""
    flat = blob.reshape(-1)
    step = 1 << 28
    return all(bool((flat[i:i + step] == SENTINEL).all()) for i in range(0, flat.numel(), step))


def fill_pattern(torch, out, base):
    """out[n] = base[n % BASE] * 2^SCALE_EXP[n % SCALES] for the images of `out`, gathered on the device."""
    n, per = out.shape[0], out[0].numel()
    scales = torch.tensor(np.ldexp(1.0, np.array(SCALE_EXP)), dtype=torch.float32, device=out.device)
    step = max(1, (1 << 26) // per)
    for n0 in range(0, n, step):
        idx = torch.arange(n0, min(n, n0 + step), device=out.device)
        torch.mul(base[idx % BASE], scales[idx % SCALES].view(-1, 1, 1, 1), out=out[n0:n0 + idx.numel()])


def worst_ratio(torch, got, want, B, first_image=0):
    """(worst |got - want| / B over every element of got, index of the first violation or None): image i of `got` is held
    to pattern image (first_image + i) % PERIOD of want / B (float64, on the device).  A NaN or an infinity counts as an
    infinite ratio."""
    n, per = got.shape[0], got[0].numel()
    step = max(1, CHUNK_ELEMS // per)
    worst = torch.zeros((), dtype=torch.float64, device=got.device)
    bad_from = []
    inf = torch.tensor(float("inf"), dtype=torch.float64, device=got.device)
    for n0 in range(0, n, step):
        n1 = min(n, n0 + step)
        idx = (torch.arange(n0, n1, device=got.device) + first_image) % PERIOD
        g = got[n0:n1].double()
        r = (g - want[idx]).abs_().div_(B[idx])
        r = torch.where(torch.isfinite(g), r, inf)
        m = r.max()
        worst = torch.maximum(worst, m)
        if not bad_from and not float(m) <= 1.0:
            at = int((r.reshape(-1) > 1.0).to(torch.uint8).argmax()) if bool((r > 1.0).any()) else int(torch.isnan(r.reshape(-1)).to(torch.uint8).argmax())
            bad_from.append(tuple(int(v) for v in np.unravel_index(n0 * per + at, tuple(got.shape))))
        del g, r
    return float(worst), (bad_from[0] if bad_from else None)


# ---- option "deconv": the top and the plan's own scratch T' past 2 and 4 GiB ---------------------------------------------------
# Deconvolution 16 -> 64 channels, 16 x 16 bottom, k4 s2 p1, 90 % sparse: the top image is 64 x 32 x 32 = 2^16 elements (2^18
# bytes, so the 7-scale period argument applies to the top as written); the inner layer has 256 channels, a 2 x 2 kernel and
# pad 1, so a T' image is 256 x 17 x 17 = 73984 elements -- no power of two: test_large_blobs_host.py runs the displacement
# proof for it.  d2s.hip indexes with 32-bit ELEMENT offsets, which d2s_plan keeps below 2^31; the byte offsets pass 2^31
# and 2^32 here.
DC_LAYER = dc.DShape("dc_top", 1, 16, 16, 16, 64, 4, 4, 2, 2, 1, 1, 1)
DC_DENSITY = 0.1
DC_TOP_IMAGE, DC_T_IMAGE = 64 * 32 * 32, 256 * 17 * 17
# (images of the call, the plan's batch, the inner kernel).  8191 / 8192: the top just under and at 2^31 bytes, T' past it
# (2.26 GiB); 8191 of 8192: the partial batch; 16385: the top one image past 2^32 bytes, T' 4.52 GiB -- every byte offset of
# d2s.hip passes 2^32 while its element offset stays under 2^31; about 8.8 GiB.  Under an inner GENERIC as far as that kernel
# accepts the size (the GPU test records which do).
DcCase = namedtuple("DcCase", "n plan_n kernel")
DC_FORWARD = [DcCase(n, p, k) for k in ("AUTO", "GENERIC") for n, p in ((8191, 8191), (8192, 8192), (8191, 8192), (16385, 16385))]
# top_diff past 2 GiB, packed into a G' of 2.26 GiB in the plan's scratch; the inner plan's backward state comes on top
# (profiles/errbound.md has the measured peak).  The backward is run at this one batch: with top_diff past 4 GiB the blobs,
# the scratch and what the inner backward keeps of G''s size come too close to the 12 GiB a case may hold.
DC_BACKWARD_N = 8193
DC_REFUSED_N = 32768              # the top is exactly 2^31 elements
DC_TOP_REFUSAL = "option \"deconv\": the top blob reaches 2^31 elements"


def dc_case_id(c):
    return "dc_top-%d%s-%s" % (c.n, "" if c.plan_n == c.n else "of%d" % c.plan_n, c.kernel)


def dc_shape(n):
    return DC_LAYER._replace(N=n)


def _dc_scaled(base):
    idx = np.arange(PERIOD)
    return np.ascontiguousarray(base[idx % BASE] * np.ldexp(np.float32(1.0), np.array(SCALE_EXP)[idx % SCALES]).astype(np.float32)[:, None, None, None])


def dc_pattern():
    """(shape of PERIOD images, skewed weights C x Mg x KH x KW, bias, base images, the PERIOD pattern images, top_diff base
    images, the PERIOD top_diff pattern images) of DC_LAYER, as pattern() and bwd_pattern() make a convolution's: the skew
    per output channel (d2s_seq_common.to_rows), top_diff of one sign."""
    if "dc" not in _PATTERNS:
        from wgrad_common import seeded
        import d2s_seq_common as ds
        s4 = dc_shape(BASE)
        k = sum(map(ord, s4.name)) + 77
        w = dc.weights(s4, k, DC_DENSITY)
        rs = np.random.RandomState(k + 1)
        x = rs.uniform(-1, 1, (BASE, s4.C, s4.H, s4.W)).astype(np.float32)
        b = rs.uniform(-0.5, 0.5, s4.M).astype(np.float32)
        td = np.abs(seeded((BASE, s4.M) + dc.out_hw(s4), k + 4))
        sk = eb.skew(s4, ds.to_rows(s4, w), x, b, k + 3, top_diff=td)
        _PATTERNS["dc"] = (dc_shape(PERIOD), ds.from_rows(s4, sk.w), sk.b, sk.x, _dc_scaled(sk.x), sk.top_diff, _dc_scaled(sk.top_diff))
    return _PATTERNS["dc"]


def dc_reference(synth):
    """(want, B) of the top: d2s_common.forward_bound with bias and ReLU on the PERIOD pattern images, read-only."""
    if "dc" not in _REFS:
        s28, w, b, _, x28 = dc_pattern()[:5]
        want, B = dc.forward_bound(eb, synth, s28, w, x28, b, relu=True)
        want.setflags(write=False)
        B.setflags(write=False)
        _REFS["dc"] = (want, B)
    return _REFS["dc"]


def dc_inner_top(synth):
    """T' of the PERIOD pattern images in float64 (the inner forward; the unpack kernel adds the bias)."""
    s28, w, _, _, x28 = dc_pattern()[:5]
    return eb.conv64(x28, dc.inner_weights(s28, w)[0], None, dc.inner_shape(synth, s28))


def dc_top_of(s, t, b):
    """The top the unpack rule makes of a T' (float64), with bias and ReLU."""
    return dc.unpack(s, t, b.astype(np.float64), relu=True)


def dc_bwd_reference(synth):
    """(bottom_diff of the PERIOD pattern images, its bound), without ReLU."""
    if "dc" not in _BWD_REFS:
        s28, w, _, _, x28, _, td28 = dc_pattern()
        want, Bs = dc.backward_bound(eb, synth, s28, w, x28, td28)
        _BWD_REFS["dc"] = (want[0], Bs[0])
    return _BWD_REFS["dc"]


def dc_pair_gradients():
    """Per pattern image the float64 weight and bias gradient of that ONE image and the same of the magnitudes (torch's
    conv_transpose2d autograd): (wd, bd, wmag, bmag), each (PERIOD, ...)."""
    if "dc" not in _PAIRS:
        s28, w, b, _, x28, _, td28 = dc_pattern()
        per = [dc.ref_backward(s28, w, x28[k:k + 1], b, td28[k:k + 1]) for k in range(PERIOD)]
        mag = [dc.ref_backward(s28, np.abs(w), np.abs(x28[k:k + 1]), np.abs(b), np.abs(td28[k:k + 1])) for k in range(PERIOD)]
        _PAIRS["dc"] = (np.stack([p[1] for p in per]), np.stack([p[2] for p in per]), np.stack([m[1] for m in mag]), np.stack([m[2] for m in mag]))
    return _PAIRS["dc"]


def dc_weight_reference(n, lost_from=None):
    """((weight_diff, bias_diff), (their bounds)) of a batch of n images accumulated into zeroed blobs, as weight_reference:
    the sum of the pattern images' gradients, each as often as it occurs; the bound is the depth of the inner plan's
    two-stage reduction over its n * H' * W' top pixels (the suite's rule, not the term count), the carry kernel's addition
    onto the zero prefill as one more term, and for the bias the P phase sums on top (gamma(k + P), as
    d2s_common.backward_bound)."""
    counts = _counts(0, n if lost_from is None else min(n, lost_from))
    wd, bd, wmag, bmag = [(g * counts.reshape((-1,) + (1,) * (g.ndim - 1))).sum(axis=0) for g in dc_pair_gradients()]
    P, _, _, hi, wi = dc.inner_dims(DC_LAYER)
    depth = 1024 + -(-n * hi * wi // 1024)
    bounds = []
    for m, extra in ((wmag, 0), (bmag, P)):
        k = float(depth + extra + 4)
        bounds.append(eb.accumulated_bound(eb.gamma(k) * m + k * eb.TINY, np.zeros_like(m), depth + extra))
    return (wd, bd), tuple(bounds)
