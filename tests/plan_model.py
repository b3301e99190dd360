"""A model of a plan for the sequence tests (seq_common.py, test_sequence_cpu.py, test_sequence_gpu.py).  Imports nothing
from the library: every method is a thin composition of the restatements the single-op tests already trust
(solver_common.step, prune_common, rewire_common, errbound).

The state: the layer (a synth shape, or anything with its geometry fields), the pattern as ascending flat positions of
blobs_[0], the values in the plan's dtype -- kept BIT-EXACT -- the optional solver histories in CSR order, and the counters
the stats report.  The model stays exact because it never computes a gradient itself: solver_step takes the gradient's
bits, rewire the score's, from a caller that has checked them against forward_bound / backward_bound first."""
from collections import namedtuple

import numpy as np

import d2s_common as dc
import errbound as eb
import prune_common as pc
from prune_common import positions  # noqa: F401  (the tests take it from here)
import rewire_common as rc
import solver_common as sc


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


COUNTERS = ("prune_count", "prune_last_dropped", "rewire_count", "rewire_last_dropped", "rewire_last_grown", "update_count")


class PlanModel(object):
    def __init__(self, desc, pos, values, relu=False, in_place=True):
        """desc: the layer; pos: ascending flat positions; values: one per position, float32 or float64 (the plan's dtype).
        in_place: whether the plan kind updates in place (stat update_fast == 1); a fast import suspends it once."""
        self.desc, self.relu, self.in_place = desc, bool(relu), bool(in_place)
        self.pos = np.ascontiguousarray(pos, np.int64)
        self.values = np.ascontiguousarray(values).copy()
        assert self.values.dtype in (np.float32, np.float64) and self.values.shape == self.pos.shape
        assert np.all(np.diff(self.pos) > 0) and (self.pos.size == 0 or 0 <= self.pos[0] and self.pos[-1] < self.dense_size)
        self.h = self.h2 = None
        self.stats = dict.fromkeys(COUNTERS, 0)
        self.no_value_map = False         # a fast import left code without a value map: the next update rebuilds
        self.update_fast = None           # what stat "update_fast" reads (None: no update has set it yet)
        self.mode, self.flips = None, 0   # the conv_mode a flip left (None: the plan's own), flips so far

    # ---- facts ---------------------------------------------------------------------------------------------------------
    @property
    def dtype(self):
        return self.values.dtype

    @property
    def f64(self):
        return self.values.dtype == np.float64

    @property
    def nnz(self):
        return int(self.pos.size)

    @property
    def dense_size(self):
        return rc.dense_size(self.desc)

    @property
    def w_shape(self):
        d = self.desc
        return (d.M, d.C // d.group, d.KH, d.KW)

    def csr(self):
        """(rowptr, colidx, values, nnz_per_group) in get_csr()'s form."""
        rp, ci, ng = pc.pattern_csr(self.desc, self.pos)
        return rp, ci, self.values.copy(), ng

    def dense(self):
        """blobs_[0]: the values at the pattern, +0 elsewhere."""
        return pc.masked_dense(self.desc, *self.csr())

    def mask(self):
        m = np.zeros(self.dense_size, bool)
        m[self.pos] = True
        return m.reshape(self.w_shape)

    def row_scale(self, row_exp, dt):
        """2^row_exp of every output channel, shaped to multiply blobs_[0]: its rows are axis 0."""
        return np.ldexp(1.0, row_exp).astype(dt)[:, None, None, None]

    def wgrad_terms(self, n, td_shape):
        """The terms of one weight-gradient element over n images (what errbound.accumulated_bound counts): the top's
        positions."""
        return n * td_shape[2] * td_shape[3]

    # ---- values --------------------------------------------------------------------------------------------------------
    def _updated(self):
        """One update's bookkeeping: the counter, and the update_fast the library will report for it."""
        self.stats["update_count"] += 1
        self.update_fast = 1 if self.in_place and not self.no_value_map else 0
        self.no_value_map = False         # the rebuild produces the map

    def set_values(self, v):
        v = np.ascontiguousarray(v)
        assert v.dtype == self.dtype and v.shape == self.values.shape
        self.values = v.copy()
        self._updated()

    def update_from_dense(self, w):
        """Reads the blob at the pattern's positions only."""
        w = np.ascontiguousarray(w)
        assert w.dtype == self.dtype and w.size == self.dense_size
        self.values = w.reshape(-1)[self.pos].copy()
        self._updated()

    def solver_step(self, grad, **hyper):
        """solver_common.step on the values and the histories (zeros before the first step); grad: nnz elements."""
        grad = np.ascontiguousarray(grad)
        assert grad.dtype == self.dtype and grad.shape == self.values.shape
        if self.h is None:
            self.h = np.zeros(self.nnz, self.dtype)
        if hyper["type"] == sc.ADAM and self.h2 is None:
            self.h2 = np.zeros(self.nnz, self.dtype)
        w, h, h2 = sc.step(self.values, grad, self.h, self.h2 if hyper["type"] == sc.ADAM else None, **hyper)
        self.values, self.h = w, h
        if h2 is not None:
            self.h2 = h2
        self.stats["update_count"] += 1
        if self.nnz > 0:                  # (an empty plan's step launches nothing and leaves update_fast as it was)
            self.update_fast = 1 if self.in_place and not self.no_value_map else 0
            self.no_value_map = False

    # ---- pattern -------------------------------------------------------------------------------------------------------
    def _realigned(self, changed):
        if changed:
            self.no_value_map = False     # a re-align generates code with its value map

    def prune(self, keep=None, threshold=None, score=None):
        """Returns the entry map (int32, old nnz elements).  The histories are NOT carried: compact_histories does that."""
        s = self.values if score is None else np.ascontiguousarray(score, self.dtype)
        m = pc.ref_map(s, keep=keep, threshold=None if threshold is None else self.dtype.type(threshold))
        kept = m >= 0
        self.stats["prune_count"] += 1
        self.stats["prune_last_dropped"] = int((~kept).sum())
        self._realigned(not kept.all())
        self.pos, self.values = self.pos[kept], self.values[kept]
        return m

    def rewire(self, grow, score, init=None, drop_keep=None, drop_threshold=None, drop_score=None):
        """Returns (entry_map, grown), both int32."""
        want = rc.ref_rewire(self.desc, self.csr(), grow, score, init=init, drop_keep=drop_keep, drop_threshold=drop_threshold,
                             drop_score=drop_score)
        m, grown = want["entry_map"], want["grown"]
        self.stats["rewire_count"] += 1
        self.stats["rewire_last_dropped"] = int((m < 0).sum())
        self.stats["rewire_last_grown"] = int(grown.size)
        self._realigned(bool((m < 0).any()) or grown.size > 0)
        self.pos, self.values = want["pos"], want["csr"][2]
        return m, grown

    def compact(self, entry_map, arr):
        """What escoin_compact_entries into zeros of the NEW nnz gives (call after the prune / rewire)."""
        return rc.reindex(np.asarray(entry_map), self.nnz, np.asarray(arr))

    def compact_histories(self, entry_map):
        if self.h is not None:
            self.h = self.compact(entry_map, self.h)
        if self.h2 is not None:
            self.h2 = self.compact(entry_map, self.h2)

    # ---- plan-level events ------------------------------------------------------------------------------------------------
    def imported(self, fast, fresh_plan):
        """An export_aligned -> import_aligned round trip: the values and pattern stay.  fast: stat import_fast; fresh_plan:
        the import went into a new plan that replaces the old one (its counters start again)."""
        self.no_value_map = bool(fast)
        if fresh_plan:
            self.stats = dict.fromkeys(COUNTERS, 0)
            self.update_fast = None

    def flipped(self, mode):
        """A conv_mode flip to "LOWERED_SPARSE" / "LOWERED_GEMM" or (None) back to the plan's own mode.  To or from
        LOWERED_GEMM the library rebuilds the device side from the host CSR, which generates code with its value map."""
        self._realigned((mode == "LOWERED_GEMM") != (self.mode == "LOWERED_GEMM"))
        self.mode = mode
        self.flips += 1

    # ---- bounds ------------------------------------------------------------------------------------------------------------
    def forward_bound(self, x, b, relu=None):
        return eb.forward_bound(self.desc, self.dense(), x, b, relu=self.relu if relu is None else relu, f64=self.f64)

    def backward_bound(self, x, b, top_diff, top=None):
        """((bottom_diff, weight_diff, bias_diff), (their bounds)); the weight gradient at the pattern, explicit zeros included."""
        return eb.backward_bound(self.desc, self.dense(), x, b, top_diff, top, f64=self.f64, mask=self.mask())

    def dense_wgrad_bound(self, x, top_diff, top=None):
        """(weight gradient at EVERY position, its bound)."""
        want, Bs = eb.backward_bound(self.desc, self.dense(), x, None, top_diff, top, f64=self.f64, mask=np.ones(self.w_shape, bool))
        return want[1], Bs[1]


# ---- option "deconv" ------------------------------------------------------------------------------------------------------
# The geometry of a Deconvolution layer's blobs_[0] and CSR is its mirror convolution's: C rows of Mg * KH * KW columns per
# group.  With these five fields the pattern restatements above (prune_common, rewire_common) apply as they stand.
Mirror = namedtuple("Mirror", "M C group KH KW")


class DeconvModel(PlanModel):
    """A plan of option "deconv": `s` is a d2s_common.DShape; pos are flat positions of the C x Mg x KH x KW blob, so csr()
    is d2s_common.csr_of's form; the bounds are errbound's on the inner stride-1 layer, through d2s_common."""

    def __init__(self, s, synth, pos, values, relu=False, in_place=True):
        self.s, self.synth = s, synth
        PlanModel.__init__(self, Mirror(s.C, s.M, s.group, s.KH, s.KW), pos, values, relu, in_place)

    def row_scale(self, row_exp, dt):
        """Output channel m = g * Mg + ml is column ml of the rows of group g."""
        s = self.s
        e = np.asarray(row_exp).reshape(s.group, 1, s.M // s.group)
        e = np.broadcast_to(e, (s.group, s.C // s.group, s.M // s.group)).reshape(s.C, s.M // s.group)
        return np.ldexp(1.0, e).astype(dt)[:, :, None, None]

    def wgrad_terms(self, n, td_shape):
        """The inner layer's top positions: an entry's gradient is summed over G' = pack(top_diff)."""
        _, _, _, hi, wi = dc.inner_dims(self.s)
        return n * hi * wi

    def forward_bound(self, x, b, relu=None):
        return dc.forward_bound(eb, self.synth, self.s, self.dense(), x, b, self.relu if relu is None else relu)

    def backward_bound(self, x, b, top_diff, top=None):
        return dc.backward_bound(eb, self.synth, self.s, self.dense(), x, top_diff, top, mask=self.mask())

    def dense_wgrad_bound(self, x, top_diff, top=None):
        raise NotImplementedError("escoin_dense_wgrad refuses a deconv plan: the op is not in its vocabulary")
