"""Plan option "deconv" in the op-sequence suite: what test_d2s_sequence_cpu.py and test_d2s_sequence_gpu.py share.  The
driver, its checks and the generator are seq_common's, unchanged; the model is plan_model.DeconvModel; the backends are
seq_backends' with the one point overridden at which the descriptor and the plan are made.  seq_common's tables name
convolution layers only, so the layers, the configurations, their seeds and their inputs are made here, the inputs the way
seq_common.make_inputs makes its own."""
import numpy as np

import d2s_common as dc
import errbound as eb
import rewire_common as rc
import seq_common as sq
from plan_model import DeconvModel, positions
from seq_backends import CpuBackend, GpuBackend

# ---- the layers: the smallest at which the pieces differ ---------------------------------------------------------------------
LAYERS = {
    # d2s_common's k4s2p1 (the common decoder layer, crop on both sides) on the sequence suite's channel counts (L3X3: 24 and
    # 20): the inner layer is 24 -> 80 channels, 2 x 2, pad 1, 5 x 7 -> 6 x 8, which forced KERNEL_JIT / KERNEL_TILED take
    # (test_the_forced_inner_kernels_exist).  N = 3: n_part = 1 is a partial batch with two images behind it.
    "DK4": dc.DShape("seq_k4s2p1", 3, 24, 5, 7, 20, 4, 4, 2, 2, 1, 1, 1),
    # groups, K not a multiple of the stride (phases with 2 x 2, 2 x 1, 1 x 2 and 1 x 1 taps), P = 9
    "DK5G2": dc.make("k5s3p2_g2"),
}
DENSITY = {"DK4": 0.1, "DK5G2": 0.4}

# ---- the vocabulary -----------------------------------------------------------------------------------------------------------
# The library refuses these three on a deconv plan by name (test_d2s_gpu.test_refusals_on_the_device asserts it): removed
# up front, as every exclusion of the suite.
_REFUSED = "refuses a plan of option deconv by name: the pattern ops and the dense gradient are defined on M x C/g x KH x KW"
EXCLUDE = {"prune": "escoin_plan_prune " + _REFUSED, "rewire": "escoin_plan_rewire " + _REFUSED,
           "dense_wgrad": "escoin_dense_wgrad " + _REFUSED}
CPU_EXCLUDE = dict(EXCLUDE, **sq._CPU_EXCLUDE)

_UNPACK = ("escoin_d2s_unpack_kernel",)
CONFIGS = [
    sq.Config("deconv_auto", "DK4", dict(deconv=1), False, False, "pruned", dict(name=_UNPACK, deconv=1), EXCLUDE),
    # the ReLU mask goes through the pack kernel, generated code inside
    sq.Config("deconv_jit", "DK4", dict(deconv=1, kernel="KERNEL_JIT", backward_kernel="KERNEL_JIT", tiling_batch=256), True, False,
              "pruned", dict(name=_UNPACK, inner=("jit",), deconv=1, kernel_choice="KERNEL_JIT", bwd_data_kernel="KERNEL_JIT"), EXCLUDE),
    sq.Config("deconv_dense", "DK4", dict(deconv=1, kernel="KERNEL_DENSE", wgrad_kernel="WGRAD_MFMA"), False, False, "pruned",
              dict(name=_UNPACK, inner=("dense",), deconv=1, kernel_choice="KERNEL_DENSE", wgrad_kernel="WGRAD_MFMA"), EXCLUDE),
    sq.Config("deconv_generic", "DK4", dict(deconv=1, kernel="KERNEL_GENERIC", backward_kernel="KERNEL_GENERIC", wgrad_kernel="WGRAD_ENTRY"),
              False, False, "pruned", dict(name=_UNPACK, inner=("generic",), deconv=1, kernel_choice="KERNEL_GENERIC",
                                           bwd_data_kernel="KERNEL_GENERIC", wgrad_kernel="WGRAD_ENTRY"), EXCLUDE),
    sq.Config("deconv_g2_auto", "DK5G2", dict(deconv=1), True, False, "pruned", dict(name=_UNPACK, deconv=1), EXCLUDE),
    sq.Config("deconv_g2_generic", "DK5G2", dict(deconv=1, kernel="KERNEL_GENERIC", backward_kernel="KERNEL_GENERIC", wgrad_kernel="WGRAD_ENTRY"),
              False, False, "pruned", dict(name=_UNPACK, inner=("generic",), deconv=1, kernel_choice="KERNEL_GENERIC",
                                           bwd_data_kernel="KERNEL_GENERIC", wgrad_kernel="WGRAD_ENTRY"), EXCLUDE),
]
CPU_CONFIGS = [
    sq.Config("cpu_deconv_k4", "DK4", dict(deconv=1), True, False, "pruned", {}, CPU_EXCLUDE),
    sq.Config("cpu_deconv_g2", "DK5G2", dict(deconv=1), False, False, "pruned", {}, CPU_EXCLUDE),
]
BY_ID = {c.id: c for c in CONFIGS + CPU_CONFIGS}


def first_seeds(cfg, count=3, limit=200):
    """seq_common.SEEDS' rule: the first `count` consecutive seeds, counted from 1, over which every op of the
    configuration's vocabulary occurs at least twice."""
    for first in range(1, limit):
        seeds = tuple(range(first, first + count))
        counts, _ = sq.coverage([cfg], {cfg.id: seeds})
        if min(counts[cfg.id].values()) >= 2:
            return seeds
    raise AssertionError("no seeds under %d cover %s" % (limit, cfg.id))


# written out, so that a sequence's name says what ran; test_d2s_sequence_cpu.test_the_seeds_are_the_first_that_cover holds
# them to the rule
SEEDS = {
    "deconv_auto": (1, 2, 3), "deconv_jit": (4, 5, 6), "deconv_dense": (1, 2, 3), "deconv_generic": (1, 2, 3),
    "deconv_g2_auto": (2, 3, 4), "deconv_g2_generic": (1, 2, 3), "cpu_deconv_k4": (1, 2, 3), "cpu_deconv_g2": (1, 2, 3),
}


# ---- the inputs ---------------------------------------------------------------------------------------------------------------
def to_rows(s, w):
    """C x Mg x KH x KW -> M x Cg x KH x KW (the mirror convolution's blob: a row per output channel)."""
    cg, mg = s.C // s.group, s.M // s.group
    return np.ascontiguousarray(w.reshape(s.group, cg, mg, s.KH, s.KW).transpose(0, 2, 1, 3, 4).reshape(s.M, cg, s.KH, s.KW))


def from_rows(s, wm):
    cg, mg = s.C // s.group, s.M // s.group
    return np.ascontiguousarray(wm.reshape(s.group, mg, cg, s.KH, s.KW).transpose(0, 2, 1, 3, 4).reshape(s.C, mg, s.KH, s.KW))


_INPUTS = {}


def make_inputs(cfg):
    """As seq_common.make_inputs: skewed weights, bottom, bias and top_diff for the checked calls, a plain bottom and
    top_diff for the gradients that feed the solver.  errbound.skew scales a weight ROW per output channel, so it is given
    the blob with output channels as rows; the exponent of channel m is thereby shared by m's P inner rows."""
    if cfg.id not in _INPUTS:
        s = LAYERS[cfg.layer]
        k = sum(map(ord, cfg.id))
        w = dc.weights(s, k, DENSITY[cfg.layer])
        rs = np.random.RandomState(k + 1)
        x = rs.uniform(-1, 1, (s.N, s.C, s.H, s.W)).astype(np.float32)
        b = rs.uniform(-0.5, 0.5, s.M).astype(np.float32)
        td = rs.uniform(-1, 1, (s.N, s.M) + dc.out_hw(s)).astype(np.float32)
        sk = eb.skew(s, to_rows(s, w), x, b, k + 4, top_diff=td)
        c = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
        px = rs.uniform(-1, 1, x.shape).astype(np.float32)
        ptd = (rs.uniform(-1, 1, td.shape) / 16).astype(np.float32)
        _INPUTS[cfg.id] = sq.Inputs(s, np.float32, from_rows(s, c(sk.w)), c(sk.x), c(sk.b), c(sk.top_diff), px, ptd, sk.row_exp)
    return _INPUTS[cfg.id]


def initial_model(synth, cfg, inp):
    w = inp.w0.reshape(-1)
    pos = np.flatnonzero(w != 0)
    return DeconvModel(inp.s, synth, pos, w[pos], relu=cfg.relu)


# ---- the backends ------------------------------------------------------------------------------------------------------------
class DeconvGpuBackend(GpuBackend):
    def _describe(self):
        return dc.desc(self.pkg, self.inp.s, True, self.cfg.relu)

    # (_new_plan: the configuration's options carry deconv=1)


class DeconvCpuBackend(CpuBackend):
    """The _cpu twins of a deconv plan.  The blob is C x Mg x KH x KW and the CSR's rows are the bottom's channels, so what the
    base class reads off the layer as a convolution's -- the blob's shape and the entries' positions -- is read off the mirror
    geometry here."""

    def __init__(self, pkg, cfg, inp, csr):
        self.pkg, self.cfg, self.inp, self.dt = pkg, cfg, inp, inp.dt
        self.mirror = DeconvModel(inp.s, None, np.zeros(0, np.int64), np.zeros(0, np.float32)).desc
        self.desc, self.plan = self._make()
        self.h = self.h2 = None
        rp, ci, va, ng = csr
        pos = positions(self.mirror, rp, ci, ng)
        w = np.zeros(rc.dense_size(self.mirror), self.dt)      # aligned on ones, then updated: explicit zeros stay entries
        w[pos] = 1
        self.plan.weight_align_cpu(w.reshape(self._w_shape()))
        w[pos] = va
        self.plan.update_values_cpu(w.reshape(self._w_shape()))
        self.update_count0 = 1
        assert self.plan.nnz() == pos.size

    def _make(self):
        desc = dc.desc(self.pkg, self.inp.s, True, self.cfg.relu)
        return desc, self.pkg.Plan(desc, deconv=1)

    def _w_shape(self):
        s = self.inp.s
        return (s.C, s.M // s.group, s.KH, s.KW)

    def set_values(self, v, source):
        rp, ci, _, ng = self.plan.get_csr()
        w = np.full(rc.dense_size(self.mirror), np.nan, self.dt)
        w[positions(self.mirror, rp, ci, ng)] = v
        self.plan.update_values_cpu(w.reshape(self._w_shape()))
