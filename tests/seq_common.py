"""Sequences of plan operations against plan_model.PlanModel: the op vocabulary, the configurations, the seeded generator
and the driver of test_sequence_cpu.py and test_sequence_gpu.py.  Imports nothing from the library; a *backend* (one for the
device entry points, one for the _cpu twins) wraps a Plan behind one method per op, numpy in and numpy out.

After every op the driver makes the check that op allows, always against the model; see Driver.  Reading the host side
(get_csr, export_aligned) changes a plan's state -- it ends a device-authoritative state -- so those are ops of the
vocabulary, drawn like any other, and the driver never calls them as a routine check: the routine check after a mutating op
is a forward."""
from collections import namedtuple

import numpy as np

import errbound as eb
import prune_common as pc
import rewire_common as rc
import solver_common as sc
from plan_model import COUNTERS, PlanModel, positions, same_bits  # noqa: F401
from upd_common import new_weights

# ---- the vocabulary ----------------------------------------------------------------------------------------------------------
OPS = ("forward", "backward", "dense_wgrad", "set_values", "update_values", "solver_step", "prune", "rewire", "get_csr",
       "import_same", "import_fresh", "flip")
# the class of an op in the ordered-pair coverage (ops that change the plan's values, pattern or device structures)
MUTATING = {"set_values": "set_values", "update_values": "update_values", "solver_step": "solver_step", "prune": "prune",
            "rewire": "rewire", "import_same": "import", "import_fresh": "import", "flip": "flip"}
MUTATING_CLASSES = ("set_values", "update_values", "solver_step", "prune", "rewire", "import", "flip")
# how often an op is drawn, relative to the others
WEIGHTS = {"forward": 1, "backward": 3, "dense_wgrad": 1, "set_values": 2, "update_values": 2, "solver_step": 3, "prune": 2,
           "rewire": 2, "get_csr": 2, "import_same": 1, "import_fresh": 1, "flip": 2}

# ---- the layers: the smallest shapes at which the named kernels still run (test_errbound_gpu.py proves it for each) -----------
# name: (synth name, (N, C, H, W, M, K), kwargs of synth.shape)
LAYERS = {
    "L3X3": ("eb3x3", (5, 24, 9, 11, 20, 3), dict(pad=1, sparsity=0.9)),
    "PW_B": ("ebpw_b", (4, 60, 5, 5, 150, 1), dict(sparsity=0.95)),
    "G5X5": ("ebg5x5", (2, 16, 12, 10, 12, 5), dict(pad=2, group=2, sparsity=0.8)),
    "STR2": ("ebs2", (3, 8, 31, 31, 8, 3), dict(pad=1, stride=2, sparsity=0.6)),
    # The dilated layer of option "s2b".  Dilation 2 x 3: the smallest pair with dil_h != dil_w, both above 1 (P = 6 residue
    # classes).  13 x 16 with pad 2 x 3 is a padded frame of 17 x 22: neither a multiple of its dilation, so the row classes
    # hold 9 and 8 rows and the column classes 8, 7 and 7 (short classes on both axes); pad <= dil * (K - 1) on both axes
    # (4 and 6), so the outer transposed plan exists.  The inner layer is 18 images of 24 x 9 x 8, pad 0, with a 7 x 6 top, on
    # L3X3's channel counts; forced KERNEL_TILED and KERNEL_JIT take it, and its transposed layer, as it is (align_rules'
    # host rules say so, test_errbound_gpu.py runs both), so nothing had to grow beyond what the
    # residue classes need (17 = 2 * 8 + 1, 22 = 3 * 7 + 1: one long class per axis, the others short).  N = 3: n_part = N // 2
    # = 1 is a partial batch, of 6 inner images, with two images past it that must stay untouched.
    "DIL": ("ebdil", (3, 24, 13, 16, 20, 3), dict(pad=2, pad_w=3, dil=2, dil_w=3, sparsity=0.9)),
}

# ---- the configurations ---------------------------------------------------------------------------------------------------------
# options: Plan options; a string names a constant of the package.  expect: what must hold once a forward and a backward
# have run: name = substrings of kernel_name (any of them), the others are stats.  exclude: op -> the reason.
Config = namedtuple("Config", "id layer options relu f64 weights expect exclude")
_NO_F64_WGRAD = "escoin_dense_wgrad runs on the fp32 matrix cores: a double plan refuses it"
_NO_F64_FORM = "the aligned form is defined for float plans: export_aligned refuses a double plan"
_NO_CPU_TWIN = "no _cpu twin: the aligned form and conv_mode belong to the device side"
_CPU_EXCLUDE = {"import_same": _NO_CPU_TWIN, "import_fresh": _NO_CPU_TWIN, "flip": _NO_CPU_TWIN}

CONFIGS = [
    Config("jit_3x3", "L3X3", dict(kernel="KERNEL_JIT", tiling_batch=256, backward_kernel="KERNEL_JIT"), True, False, "pruned",
           dict(name=("jit",), bwd_data_kernel="KERNEL_JIT"), {}),
    Config("tiled_3x3", "L3X3", dict(kernel="KERNEL_TILED", backward_kernel="KERNEL_DENSE", wgrad_kernel="WGRAD_STAGED"), False, False,
           "pruned", dict(name=("tiled",), bwd_data_kernel="KERNEL_DENSE", wgrad_kernel="WGRAD_STAGED"), {}),
    Config("generic_3x3", "L3X3", dict(kernel="KERNEL_GENERIC", backward_kernel="KERNEL_GENERIC", wgrad_kernel="WGRAD_ENTRY"), False, False,
           "pruned", dict(name=("generic",), bwd_data_kernel="KERNEL_GENERIC", wgrad_kernel="WGRAD_ENTRY"), {}),
    Config("dense_mfma", "L3X3", dict(kernel="KERNEL_DENSE", backward_kernel="BWD_MFMA", wgrad_kernel="WGRAD_MFMA"), False, False,
           "pruned", dict(name=("escoin_dense_mfma_kernel",), bwd_data_kernel="BWD_MFMA", wgrad_kernel="WGRAD_MFMA"), {}),
    Config("mixed_groups", "G5X5", dict(dense_threshold_pct=30, tiling_batch=256), False, False, "mixed", dict(name=(" + ",)), {}),
    Config("pointwise", "PW_B", dict(kernel="KERNEL_JIT", tiling_batch=256), False, False, "pruned", dict(name=("jit",)), {}),
    Config("jit_loader", "L3X3", dict(kernel="KERNEL_JIT", tiling_batch=256, code_loader=1), False, False, "pruned",
           dict(name=("jit",), code_direct=0), {}),      # code the HIP module loader placed: every update rebuilds (update_fast 0)
    Config("s2d_inner", "STR2", dict(s2d=1), False, False, "pruned", dict(s2d=1), {}),
    Config("s2d_outer_mfma", "STR2", dict(s2d=1, backward_kernel="BWD_MFMA"), False, False, "pruned",
           dict(s2d=1, bwd_data_kernel="BWD_MFMA"), {}),
    Config("s2d_outer_generic", "STR2", dict(s2d=1, backward_kernel="KERNEL_GENERIC", wgrad_kernel="WGRAD_ENTRY"), False, False, "pruned",
           dict(s2d=1, bwd_data_kernel="KERNEL_GENERIC", wgrad_kernel="WGRAD_ENTRY"), {}),
    # option "s2b": the weights also live in every copy of the inner plan of N * P images, which a prune, rewire, set_csr or
    # conv_mode flip tears down and rebuilds.  Float plans: every op of the vocabulary applies
    Config("s2b_inner", "DIL", dict(s2b=1), False, False, "pruned", dict(s2b=1), {}),
    Config("s2b_inner_jit", "DIL", dict(s2b=1, kernel="KERNEL_JIT", backward_kernel="KERNEL_JIT", tiling_batch=256), True, False, "pruned",
           dict(s2b=1, name=("jit",), bwd_data_kernel="KERNEL_JIT"), {}),      # the ReLU mask through the pack kernel, generated code inside
    Config("s2b_outer_mfma", "DIL", dict(s2b=1, backward_kernel="BWD_MFMA"), False, False, "pruned",
           dict(s2b=1, bwd_data_kernel="BWD_MFMA"), {}),
    Config("s2b_outer_generic", "DIL", dict(s2b=1, backward_kernel="KERNEL_GENERIC", wgrad_kernel="WGRAD_ENTRY"), False, False, "pruned",
           dict(s2b=1, bwd_data_kernel="KERNEL_GENERIC", wgrad_kernel="WGRAD_ENTRY"), {}),
    Config("double", "L3X3", dict(wgrad_kernel="WGRAD_ENTRY"), False, True, "pruned",
           dict(name=("f64",), bwd_data_kernel="KERNEL_GENERIC", wgrad_kernel="WGRAD_ENTRY"),
           {"dense_wgrad": _NO_F64_WGRAD, "import_same": _NO_F64_FORM, "import_fresh": _NO_F64_FORM}),
]
# the CPU twins: float and double plans; dense_wgrad_cpu serves both dtypes
CPU_CONFIGS = [
    Config("cpu_3x3_f32", "L3X3", {}, True, False, "pruned", {}, _CPU_EXCLUDE),
    Config("cpu_groups_f64", "G5X5", {}, False, True, "mixed", {}, _CPU_EXCLUDE),
    Config("cpu_stride2_f32", "STR2", {}, False, False, "pruned", {}, _CPU_EXCLUDE),
    Config("cpu_dilated_f32", "DIL", {}, False, False, "pruned", {}, _CPU_EXCLUDE),
]
BY_ID = {c.id: c for c in CONFIGS + CPU_CONFIGS}

# Seeds and length: chosen so that test_generator_coverage holds (every op of a configuration's vocabulary at least twice
# over its seeds; every ordered pair of distinct mutating classes adjacent somewhere in the device suite).  The "s2b" and
# cpu_dilated_f32 rows: the first three consecutive seeds, counted from 1, that coverage() accepts for the configuration.
LENGTH = 20
SEEDS = {
    "jit_3x3": (6, 7, 8), "tiled_3x3": (2, 3, 4), "generic_3x3": (13, 14, 15), "dense_mfma": (4, 5, 6), "mixed_groups": (1, 2, 3),
    "pointwise": (9, 10, 11), "jit_loader": (3, 4, 5), "s2d_inner": (6, 7, 8), "s2d_outer_mfma": (12, 13, 14),
    "s2d_outer_generic": (5, 6, 7), "double": (1, 2, 3),
    "s2b_inner": (5, 6, 7), "s2b_inner_jit": (11, 12, 13), "s2b_outer_mfma": (1, 2, 3), "s2b_outer_generic": (5, 6, 7),
    "cpu_3x3_f32": (1, 2, 3), "cpu_groups_f64": (2, 3, 4), "cpu_stride2_f32": (1, 2, 3), "cpu_dilated_f32": (2, 3, 4),
}


def vocabulary(cfg):
    """The ops a configuration draws from: OPS without its exclusions (removed up front, never skipped at run time)."""
    return tuple(op for op in OPS if op not in cfg.exclude)


def vocabulary_table():
    """The table profiles/sequence_fuzz.md shows: (configuration, op, reason) for every exclusion."""
    return [(c.id, op, why) for c in CONFIGS + CPU_CONFIGS for op, why in sorted(c.exclude.items())]


# ---- the generator -----------------------------------------------------------------------------------------------------------
def _params(op, rs, vocab):
    """The parameters of one op: fractions and switches only, so that an op list does not depend on the plan's state and can
    be pasted as a directed test.  The driver resolves them against the model (keep = a fraction of the current nnz ...)."""
    flag = lambda: bool(rs.randint(0, 2))  # noqa: E731
    seed = lambda: int(rs.randint(1, 1 << 20))  # noqa: E731
    if op == "forward":
        return dict(bias=flag(), partial=flag())
    if op == "backward":
        return dict(bias=flag(), compact=flag(), partial=flag(), accumulate=flag(), data=bool(rs.randint(0, 4)), seed=seed())
    if op in ("set_values", "update_values"):
        return dict(source=("host", "device")[rs.randint(0, 2)], seed=seed())
    if op == "solver_step":
        return dict(partial=flag())
    if op == "prune":
        return dict(mode=("keep", "threshold", "score")[rs.randint(0, 3)], frac=round(float(rs.uniform(0.6, 0.95)), 2), seed=seed())
    if op == "rewire":
        scores = ("ties", "dense_wgrad") if "dense_wgrad" in vocab else ("ties",)
        return dict(drop=(None, "keep", "threshold", "score")[rs.randint(0, 4)], drop_frac=round(float(rs.uniform(0.7, 0.95)), 2),
                    grow_frac=round(float(rs.uniform(0.05, 0.3)), 2), init=flag(), score=scores[rs.randint(0, len(scores))], seed=seed())
    if op == "flip":
        return dict(mode=("sparse", "gemm", "both")[rs.randint(0, 3)])
    return {}


def generate(cfg, seed, length=LENGTH):
    """(hyper, ops): the solver rule of the sequence and `length` ops drawn from the configuration's vocabulary."""
    vocab = vocabulary(cfg)
    rs = np.random.RandomState(seed * 7919 + sum(map(ord, cfg.id)))
    rule = ("sgd", "nesterov", "adam")[rs.randint(0, 3)]
    reg = ("none", "L2", "L1")[rs.randint(0, 3)]
    hyper = dict(type=sc.RULES[rule], regularization=sc.REGS[reg], rate=1e-2 if rule != "adam" else 1e-3, momentum=0.9,
                 momentum2=0.999, delta=1e-8, decay=0.0 if reg == "none" else 1e-3, diff_scale=(1.0, 0.5)[rs.randint(0, 2)])
    p = np.array([WEIGHTS[op] for op in vocab], np.float64)
    names = [vocab[i] for i in rs.choice(len(vocab), size=length, p=p / p.sum())]
    return hyper, [(op, _params(op, rs, vocab)) for op in names]


def coverage(configs, seeds=SEEDS, length=LENGTH):
    """(per configuration: op -> count over its seeds, the set of adjacent ordered pairs of distinct mutating classes over all
    the configurations, forwards / backwards / reads in between ignored)."""
    counts, pairs = {}, set()
    for cfg in configs:
        c = dict.fromkeys(vocabulary(cfg), 0)
        for seed in seeds[cfg.id]:
            last = None
            for op, _ in generate(cfg, seed, length)[1]:
                c[op] += 1
                k = MUTATING.get(op)
                if k is not None:
                    if last is not None and last != k:
                        pairs.add((last, k))
                    last = k
        counts[cfg.id] = c
    return counts, pairs


# ---- the inputs of a configuration --------------------------------------------------------------------------------------------
Inputs = namedtuple("Inputs", "s dt w0 x b td px ptd row_exp")


def mixed_weights(s, seed):
    """A grouped layer whose first conv group is 60 % dense and whose others keep 8 % (the "mixed_groups" plan kind of the
    update, prune and solver tests as well)."""
    rs = np.random.RandomState(seed)
    w = rs.uniform(-1, 1, (s.M, s.C // s.group, s.KH, s.KW)).astype(np.float32)
    w[w == 0] = 0.5
    mg = s.M // s.group
    keep = rs.uniform(0, 1, w.shape)
    w[:mg][keep[:mg] >= 0.6] = 0
    w[mg:][keep[mg:] >= 0.08] = 0
    return w


_INPUTS = {}


def make_inputs(synth, cfg):
    """The layer and its inputs, made once per configuration and never written: skewed weights, bottom, bias and top_diff
    (errbound.skew, as in test_errbound_gpu.py) for the checked forwards and backwards; a plain bottom and top_diff of
    order 1 for the gradients that feed the solver and rewire's grow score."""
    if cfg.id not in _INPUTS:
        name, dims, kw = LAYERS[cfg.layer]
        s = synth.shape(name, *dims, **kw)
        k = sum(map(ord, cfg.id))
        w = mixed_weights(s, k) if cfg.weights == "mixed" else synth.pruned_weights(s, k)
        x, b = synth.activations(s, k + 1), synth.bias_vector(s, k + 2)
        td = np.random.RandomState(k + 3).uniform(-1, 1, (s.N, s.M) + synth.out_hw(s)).astype(np.float32)
        sk = eb.skew(s, w, x, b, k + 4, top_diff=td)
        dt = np.float64 if cfg.f64 else np.float32
        c = lambda a: None if a is None else np.ascontiguousarray(a, dt)  # noqa: E731
        px = synth.activations(s, k + 5)
        ptd = (np.random.RandomState(k + 6).uniform(-1, 1, td.shape) / 16).astype(np.float32)
        inp = Inputs(s, dt, c(sk.w), c(sk.x), c(sk.b), c(sk.top_diff), c(px), c(ptd), sk.row_exp)
        _INPUTS[cfg.id] = inp
    return _INPUTS[cfg.id]


def initial_model(cfg, inp):
    w = inp.w0.reshape(-1)
    pos = np.flatnonzero(w != 0)
    return PlanModel(inp.s, pos, w[pos], relu=cfg.relu, in_place=not cfg.options.get("code_loader"))


# ---- the driver ---------------------------------------------------------------------------------------------------------------
class SequenceError(AssertionError):
    """A failed sequence: `index` is the op at which the driver noticed (len(ops): the end-of-sequence comparison)."""

    def __init__(self, index, text, cause):
        AssertionError.__init__(self, "%s\n%s: %s" % (text, type(cause).__name__, cause))
        self.index, self.cause = index, cause


def describe(cfg, seed, hyper, ops, index):
    lines = ["sequence failed: configuration %s, seed %r, op %d of %d" % (cfg.id, seed, index, len(ops)),
             "  hyper = %r" % (hyper,), "  ops = ["]
    lines += ["    %s(%r, %r),%s" % ("", op, params, "        # <-- failed here" if i == index else "") for i, (op, params) in enumerate(ops)]
    lines.append("  ]" + ("        # <-- failed in the end-of-sequence comparison with a fresh plan" if index == len(ops) else ""))
    return "\n".join(lines)


def run_sequence(backend, cfg, inp, hyper, ops, seed=None, worst=None, model=None, finish=True):
    """Runs the ops on the backend and the model; raises SequenceError, after printing the configuration, the seed, the
    full op list and the failing index, at the first op whose check fails.  Returns the driver."""
    drv = Driver(backend, model or initial_model(cfg, inp), inp, hyper, worst)
    i = 0
    try:
        for i, (op, params) in enumerate(ops):
            getattr(drv, "op_" + op)(**params)
        if finish:
            i = len(ops)
            drv.finish()
    except SequenceError:
        raise
    except Exception as e:  # an EscoinError inside a sequence fails it like any assertion: nothing is skipped at run time
        text = describe(cfg, seed, hyper, ops, i)
        print(text)
        raise SequenceError(i, text, e)
    return drv


class Driver(object):
    """One backend and one model through a list of ops.  The backend (see test_sequence_cpu.CpuBackend) holds the plan and the
    solver histories; every array crosses as numpy.  What is checked, always against the model:
      forward, backward, dense_wgrad   every element within errbound's float64 bound (eb.within)
      prune, rewire                    the entry map, the grown list, nnz, the stats and the compacted histories: exact
      solver_step                      the gradient within its bound FIRST, then those bits go to the model; the histories
                                       read back: exact bits
      set_values, update_values        stat update_fast as the model predicts (backends that report it)
      get_csr, import                  exact bits
    and after every mutating op a forward (never a host read).  What depends on the layout of blobs_[0] -- which axis a row
    exponent scales, how many terms a weight-gradient sum has -- the driver asks the model (plan_model.DeconvModel answers
    for a C x Mg x KH x KW blob)."""

    def __init__(self, backend, model, inp, hyper, worst=None):
        self.b, self.m, self.inp, self.hyper = backend, model, inp, hyper
        self.worst = {} if worst is None else worst
        self.n_part = max(1, inp.s.N // 2)

    # ---- helpers ---------------------------------------------------------------------------------------------------------
    def _within(self, got, want, B, kernel, what):
        return eb.within(got, want, B, kernel, what=what, worst=self.worst)

    def _forward(self, x, bias, n, what, prefill=False):
        """A checked forward of the first n images; with `prefill` into the head of a full, pre-filled top blob."""
        b = self.inp.b if bias else None
        want, B = self.m.forward_bound(x[:n], b)
        if prefill:
            top = self.b.forward(x[:n], b, prefill=-7.5, full=x.shape[0])
            assert top.shape[0] == x.shape[0] and np.all(top[n:] == -7.5), (what, "images past the call's were written")
            top = top[:n]
        else:
            top = self.b.forward(x[:n], b)
        self._within(top, want, B, "forward " + self.b.label("forward"), what)
        return top

    def _routine(self, what):
        self._forward(self.inp.x, self.inp.b is not None, self.inp.s.N, (what, "the forward after it"))

    def _stats(self, what):
        for key in COUNTERS:
            if self.b.reports(key):
                assert self.b.stat(key) == self.m.stats[key], (what, key, self.b.stat(key), self.m.stats[key])
        assert self.b.nnz() == self.m.nnz, (what, "nnz", self.b.nnz(), self.m.nnz)

    def _update_fast(self, what):
        if self.b.reports("update_fast") and self.m.update_fast is not None:
            assert self.b.stat("update_fast") == self.m.update_fast, (what, "update_fast", self.b.stat("update_fast"), self.m.update_fast)

    def _histories(self, what):
        h, h2 = self.b.histories()
        for name, got, want in (("history", h, self.m.h), ("history2", h2, self.m.h2)):
            assert (got is None) == (want is None), (what, name)
            if want is not None:
                assert got.shape == want.shape and got.dtype == want.dtype, (what, name, got.shape, want.shape)
                bits = np.uint32 if want.dtype == np.float32 else np.uint64
                assert same_bits(got, want), (what, name, "differs at %d of %d entries" % (int((got.view(bits) != want.view(bits)).sum()), want.size))

    def _gradient(self, x, td, n, bias, what):
        """The compact weight gradient of the first n images, every element within its bound; returns its bits."""
        b = self.inp.b if bias else None
        top = self._forward(x, bias, n, (what, "forward")) if self.m.relu else None
        want, Bs = self.m.backward_bound(x[:n], b, td[:n], top)
        _, vd, _ = self.b.backward(td[:n], x[:n], top, data=False, wgrad="compact", bias=False)
        self._within(vd, want[1].reshape(-1)[self.m.pos], Bs[1].reshape(-1)[self.m.pos], "values_diff " + self.b.label("wgrad"), what)
        return vd

    def _dense_wgrad(self, what):
        inp = self.inp
        top = self._forward(inp.px, inp.b is not None, inp.s.N, (what, "forward")) if self.m.relu else None
        want, B = self.m.dense_wgrad_bound(inp.px, inp.ptd, top)
        got = self.b.dense_wgrad(inp.ptd, inp.px, top)
        self._within(got, want, B, "dense_wgrad " + self.b.label("dense_wgrad"), what)
        return got

    def _row_scale(self):
        return self.m.row_scale(self.inp.row_exp, self.inp.dt)

    # ---- the ops ---------------------------------------------------------------------------------------------------------
    def op_forward(self, bias, partial):
        bias = bias and self.inp.b is not None
        self._forward(self.inp.x, bias, self.n_part if partial else self.inp.s.N, ("forward", bias, partial), prefill=partial)

    def op_backward(self, bias, compact, partial, accumulate, data, seed):
        inp, m = self.inp, self.m
        bias = bias and inp.b is not None
        n = self.n_part if partial else inp.s.N
        what = ("backward", dict(bias=bias, compact=compact, partial=partial, accumulate=accumulate, data=data))
        b = inp.b if bias else None
        top = self._forward(inp.x, bias, n, (what, "forward")) if m.relu else None
        want, Bs = m.backward_bound(inp.x[:n], b, inp.td[:n], top)
        base = None
        if accumulate:      # the weight gradient accumulates into a pre-filled blob
            base = np.random.RandomState(seed).uniform(-1, 1, m.nnz if compact else m.dense_size).astype(inp.dt)
            base = base if compact else base.reshape(m.w_shape)
        bd, wd, bsd = self.b.backward(inp.td[:n], inp.x[:n], top, data=data, wgrad="compact" if compact else "dense", bias=bias, base=base)
        if data:
            self._within(bd, want[0], Bs[0], "bottom_diff " + self.b.label("dgrad"), what)
        wwant, wB = want[1], Bs[1]
        if compact:
            wwant, wB = wwant.reshape(-1)[m.pos], wB.reshape(-1)[m.pos]
        if accumulate:
            wB = eb.accumulated_bound(wB, base, m.wgrad_terms(n, inp.td.shape), f64=m.f64)
            wwant = wwant + base.astype(np.float64)
        if not compact:      # outside the pattern nothing is written: the blob keeps what it held
            outside = ~m.mask()
            keep = base[outside] if accumulate else np.zeros(int(outside.sum()), inp.dt)
            assert same_bits(wd[outside], keep), (what, "weight_diff was written outside the pattern")
            wd, wwant, wB = wd[~outside], wwant[~outside], wB[~outside]
        self._within(wd, wwant, wB, ("values_diff " if compact else "weight_diff ") + self.b.label("wgrad"), what)
        if bias:
            self._within(bsd, want[2], Bs[2], "bias_diff " + self.b.label("wgrad"), what)

    def op_dense_wgrad(self):
        self._dense_wgrad(("dense_wgrad",))

    def _new_dense(self, seed):
        """A blob of new values at the pattern (a few explicit zeros, one -0.0), rows scaled as the layer's, NaN outside."""
        w_new, w_nan = new_weights(self.m.dense(), seed, mask=self.m.mask())
        return w_new * self._row_scale(), w_nan * self._row_scale()

    def op_set_values(self, source, seed):
        w_new, _ = self._new_dense(seed)
        v = w_new.reshape(-1)[self.m.pos].copy()
        self.b.set_values(v, source)
        self.m.set_values(v)
        self._update_fast(("set_values", source))
        self._routine(("set_values", source))

    def op_update_values(self, source, seed):
        _, w_nan = self._new_dense(seed)
        self.b.update_values(w_nan, source)
        self.m.update_from_dense(w_nan)
        self._update_fast(("update_values", source))
        self._routine(("update_values", source))

    def op_solver_step(self, partial=False):
        inp = self.inp
        n = self.n_part if partial else inp.s.N
        g = self._gradient(inp.px, inp.ptd, n, inp.b is not None, ("solver_step", "gradient"))
        self.b.solver_step(g.copy(), self.hyper)
        self.m.solver_step(g, **self.hyper)
        self._update_fast(("solver_step",))
        self._histories(("solver_step",))
        self._routine(("solver_step",))

    def _ties(self, n, seed):
        """n scores of a few magnitudes and both signs: any boundary is a tie boundary."""
        return pc.score_cases(n, self.inp.dt, seed)["ties"]

    def _drop(self, mode, frac, seed):
        """(keep, threshold, score) of a drop by `mode` that keeps about `frac` of the entries (frac 0: none; otherwise one at
        least)."""
        m = self.m
        keep = max(1, int(round(frac * m.nnz))) if m.nnz and frac > 0 else 0
        if mode == "keep":
            return keep, None, None
        if mode == "threshold":
            mags = np.sort(np.abs(m.values))[::-1]
            return None, float(mags[min(keep, m.nnz) - 1]) if m.nnz else 0.5, None
        score = self._ties(m.nnz, seed)
        return pc.tie_boundary_keep(score, keep) if m.nnz > 1 else keep, None, score

    def op_prune(self, mode, frac, seed):
        keep, thr, score = self._drop(mode, frac, seed)
        what = ("prune", mode, keep, thr)
        got = self.b.prune(keep=keep, threshold=thr, score=score)
        want = self.m.prune(keep=keep, threshold=thr, score=score)
        differ = int((got != want).sum()) if got.shape == want.shape else -1
        assert got.dtype == np.int32 and np.array_equal(got, want), (what, "entry map differs at %d entries" % differ)
        self._stats(what)
        self.b.compact_histories(got)
        self.m.compact_histories(want)
        self._histories(what)
        self._routine(what)

    def op_rewire(self, drop, drop_frac, grow_frac, init, score, seed):
        m, inp = self.m, self.inp
        what = ("rewire", drop, drop_frac, grow_frac, init, score)
        if score == "dense_wgrad":      # the checked dense weight gradient's bits are the grow score (a RigL step)
            sc_arr = self._dense_wgrad((what, "score")).reshape(-1).copy()
        else:
            sc_arr = self._ties(m.dense_size, seed + 1)
        cand = rc.candidates(m.dense_size, m.pos)
        grow = int(round(grow_frac * max(m.nnz, 8)))
        if score == "ties" and cand.size > 1:
            grow = pc.tie_boundary_keep(sc_arr[cand], max(min(grow, cand.size - 1), 1))
        init_arr = None
        if init:
            init_arr = (np.random.RandomState(seed + 2).uniform(-1, 1, m.w_shape).astype(inp.dt) * self._row_scale()).reshape(-1)
            init_arr[::7] = -0.0
        kw = {}
        if drop is not None:
            keep, thr, dscore = self._drop(drop, drop_frac, seed + 3)
            kw = dict(drop_keep=keep, drop_threshold=thr, drop_score=dscore)
        got_map, got_grown = self.b.rewire(grow, sc_arr, init_arr, **kw)
        want_map, want_grown = m.rewire(grow, sc_arr, init=init_arr, **kw)
        for name, a, w in (("entry map", got_map, want_map), ("grown list", got_grown, want_grown)):
            assert a.dtype == np.int32 and np.array_equal(a, w), (what, "%s differs (sizes %d / %d)" % (name, a.size, w.size))
        self._stats(what)
        self.b.compact_histories(got_map)
        m.compact_histories(want_map)
        self._histories(what)
        self._routine(what)

    def _csr_equal(self, what):
        got, want = self.b.get_csr(), self.m.csr()
        for name, a, w in zip(("rowptr", "colidx", "values", "nnz_per_group"), got, want):
            assert same_bits(np.asarray(a), np.asarray(w)) if name == "values" else np.array_equal(a, w), (what, "get_csr", name)

    def op_get_csr(self):
        self._csr_equal(("get_csr",))

    def _import(self, fresh):
        what = ("import", "into a fresh plan" if fresh else "into the same plan")
        fast = self.b.export_import(fresh)
        self.m.imported(fast, fresh)
        self._stats(what)
        self._routine(what)

    def op_import_same(self):
        self._import(False)

    def op_import_fresh(self):
        self._import(True)

    def op_flip(self, mode):
        for target in {"sparse": ("LOWERED_SPARSE",), "gemm": ("LOWERED_GEMM",), "both": ("LOWERED_SPARSE", "LOWERED_GEMM")}[mode]:
            self.b.flip(target)
            self.m.flipped(target)
            self._routine(("flip", target))
        self.b.flip(None)      # back to the configuration's own mode
        self.m.flipped(None)
        self._routine(("flip", mode, "back"))

    def op_check(self, fn):
        """A directed test's own assertion between two ops: fn(driver)."""
        fn(self)

    # ---- the end of a sequence: the guarantee every single-op test asserts ------------------------------------------------------
    def finish(self):
        """get_csr against the model, then the plan against a fresh plan with the same options aligned on the model's CSR:
        kernel, tiling, the bits of forward, data gradient and compact weight gradient as the plans stand; then the same
        final calls on both and the accounting, state by state and in total."""
        inp, m = self.inp, self.m
        self._csr_equal(("end",))
        self._stats(("end",))
        ref = self.b.fresh(m.csr())
        plans, top_of = (self.b, ref), lambda top: top if m.relu else None  # noqa: E731
        try:
            assert self.b.kernel_name == ref.kernel_name and self.b.tiling_info == ref.tiling_info, \
                ("end", self.b.kernel_name, ref.kernel_name, self.b.tiling_info, ref.tiling_info)
            # 1. as the plans stand: a stale copy in the sequence's plan shows here
            first = []
            for p in plans:
                top = p.forward(inp.x, inp.b)
                bd, vd, _ = p.backward(inp.td, inp.x, top_of(top), data=True, wgrad="compact", bias=False)
                first.append((top, bd, vd))
            for name, a, w in zip(("forward", "bottom_diff", "values_diff"), first[0], first[1]):
                assert same_bits(a, w), ("end", name, "differs from the fresh plan's")
            # 2. the same final calls on both.  The update comes first: a plan that a fast import left without a value map
            #    rebuilds on it (as the fresh plan never has to), and every state below is then built on both alike.  The
            #    step changes nothing (rate 0 on zero histories) and gives both update states the entry view.
            last = []
            for p in plans:
                p.set_values(m.values, "device")
                top = p.forward(inp.x, inp.b)
                bd, vd, _ = p.backward(inp.td, inp.x, top_of(top), data=True, wgrad="compact", bias=False)
                if p.supports("dense_wgrad"):
                    p.dense_wgrad(inp.ptd, inp.px, top_of(top))
                p.solver_step(vd.copy(), dict(type=sc.SGD, rate=0.0, momentum=0.0), own_histories=True)
                p.set_values(m.values, "device")
                last.append((top, bd, vd, p.accounting(), p.workspace_bytes))
            for name, a, w in zip(("forward", "bottom_diff", "values_diff"), last[0], last[1]):
                assert same_bits(a, w), ("end", name, "after the final calls differs from the fresh plan's")
            # the backward, update and dense-wgrad states and the list's length: equal whatever the sequence did.  The
            # total as well, unless the sequence ran a lowered forward: that sizes a column buffer, which stays
            for key in sorted(set(last[0][3]) - {"device_bytes"}):
                assert last[0][3][key] == last[1][3][key], ("end", key, last[0][3], last[1][3])
            if m.flips == 0:
                assert last[0][4] == last[1][4], ("end", "workspace_bytes", last[0][4], last[1][4], last[0][3], last[1][3])
            else:       # ... so both plans visit the lowered modes (a rebuild: hence last), and then the totals are equal
                toured = []
                for p in plans:
                    tops = []
                    for mode in ("LOWERED_GEMM", "LOWERED_SPARSE", None):
                        p.flip(mode)
                        tops.append((p.kernel_name, p.forward(inp.x, inp.b)))
                    toured.append((tops, p.workspace_bytes))
                for (ka, a), (kw, w) in zip(toured[0][0], toured[1][0]):
                    assert ka == kw and same_bits(a, w), ("end", "forward on the tour of the modes", ka, kw)
                assert toured[0][1] == toured[1][1], ("end", "workspace_bytes after the tour", toured[0][1], toured[1][1])
            got, want = self.b.get_csr(), ref.get_csr()
            assert all(same_bits(np.asarray(a), np.asarray(w)) for a, w in zip(got, want)) and same_bits(got[2], m.values), \
                ("end", "get_csr after the final calls")
        finally:
            ref.close()


# ---- directed sequences: one per transition the single-op tests leave unasserted ----------------------------------------------------
def _upd(op, source, seed):
    return (op, dict(source=source, seed=seed))


BWD = ("backward", dict(bias=True, compact=True, partial=False, accumulate=False, data=True, seed=1))
STEP = ("solver_step", dict(partial=False))


def supported(cfg, ops):
    """The ops of a directed list a configuration's vocabulary holds (removed up front, as in the random sequences)."""
    return [(op, params) for op, params in ops if op == "check" or op in vocabulary(cfg)]


def list_lifecycle(first, grown, same):
    """set_values before the first backward, the backward (a copy appears), set_values again, a solver step (the list is
    rebuilt for the entry view), updates from both sources -- a backward after each: the data gradient reads the copy.
    first / grown / same: the caller's checks of stat update_destinations."""
    chk = lambda fn: ("check", dict(fn=fn))  # noqa: E731
    return [_upd("set_values", "device", 1), chk(first), BWD, _upd("set_values", "device", 2), chk(grown), BWD, STEP, chk(same), BWD,
            _upd("set_values", "host", 3), chk(same), BWD, _upd("update_values", "device", 4), chk(same), BWD, STEP, chk(same),
            _upd("update_values", "host", 5), chk(same), BWD, ("get_csr", {})]


# host-source after device-source updates and the reverse, a host reader between them: the backward state's build, get_csr,
# export_aligned, prune, a conv_mode flip
SOURCES_AND_READERS = [
    _upd("update_values", "device", 1), BWD, _upd("set_values", "host", 2), ("get_csr", {}), _upd("update_values", "device", 3), ("get_csr", {}),
    _upd("set_values", "host", 4), BWD, _upd("set_values", "device", 5), ("import_same", {}), _upd("update_values", "host", 6), BWD, STEP,
    ("prune", dict(mode="keep", frac=0.8, seed=7)), _upd("set_values", "host", 8), BWD, _upd("update_values", "device", 9),
    ("flip", dict(mode="both")),
    _upd("set_values", "host", 10), ("flip", dict(mode="gemm")), _upd("set_values", "device", 11), BWD, STEP, ("flip", dict(mode="sparse")),
    _upd("update_values", "host", 12), ("get_csr", {})]


def fast_import(is_fast, fast0, fast1):
    """A fast import (code present, no value map) -> an update (must rebuild) -> a second import -> a solver step on the
    values-only list -> a step in place -> a third import -> prune -> an update (in place again)."""
    chk = lambda fn: ("check", dict(fn=fn))  # noqa: E731
    return [("import_fresh", {}), chk(is_fast), _upd("update_values", "device", 1), chk(fast0), BWD, ("import_same", {}), chk(is_fast),
            STEP, chk(fast0), STEP, chk(fast1), BWD, ("import_same", {}), chk(is_fast), ("prune", dict(mode="keep", frac=0.8, seed=2)),
            _upd("set_values", "device", 3), chk(fast1),
            BWD, ("get_csr", {})]


def derived_plan_lifecycle(check):
    """What only a plan with an inner plan (option "s2d" / "s2b") has: every point at which the inner plan is torn down and
    rebuilt, an update or a backward on either side of it, and check(driver) after each op.  The points: the first backward
    (the inner or the outer backward copy appears), prune, the conv_mode flips (the lowered modes run without the inner
    plan; an update between two of them), rewire on the checked dense weight gradient, both imports, a prune to nothing and
    a rewire that grows from nothing."""
    ops = [_upd("set_values", "device", 1), BWD, ("prune", dict(mode="keep", frac=0.8, seed=2)), _upd("set_values", "host", 3),
           ("flip", dict(mode="sparse")), _upd("update_values", "device", 4), ("flip", dict(mode="gemm")), ("flip", dict(mode="both")),
           ("rewire", dict(drop="keep", drop_frac=0.8, grow_frac=0.2, init=False, score="dense_wgrad", seed=5)),
           ("import_same", {}), STEP, ("import_fresh", {}), _upd("set_values", "device", 6),
           ("prune", dict(mode="keep", frac=0.0, seed=7)),
           ("rewire", dict(drop=None, drop_frac=1.0, grow_frac=4.0, init=False, score="ties", seed=8)), BWD]
    out = []
    for op in ops:
        out += [op, ("check", dict(fn=check))]
    return out


# The shortest sequence on which a plan of option "s2b" with a forced KERNEL_JIT / KERNEL_TILED was left unaligned: the flip to
# LOWERED_SPARSE rebuilds the plan on the dilated geometry itself, where the forced kernel -- the inner plan's -- does not exist
FLIP_UNDER_A_FORCED_INNER_KERNEL = [("flip", dict(mode="sparse"))]


# The shortest sequence that the device binding refused before solver_step and compact_entries took arrays of 0 elements
# (an empty tensor's pointer is NULL): every entry pruned -- the histories compact into nothing -- then a step
STEP_ON_NOTHING = [STEP, ("prune", dict(mode="keep", frac=0.0, seed=1)), STEP]

# a RigL schedule: dense_wgrad -> rewire -> compact_entries -> solver_step, prunes in between
RIGL = ([("solver_step", dict(partial=False))] * 2 +
        [("rewire", dict(drop="keep", drop_frac=0.8, grow_frac=0.2, init=False, score="dense_wgrad", seed=11)),
         ("solver_step", dict(partial=True)), ("prune", dict(mode="keep", frac=0.7, seed=12)), ("solver_step", dict(partial=False)),
         ("rewire", dict(drop="threshold", drop_frac=0.9, grow_frac=0.3, init=True, score="dense_wgrad", seed=13)),
         ("backward", dict(bias=True, compact=True, partial=False, accumulate=True, data=True, seed=14)),
         ("solver_step", dict(partial=False)), ("get_csr", {})])


def empty_then_grow(check_empty_forward):
    """The ops of the empty-pattern sequence; check_empty_forward(driver) asserts what the forward of an empty plan gives."""
    return [("solver_step", dict(partial=False)),
            ("prune", dict(mode="keep", frac=0.0, seed=1)),            # keep = 0: every entry dropped (see Driver._drop)
            ("check", dict(fn=check_empty_forward)),
            ("solver_step", dict(partial=False)),                      # nnz == 0: nothing is launched
            ("update_values", dict(source="device", seed=2)),          # reads no position: the blob is NaN throughout
            ("rewire", dict(drop=None, drop_frac=1.0, grow_frac=4.0, init=False, score="ties", seed=3)),
            ("solver_step", dict(partial=False)),                      # the grown entries' gradient, within bound, then the step
            ("backward", dict(bias=True, compact=True, partial=False, accumulate=False, data=True, seed=4)),
            ("update_values", dict(source="device", seed=5)),
            ("solver_step", dict(partial=True))]


def empty_forward_is_the_bias(drv):
    """An empty plan's forward is the bias (or 0), exactly."""
    inp = drv.inp
    assert drv.m.nnz == 0 and drv.b.nnz() == 0
    for b in ((inp.b, None) if inp.b is not None else (None,)):
        top = drv.b.forward(inp.x, b)
        want = np.zeros(top.shape, inp.dt) if b is None else np.broadcast_to(b[None, :, None, None], top.shape).astype(inp.dt)
        if drv.m.relu:
            want = np.maximum(want, 0)
        assert np.array_equal(top, want), "the forward of an empty plan is not the bias"
