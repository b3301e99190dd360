#!/usr/bin/env python3
"""Seeded random convolution geometries through the pattern-preserving Backward (escoin_backward[_values][_f64] and the CPU
mode) against torch float64 autograd on the CPU: the data gradient through every backward_kernel (the transposed forward
plan on every forward kernel family, the gather kernel bit for bit against the CPU mode), the weight / bias gradient under
every wgrad_kernel in dense and compact form, accumulation into prefilled blobs, calls on fewer images than the plan's
batch, blobs that are windows of larger allocations off a 16-byte boundary, in-place weight updates between two calls, and
determinism.  One case in four runs on inputs whose rows, channels and images differ in scale by up to 2^48
(tools/error_bound.py skew) and is checked element by element against the derived bound instead of the max-norm; which cases
is drawn from a second generator, so a (seed, k) names the same geometry and weights as before.  A sibling of
tools/fuzz_parity.py.
    python tools/fuzz_backward.py [cases] [seed] [--cpu] > fuzz_backward.txt
Prints one line per failure (everything needed to rebuild the case) and a summary; exit code 1 on any failure.  Unlike
fuzz_parity.py an exception that is not a documented refusal (EscoinError, ESCOIN_EINVAL) ends the run at once: nothing
more is started on a device after a runtime error."""
import os
import sys
import time
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import __graft_entry__ as ge  # noqa: E402
import error_bound as eb  # noqa: E402
from conftest import rel_err  # noqa: E402
from upd_common import new_weights  # noqa: E402
from wgrad_common import csr_positions, tiled_ok, torch_backward  # noqa: E402

TOL = 1e-4          # the project's fp32 tolerance (tests/test_backward_gpu.py)
TOL_F64 = 1e-12
SENTINEL = -1234.5  # exact in float32

SKEW_STREAM = 0x5CA1E       # which cases are skewed: RandomState(seed ^ SKEW_STREAM), apart from the generator's own
SKEWED = "(cases skewed and checked per element)"

Case = namedtuple("Case", "k cls s dist relu tb mlb f64 accumulate n_part window update skew")

DATA_KERNELS = ("auto", "generic", "tiled", "jit", "dense")
KERNEL_NAMES = {0: "auto", 1: "generic", 2: "tiled", 3: "dense", 4: "jit"}
WGRAD_NAMES = {0: "auto", 1: "entry", 2: "staged", 3: "mfma"}


# ---- generator and geometry predicates (no device, no library) --------------------------------------------------------
def generate(cases, seed, synth):
    """The `cases` cases of `seed`, classes by k % 5 -- 0: anything goes, 1: stride 1 (the transposed plan and the staged
    kernel serve it), 2: pointwise, 3: many channels, 4: many small images.  Sizes are the smallest that still cross
    each boundary: 1024-pixel chunks that span several images, tile slots past the batch, more than one channel block."""
    rng = np.random.RandomState(seed)
    rng_skew = np.random.RandomState((seed ^ SKEW_STREAM) & 0xFFFFFFFF)
    out = []
    for k in range(cases):
        cls = k % 5
        KH = int(rng.choice([1, 1, 2, 3, 3, 3, 4, 5, 7]))
        KW = KH if rng.randint(4) else int(rng.choice([1, 2, 3, 5]))
        if cls == 2:
            KH = KW = 1
        sh, sw = (1, 1) if cls != 0 and rng.randint(4) else (int(rng.choice([1, 2, 3])), int(rng.choice([1, 2, 3])))
        if cls == 1:
            sh = sw = 1
        if cls == 2:
            sh = sw = 2 if rng.randint(3) == 0 else 1
        dh, dw = (1, 1) if cls != 0 or rng.randint(3) else (int(rng.choice([1, 2, 3])), int(rng.choice([1, 2, 3])))
        ph = int(rng.randint(0, KH)) if KH > 1 else 0
        pw = int(rng.randint(0, KW)) if KW > 1 else 0
        if rng.randint(8) == 0 and cls != 1:
            ph, pw = ph + dh * (KH - 1) + 1, pw + 2         # more padding than the kernel reaches
        eh, ew = dh * (KH - 1) + 1, dw * (KW - 1) + 1
        lo_h, lo_w = max(eh - 2 * ph, 1), max(ew - 2 * pw, 1)
        group = int(rng.choice([1, 1, 1, 2, 3, 4]))
        if cls == 3:
            C, M = group * int(rng.randint(40, 161)), group * int(rng.randint(30, 161))
            N = int(rng.randint(1, 4))
            H, W = int(rng.randint(lo_h, max(lo_h, 14) + 1)), int(rng.randint(lo_w, max(lo_w, 20) + 1))
        elif cls == 4:
            C, M = group * int(rng.randint(1, 12)), group * int(rng.randint(1, 41))
            N = int(rng.randint(100, 301))
            H, W = int(rng.randint(lo_h, max(lo_h, 10) + 1)), int(rng.randint(lo_w, max(lo_w, 10) + 1))
        else:
            C, M = group * int(rng.randint(1, 41)), group * int(rng.randint(1, 41))
            N = int(rng.randint(1, 13))
            H, W = int(rng.randint(lo_h, max(lo_h, 30) + 1)), int(rng.randint(lo_w, max(lo_w, 66) + 1))
        sp = float(rng.choice([0.0, 0.3, 0.5, 0.7, 0.8, 0.9, 0.95, 0.99, 1.0]))
        dist = str(rng.choice(synth.SPARSITY_DISTS))
        bias, relu = bool(rng.randint(2)), bool(rng.randint(3) == 0)
        tb = int(rng.choice([0, 0, 64, 256, 257]))
        s = synth.shape("bz%d" % k, N, C, H, W, M, KH, KW=KW, pad=ph, pad_w=pw, stride=sh, stride_w=sw, dil=dh, dil_w=dw,
                        group=group, sparsity=sp, bias=bias)
        oh, ow = synth.out_hw(s)
        # sub-batch launches: a few images' worth of the larger of the forward's and the transposed plan's bottom
        mlb = 4 * max(C * H * W, M * oh * ow) * int(rng.randint(3, 9)) + 100 if cls == 4 and rng.randint(2) else 0
        f64 = rng.randint(5) == 0
        accumulate = rng.randint(3) == 0
        n_part = int(rng.randint(1, N)) if N > 1 and rng.randint(3) == 0 else 0
        window = int(rng.choice([1, 3])) if rng.randint(4) == 0 else 0
        update = rng.randint(5) == 0
        out.append(Case(k, cls, s, dist, relu, tb, mlb, bool(f64), bool(accumulate), n_part, window, bool(update),
                        bool(rng_skew.randint(4) == 0)))
    return out


def geometry_transposable(s):
    """tests/test_backward_gpu.py's _transposable: stride 1 and no more padding than the kernel reaches."""
    return (s.stride_h == 1 and s.stride_w == 1 and s.pad_h <= s.dil_h * (s.KH - 1) and
            s.pad_w <= s.dil_w * (s.KW - 1))


def transposable(c):
    """Whether the library serves the case by a transposed forward plan: the geometry, a float plan, and an output
    channel index of a group that fits 15 bits."""
    return geometry_transposable(c.s) and not c.f64 and c.s.M // c.s.group <= 32767


def transposed_shape(synth, s):
    """The forward layer whose output is the data gradient: C and M swapped, pad' = dil * (K - 1) - pad, groups kept."""
    oh, ow = synth.out_hw(s)
    return synth.shape(s.name + "^T", s.N, s.M, oh, ow, s.C, s.KH, KW=s.KW, pad=s.dil_h * (s.KH - 1) - s.pad_h,
                       pad_w=s.dil_w * (s.KW - 1) - s.pad_w, dil=s.dil_h, dil_w=s.dil_w, group=s.group, bias=False)


def tiled_admits(synth, c):
    """A forced TILED / JIT may be refused only when this is False: tiled_ok (tests/test_gpu_parity.py's geometry
    predicate) of the transposed descriptor.  The one refusal it does not model is the stream kernel's size limit, which
    depends on the weights: STREAM_REFUSAL below."""
    return transposable(c) and tiled_ok(transposed_shape(synth, c.s))


# escoin_capi.hip: a forced TILED whose weight stream (a function of the nonzeros, not of the geometry) exceeds the LDS
# left beside the input planes.  tools/fuzz_parity.py accepts the same refusal of the forward.
STREAM_REFUSAL = "tiled kernel requested but its weight stream does not fit the LDS budget"
STREAM_REFUSALS = "tiled refusals (admitted geometry: the weight stream exceeds the LDS budget)"
AUTO_FAST = "(AUTO ran a fast kernel where the transposed descriptor is admitted and not pointwise)"


def auto_fast_candidate(synth, c):
    """Cases whose AUTO data gradient must show a fast kernel in bwd_data_kernel: the transposed plan exists and the tiled
    families cover it.  (Pointwise launches are left out: KERNEL_AUTO's small-launch rule may give them the generic
    kernel; so are plans without a nonzero, for which there is neither code nor a stream to build.)  GENERIC there would
    mean the gather kernel, or a transposed plan that fell back."""
    return tiled_admits(synth, c) and c.s.KH * c.s.KW > 1 and c.s.sparsity < 1.0


def data_kernels(c):
    """The backward_kernel values a case is run under."""
    return DATA_KERNELS if geometry_transposable(c.s) else DATA_KERNELS[:2]


def staged_candidate(c):
    """Float stride-1 cases: the staged weight-gradient kernel serves them unless a chunk tile exceeds its LDS budget."""
    return not c.f64 and c.s.stride_h == 1 and c.s.stride_w == 1


def expected_runs(synth, cs):
    """What a clean device run of these cases must at least have done (the suite's coverage floors)."""
    e = dict(transposed=0, gather=0, jit=0, staged_candidates=0, auto_fast=0)
    for c in cs:
        for kn in data_kernels(c):
            if kn == "generic" or not transposable(c):
                e["gather"] += kn in ("auto", "generic")
            elif kn in ("auto", "dense") or tiled_admits(synth, c):
                e["transposed"] += 1
        e["jit"] += tiled_admits(synth, c)
        e["staged_candidates"] += staged_candidate(c)
        e["auto_fast"] += auto_fast_candidate(synth, c)
    return e


def inputs(synth, c):
    """(w, x, bias, top_diff) of a case in its dtype; the double cases hold the float values.  A skewed case's are scaled
    by exact powers of two (error_bound.skew)."""
    s = c.s
    dt = np.float64 if c.f64 else np.float32
    w = synth.pruned_weights(s, 1000 + c.k, dist=c.dist)
    b = synth.bias_vector(s, 2000 + c.k)
    x = synth.activations(s, 3000 + c.k)
    oh, ow = synth.out_hw(s)
    td = np.random.RandomState(4000 + c.k).uniform(-1, 1, (s.N, s.M, oh, ow)).astype(np.float32)
    if c.skew:
        sk = eb.skew(s, w, x, b, 7000 + c.k, top_diff=td)
        w, x, b, td = sk.w, sk.x, sk.b, sk.top_diff
    return w.astype(dt), x.astype(dt), None if b is None else b.astype(dt), td.astype(dt)


def describe(seed, c):
    s = c.s
    return ("seed=%d k=%d %s dist=%s relu=%d tb=%d mlb=%d f64=%d acc=%d n_part=%d window=%d update=%d skew=%d" %
            (seed, c.k, tuple(s[1:17]), c.dist, c.relu, c.tb, c.mlb, c.f64, c.accumulate, c.n_part, c.window, c.update, c.skew))


def _prefill(c, w, pattern):
    """The accumulation case's blobs before the call: seeded values at the pattern and NaN outside it, seeded bias."""
    rs = np.random.RandomState(5000 + c.k)
    wd0 = np.where(pattern, rs.uniform(-1, 1, w.shape), np.nan).astype(w.dtype)
    bsd0 = rs.uniform(-1, 1, (c.s.M,)).astype(w.dtype)
    return wd0, bsd0


def _same_nan_bits(a, b, where):
    return a[where].tobytes() == b[where].tobytes()


class _Checker(object):
    """Collects failure lines; every line carries the seed, k, the shape tuple and the options."""

    def __init__(self, seed, out):
        self.seed, self.out, self.lines, self.worst = seed, out, [], {}

    def fail(self, c, what):
        line = "FAIL %s: %s" % (what, describe(self.seed, c))
        self.lines.append(line)
        print(line, file=self.out, flush=True)

    def close(self, c, what, got, want, tol):
        if got.shape != want.shape:
            self.fail(c, "%s: shape %s, want %s" % (what, got.shape, want.shape))
            return
        err = rel_err(got, want) if got.size else 0.0
        if not err <= tol:
            self.fail(c, "%s: rel err %.3g > %.3g" % (what, err, tol))

    def same(self, c, what, a, b):
        if a.shape != b.shape or a.tobytes() != b.tobytes():
            self.fail(c, "%s: bytes differ (rel err %.3g)" % (what, rel_err(a, b) if a.shape == b.shape and a.size else -1))

    def bounded(self, c, what, got, want, B, name):
        """A skewed case's check: every element within its bound (error_bound.check); the worst ratio is kept per `name`."""
        if got.shape != want.shape:
            self.fail(c, "%s: shape %s, want %s" % (what, got.shape, want.shape))
            return
        ratio, idx = eb.check(got, want, B)
        self.worst[name] = max(self.worst.get(name, 0.0), ratio)
        if not ratio <= 1.0:
            self.fail(c, "%s via %s: element %s off by %.3g x its bound (got %r, want %r)" %
                      (what, name, idx, ratio, float(got[idx]), float(want[idx])))

    def gradients(self, c, what, got, want, pattern, tol, base=None, bounds=None, names=("", ""), n_images=None):
        """(bottom_diff, weight_diff, bias_diff) against the reference; with `base` = (weight_diff, bias_diff) before
        the call the outputs accumulated: base + gradient at the pattern, the bits outside it unchanged.  With `bounds`
        (a skewed case: error_bound.backward_bound's) every element is held to its bound instead of the max-norm `tol`;
        names: (data-gradient kernel, weight-gradient kernel) for the summary."""
        bd, wd, bsd = got
        if bd is not None:
            if bounds is None:
                self.close(c, what + " bottom_diff", bd, want[0], tol)
            else:
                self.bounded(c, what + " bottom_diff", bd, want[0], bounds[0], names[0])
        n_terms = (c.s.N if n_images is None else n_images) * int(np.prod(ge.load_package().synth.out_hw(c.s)))
        if wd is not None:
            if base is None:
                if bounds is None:
                    self.close(c, what + " weight_diff", wd, want[1], tol)
                else:
                    self.bounded(c, what + " weight_diff", wd, want[1], bounds[1], names[1])
                if np.any(wd[~pattern] != 0):
                    self.fail(c, what + " weight_diff: written outside the pattern")
            else:
                acc_want = np.where(pattern, base[0].astype(np.float64) + want[1], 0)
                if bounds is None:
                    self.close(c, what + " weight_diff (accumulated)", np.where(pattern, wd, 0), acc_want, tol)
                else:
                    B = eb.accumulated_bound(bounds[1], np.where(pattern, base[0], 0), n_terms, c.f64)
                    self.bounded(c, what + " weight_diff (accumulated)", np.where(pattern, wd, 0), acc_want, B, names[1])
                if not _same_nan_bits(wd, base[0], ~pattern):
                    self.fail(c, what + " weight_diff: the prefill outside the pattern changed")
        if bsd is not None:
            bwant = want[2] if base is None else base[1].astype(np.float64) + want[2]
            if bounds is None:
                self.close(c, what + " bias_diff", bsd, bwant, tol)
            else:
                B = bounds[2] if base is None else eb.accumulated_bound(bounds[2], base[1], n_terms, c.f64)
                self.bounded(c, what + " bias_diff", bsd, bwant, B, names[1] + " bias")


# ---- CPU mode -----------------------------------------------------------------------------------------------------------
def _reference(c, x, w, b, td, top, mask=None):
    """(the float64 gradients, their per-element bounds for a skewed case or None)."""
    if c.skew:
        return eb.backward_bound(c.s, w, x, b, td, top, f64=c.f64, mask=mask)
    return torch_backward(x, w, b, c.s, td, top, mask=mask), None


def _cpu_case(pkg, synth, c0, chk, count):
    s = c0.s
    w32, x32, b32, td32 = inputs(synth, c0._replace(f64=False))
    pattern = w32 != 0
    want = None
    for dt in (np.float32, np.float64):
        c = c0._replace(f64=dt == np.float64)       # (the dtype of this pass: what the bounds and a failure line go by)
        tol = TOL if dt == np.float32 else TOL_F64
        w, x, td = w32.astype(dt), x32.astype(dt), td32.astype(dt)
        b = None if b32 is None else b32.astype(dt)
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=c.relu))
        plan.weight_align_cpu(w)
        top = plan.forward_cpu(x, b) if c.relu else None
        # (the float and the double forward may disagree on the sign of an output next to zero: one reference each then;
        #  a skewed case's bounds depend on the dtype)
        if want is None or c.relu or c.skew:
            want, bounds = _reference(c, x, w, b, td, top)
        what = "cpu %s" % np.dtype(dt).name
        names = (what + " data", what + " weights")
        got = plan.backward_cpu(td, bottom=x, top=top, weight_diff=True, bias_diff=True if b is not None else None)
        chk.gradients(c, what, got, want, pattern, tol, bounds=bounds, names=names)
        _, vd, bsd2 = plan.backward_cpu(td, bottom=x, top=top, bottom_diff=None, values_diff=True,
                                        bias_diff=True if b is not None else None)
        chk.same(c, what + " values_diff against weight_diff at the CSR positions", vd, got[1].reshape(-1)[csr_positions(plan)])
        if b is not None:
            chk.same(c, what + " bias_diff of the compact call", bsd2, got[2])
        again = plan.backward_cpu(td, bottom=x, top=top, weight_diff=True, bias_diff=True if b is not None else None)
        for name, a, e in zip(("bottom_diff", "weight_diff", "bias_diff"), again, got):
            if a is not None:
                chk.same(c, what + " second call " + name, a, e)
        count("cpu backward calls", 3)
        if c.accumulate:
            wd0, bsd0 = _prefill(c, w, pattern)
            wd, bsd = wd0.copy(), bsd0.copy() if b is not None else None
            acc = plan.backward_cpu(td, bottom=x, top=top, weight_diff=wd, bias_diff=bsd)
            chk.gradients(c, what + " accumulate", acc, want, pattern, tol, base=(wd0, bsd0), bounds=bounds, names=names)
            chk.same(c, what + " accumulate bottom_diff", acc[0], got[0])
            count("accumulation cases", dt == np.float32)
        if c.n_part:
            n = c.n_part
            ptop = None if top is None else top[:n]
            pwant, pbounds = _reference(c, x[:n], w, b, td[:n], ptop)
            part = plan.backward_cpu(td[:n], bottom=x[:n], top=ptop, weight_diff=True, bias_diff=True if b is not None else None)
            chk.gradients(c, what + " partial %d" % n, part, pwant, pattern, tol, bounds=pbounds, names=names, n_images=n)
            chk.same(c, what + " partial %d bottom_diff against the full call's" % n, part[0], got[0][:n])
            count("partial calls", dt == np.float32)
        plan.close()
    count(SKEWED, c0.skew)


# ---- device ------------------------------------------------------------------------------------------------------------
class _Refused(Exception):
    pass


def _refusal(pkg, e):
    """A documented refusal: EscoinError carrying ESCOIN_EINVAL.  Everything else (a HIP runtime error included) stops the
    run."""
    return isinstance(e, pkg.EscoinError) and "failed (-1)" in str(e)


def _device_case(pkg, synth, torch, dev, c, chk, count):
    s = c.s
    w, x, b, td = inputs(synth, c)
    dt = w.dtype
    tol = TOL_F64 if c.f64 else TOL
    pattern = w != 0
    has_b = b is not None
    tdt = torch.float64 if c.f64 else torch.float32
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    down = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731

    def window(a=None, shape=None, fill=float("nan")):
        """A blob as a view into a larger allocation, c.window elements past a 16-byte boundary: (allocation, view, lead)."""
        shape = a.shape if a is not None else shape
        n, lead = int(np.prod(shape)), 64 + c.window
        big = torch.full((lead + n + 67,), fill, dtype=tdt, device=dev)
        view = big[lead:lead + n].view(tuple(shape))
        if a is not None:
            view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        return big, view, lead

    def intact(what, big, view, lead):
        h = big.cpu().numpy()
        n = view.numel()
        if np.any(h[:lead] != SENTINEL) or np.any(h[lead + n:] != SENTINEL):
            chk.fail(c, what + ": written outside the blob")

    xd, bd_, tdd = up(x), up(b), up(td)
    opts = {"tiling_batch": c.tb}
    if c.mlb:
        opts["max_launch_bytes"] = c.mlb
    refs = {}

    def reference(key, xx, ww, tt, top, mask=None):
        if key not in refs:
            refs[key] = _reference(c, xx, ww, b, tt, top, mask=mask)
        return refs[key]

    # (data kernel, weight-gradient kernel, outputs asked for)
    runs = [(kn, "auto", True) for kn in data_kernels(c)]
    runs[1] = ("generic", "entry", True)
    runs.append(("generic", "staged", False))
    runs.append(("generic", "mfma", False))
    top_np = None
    for kn, wk, want_bd in runs:
        kernel = getattr(pkg, "KERNEL_" + kn.upper())
        what = "%s/%s" % (kn, wk)
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=c.relu), backward_kernel=kernel,
                        wgrad_kernel=getattr(pkg, "WGRAD_" + wk.upper()), **opts)
        try:
            plan.weight_align(w)
            top = plan.forward(xd, bd_) if c.relu else None
            if c.relu and top_np is None:
                top_np = down(top)      # every plan of the case has the same forward: one mask, one reference
            topd = up(top_np)
            want, bounds = reference("full", x, w, td, top_np)
            call = dict(bottom=xd, top=topd, bottom_diff=True if want_bd else None, weight_diff=True,
                        bias_diff=True if has_b else None)
            try:
                r1 = plan.backward(tdd, **call)
            except pkg.EscoinError as e:
                if not _refusal(pkg, e):
                    raise
                if wk == "staged":
                    if staged_candidate(c):
                        count("staged refusals (float, stride 1: the LDS budget)", 1)
                    continue
                if wk == "mfma" and c.f64:
                    count("mfma refusals (double plans)", 1)
                    continue
                fast = kn in ("tiled", "jit", "dense")
                if fast and (not transposable(c) or (kn != "dense" and not tiled_admits(synth, c))):
                    continue
                if kn == "tiled" and STREAM_REFUSAL in str(e):
                    count(STREAM_REFUSALS, 1)
                    continue
                chk.fail(c, "%s refused: %s" % (what, e))
                continue
            torch.cuda.synchronize()
            got = tuple(down(t) for t in r1)
            ran_k, ran_w = plan.stat("bwd_data_kernel"), plan.stat("wgrad_kernel")
            how = dict(bounds=bounds, names=("bwd_data_kernel " + KERNEL_NAMES[ran_k], "wgrad_kernel " + WGRAD_NAMES[ran_w]))
            chk.gradients(c, what, got, want, pattern, tol, **how)
            if want_bd:
                count("bwd_data_kernel " + KERNEL_NAMES[ran_k], 1)
                on_tplan = transposable(c) and kn != "generic"
                count("(data gradients on the transposed plan)" if on_tplan else "(data gradients on the gather kernel)", 1)
                if not on_tplan and ran_k != pkg.KERNEL_GENERIC:
                    chk.fail(c, "%s: bwd_data_kernel %d where only the gather kernel serves" % (what, ran_k))
                if on_tplan and kn != "auto" and ran_k != kernel:
                    chk.fail(c, "%s: bwd_data_kernel %d, forced %d" % (what, ran_k, kernel))
                if kn == "auto" and auto_fast_candidate(synth, c):
                    count(AUTO_FAST, ran_k != pkg.KERNEL_GENERIC)
            count("wgrad_kernel " + WGRAD_NAMES[ran_w], 1)
            if wk != "auto" and ran_w != getattr(pkg, "WGRAD_" + wk.upper()):
                chk.fail(c, "%s: wgrad_kernel %d ran" % (what, ran_w))
            # compact form: bit-equal to the dense form gathered at the CSR positions
            _, vd, _ = plan.backward(tdd, bottom=xd, top=topd, bottom_diff=None, values_diff=True)
            chk.same(c, what + " values_diff against weight_diff at the CSR positions", down(vd),
                     got[1].reshape(-1)[csr_positions(plan)])
            # determinism
            r2 = plan.backward(tdd, **call)
            torch.cuda.synchronize()
            for name, a, e in zip(("bottom_diff", "weight_diff", "bias_diff"), r2, got):
                if a is not None:
                    chk.same(c, what + " second call " + name, down(a), e)
            # the gather kernel keeps the CPU mode's order
            if kn == "generic" and want_bd:
                cpu = plan.backward_cpu(td, bottom=x, top=top_np, weight_diff=True)
                chk.same(c, what + " bottom_diff against the CPU mode's", got[0], cpu[0])
            if c.accumulate:
                wd0, bsd0 = _prefill(c, w, pattern)
                acc = plan.backward(tdd, bottom=xd, top=topd, bottom_diff=None, weight_diff=up(wd0),
                                    bias_diff=up(bsd0) if has_b else None)
                torch.cuda.synchronize()
                chk.gradients(c, what + " accumulate", tuple(down(t) for t in acc), want, pattern, tol, base=(wd0, bsd0), **how)
                count("accumulation cases", kn == "auto")
            if c.n_part:
                n = c.n_part
                ptop = None if top_np is None else top_np[:n]
                pwant, pbounds = reference("part", x[:n], w, td[:n], ptop)
                full = torch.full((s.N, s.C, s.H, s.W), SENTINEL, dtype=tdt, device=dev)
                part = plan.backward(tdd[:n], bottom=xd[:n], top=None if topd is None else topd[:n],
                                     bottom_diff=full[:n] if want_bd else None, weight_diff=True,
                                     bias_diff=True if has_b else None)
                torch.cuda.synchronize()
                pg = tuple(down(t) for t in part)
                chk.gradients(c, what + " partial %d" % n, pg, pwant, pattern, tol, n_images=n, **dict(how, bounds=pbounds))
                if want_bd:
                    chk.same(c, what + " partial %d bottom_diff against the full call's" % n, pg[0], got[0][:n])
                    if np.any(down(full[n:]) != SENTINEL):
                        chk.fail(c, what + " partial %d: bottom_diff rows past the call's images written" % n)
                count("partial calls", 1)
            if c.window:
                ins = [window(x), window(td)] + ([window(top_np)] if c.relu else [])
                wd0, bsd0 = _prefill(c, w, pattern) if c.accumulate else (np.zeros_like(w), np.zeros(s.M, dt))
                outs = [window(shape=x.shape, fill=SENTINEL) if want_bd else None, window(wd0, fill=SENTINEL),
                        window(bsd0, fill=SENTINEL) if has_b else None]
                res = plan.backward(ins[1][1], bottom=ins[0][1], top=ins[2][1] if c.relu else None,
                                    bottom_diff=outs[0][1] if want_bd else None, weight_diff=outs[1][1],
                                    bias_diff=outs[2][1] if has_b else None)
                torch.cuda.synchronize()
                wg = tuple(down(t) for t in res)
                for name, a in zip(("bottom_diff", "weight_diff", "bias_diff"), wg):
                    if a is not None and np.any(np.isnan(a if name != "weight_diff" else a[pattern])):
                        chk.fail(c, "%s window +%d: NaN from outside an input blob reached %s" % (what, c.window, name))
                chk.gradients(c, what + " window +%d" % c.window, wg, want, pattern, tol,
                              base=(wd0, bsd0) if c.accumulate else None, **how)
                for name, o in zip(("bottom_diff", "weight_diff", "bias_diff"), outs):
                    if o is not None:
                        intact("%s window +%d %s" % (what, c.window, name), *o)
                count("window cases", kn == "auto")
            if c.update:
                w_new, w_nan = new_weights(w, 6000 + c.k)
                plan.update_values(up(w_nan))
                utop = plan.forward(xd, bd_) if c.relu else None
                utop_np = down(utop)
                # (the new top is this plan's own: its forward kernel family may differ in the last bits from another's)
                uwant, ubounds = _reference(c, x, w_new, b, td, utop_np, mask=pattern)
                ur = plan.backward(tdd, bottom=xd, top=utop, bottom_diff=True if want_bd else None, weight_diff=True,
                                   bias_diff=True if has_b else None)
                torch.cuda.synchronize()
                chk.gradients(c, what + " after update_values", tuple(down(t) for t in ur), uwant, pattern, tol,
                              **dict(how, bounds=ubounds))
                count("update cases", kn == "auto")
        finally:
            plan.close()
    count(SKEWED, c.skew)


def fuzz(cases, seed, out=sys.stdout, device=True, worst=None):
    """Runs `cases` random geometries; returns (runs, failure lines, counts by name).  device=False: the same generator
    and reference through backward_cpu only (no torch.cuda).  worst: a dict that receives the largest err / bound of the
    skewed cases per kernel name."""
    pkg = ge.load_package()
    synth = pkg.synth
    chk = _Checker(seed, out)
    by_name = {}

    def count(name, n):
        by_name[name] = by_name.get(name, 0) + int(n)
    if device:
        import torch
        dev = torch.device("cuda:0")
    for name in ("partial calls", "accumulation cases", "window cases", "update cases", SKEWED,
                 "staged refusals (float, stride 1: the LDS budget)", STREAM_REFUSALS, AUTO_FAST):
        count(name, 0)
    t0 = time.time()
    for c in generate(cases, seed, synth):
        try:
            if device:
                _device_case(pkg, synth, torch, dev, c, chk, count)
            else:
                _cpu_case(pkg, synth, c, chk, count)
        except Exception as e:      # not a refusal: nothing more is started
            chk.fail(c, "stopped by %s: %s" % (type(e).__name__, e))
            break
        if c.k % 50 == 49:
            print("# %d cases, %d failures, %.0f s" % (c.k + 1, len(chk.lines), time.time() - t0), file=out, flush=True)
    runs = sum(v for n, v in by_name.items() if n.startswith(("bwd_data_kernel", "wgrad_kernel", "cpu backward")))
    if worst is not None:
        worst.update(chk.worst)
    return runs, chk.lines, by_name


def main():
    args = [a for a in sys.argv[1:] if a != "--cpu"]
    cases = int(args[0]) if len(args) > 0 else 300
    seed = int(args[1]) if len(args) > 1 else 20261019
    t0 = time.time()
    worst = {}
    ran, lines, by_name = fuzz(cases, seed, device="--cpu" not in sys.argv[1:], worst=worst)
    print("cases %d seed %d runs %d failures %d seconds %.0f" % (cases, seed, ran, len(lines), time.time() - t0))
    for n in sorted(by_name):
        print("  %-60s %d" % (n, by_name[n]))
    print("worst err / bound of the skewed cases, per kernel:")
    for n in sorted(worst):
        print("  %-60s %.3g" % (n, worst[n]))
    sys.exit(1 if lines else 0)


if __name__ == "__main__":
    main()
