"""The two backends of the sequence tests (seq_common.Driver): the _cpu twins and the device entry points, each behind one
method per op, numpy in and numpy out.  Imports nothing from the library: the loaded package is handed in."""
import numpy as np

import rewire_common as rc
import solver_common as sc
from prune_common import positions

def _c(a, dt):
    return None if a is None else np.ascontiguousarray(a, dt)


class CpuBackend(object):
    """The _cpu twins behind the driver's interface: weight_align_cpu, forward_cpu, backward_cpu, update_values_cpu,
    solver_step_cpu, prune_cpu, rewire_cpu, dense_wgrad_cpu, get_csr.  `pkg` is the loaded package."""

    def __init__(self, pkg, cfg, inp, csr):
        self.pkg, self.cfg, self.inp, self.dt = pkg, cfg, inp, inp.dt
        self.desc, self.plan = self._make()
        self.h = self.h2 = None
        rp, ci, va, ng = csr
        pos = positions(inp.s, rp, ci, ng)
        w = np.zeros(rc.dense_size(inp.s), self.dt)      # aligned on ones, then updated: explicit zeros stay entries
        w[pos] = 1
        self.plan.weight_align_cpu(w.reshape(self._w_shape()))
        w[pos] = va
        self.plan.update_values_cpu(w.reshape(self._w_shape()))
        self.update_count0 = 1                           # (the construction's own update)
        assert self.plan.nnz() == pos.size

    def _make(self):
        """(descriptor, plan): the one point a derived backend overrides (test_d2s_sequence_cpu.py)."""
        desc = self.pkg.ConvDesc.from_shape(self.inp.s, fuse_relu=self.cfg.relu)
        return desc, self.pkg.Plan(desc)

    def _w_shape(self):
        s = self.inp.s
        return (s.M, s.C // s.group, s.KH, s.KW)

    # facts
    def reports(self, key):
        return key != "update_fast"

    def supports(self, op):
        return op not in self.cfg.exclude

    def stat(self, key):
        return self.plan.stat(key) - (self.update_count0 if key == "update_count" else 0)

    def nnz(self):
        return self.plan.nnz()

    def label(self, kind):
        return "cpu %s" % ("f64" if self.dt == np.float64 else "f32")

    kernel_name = property(lambda self: self.plan.kernel_name)
    tiling_info = property(lambda self: self.plan.tiling_info)
    workspace_bytes = property(lambda self: self.plan.workspace_bytes)

    def accounting(self):
        return {}

    def get_csr(self):
        return self.plan.get_csr()

    def close(self):
        self.plan.close()

    def fresh(self, csr):
        return type(self)(self.pkg, self.cfg, self.inp, csr)

    # computing ops
    def forward(self, x, b, prefill=None, full=None):
        if prefill is None:
            return self.plan.forward_cpu(_c(x, self.dt), _c(b, self.dt))
        oh, ow = self.plan.out_hw
        top = np.full((full, self.inp.s.M, oh, ow), prefill, self.dt)
        self.plan.forward_cpu(_c(x, self.dt), _c(b, self.dt), out=top[:x.shape[0]])
        return top

    def backward(self, td, x, top, data, wgrad, bias, base=None):
        acc = True if base is None else base.copy()
        bd, wd, bsd = self.plan.backward_cpu(_c(td, self.dt), bottom=_c(x, self.dt), top=_c(top, self.dt), bottom_diff=True if data else None,
                                             weight_diff=acc if wgrad == "dense" else None, values_diff=acc if wgrad == "compact" else None,
                                             bias_diff=True if bias else None)
        return bd, wd, bsd

    def dense_wgrad(self, td, x, top):
        return self.plan.dense_wgrad_cpu(_c(td, self.dt), _c(x, self.dt), _c(top, self.dt))

    # mutating ops
    def update_values(self, w, source):
        self.plan.update_values_cpu(_c(w, self.dt))

    def set_values(self, v, source):
        """No set_values twin: the values scattered to the plan's own positions, then update_values_cpu."""
        rp, ci, _, ng = self.plan.get_csr()
        w = np.full(rc.dense_size(self.inp.s), np.nan, self.dt)
        w[positions(self.inp.s, rp, ci, ng)] = v
        self.plan.update_values_cpu(w.reshape(self._w_shape()))

    def _zeros(self, n):
        return np.zeros(n, self.dt)

    def solver_step(self, g, hyper, own_histories=False):
        adam = hyper["type"] == sc.ADAM
        n = self.plan.nnz()
        if own_histories:
            h, h2 = self._zeros(n), (self._zeros(n) if adam else None)
        else:
            if self.h is None:
                self.h = self._zeros(n)
            if adam and self.h2 is None:
                self.h2 = self._zeros(n)
            h, h2 = self.h, (self.h2 if adam else None)
        self._step(_c(g, self.dt), h, h2, hyper)

    def _step(self, g, h, h2, hyper):
        self.plan.solver_step_cpu(g, h, h2, **hyper)

    def histories(self):
        return (None if self.h is None else np.array(self.h), None if self.h2 is None else np.array(self.h2))

    def compact_histories(self, entry_map):
        n = self.plan.nnz()
        if self.h is not None:
            self.h = self.pkg.compact_entries(entry_map, self.h, out=self._zeros(n))
        if self.h2 is not None:
            self.h2 = self.pkg.compact_entries(entry_map, self.h2, out=self._zeros(n))

    def prune(self, keep=None, threshold=None, score=None):
        return self.plan.prune_cpu(keep=keep, threshold=threshold, score=score)

    def rewire(self, grow, score, init=None, drop_keep=None, drop_threshold=None, drop_score=None):
        return self.plan.rewire_cpu(grow, score, init=init, drop_keep=drop_keep, drop_threshold=drop_threshold, drop_score=drop_score)


class GpuBackend(object):
    """The device entry points behind the driver's interface.  `pkg` is the loaded package, `dev` a torch device; the
    configuration's options go to every plan this backend makes (the fresh plan of the end-of-sequence comparison and the
    target of import_fresh included)."""
    _STATS = {"bwd_data_kernel": "dgrad", "wgrad_kernel": "wgrad"}

    def __init__(self, pkg, dev, cfg, inp, csr):
        import torch
        self.torch, self.pkg, self.dev, self.cfg, self.inp, self.dt = torch, pkg, dev, cfg, inp, inp.dt
        self.tdt = torch.float64 if cfg.f64 else torch.float32
        self.opts = {k: getattr(pkg, v) if isinstance(v, str) else v for k, v in cfg.options.items()}
        self.desc = self._describe()
        self.plan = self._new_plan()
        self.plan.set_csr(*csr)
        self.mode = None                 # the conv_mode a flip left (None: the configuration's own, SCONV_PAR)
        self.h = self.h2 = None
        self._const = {}

    def _describe(self):
        """The descriptor: with _new_plan, the one point a derived backend overrides (test_d2s_sequence_gpu.py)."""
        return self.pkg.ConvDesc.from_shape(self.inp.s, fuse_relu=self.cfg.relu)

    def _new_plan(self):
        return self.pkg.Plan(self.desc, **self.opts)

    def _up(self, a):
        return None if a is None else self.torch.from_numpy(np.ascontiguousarray(a, self.dt)).to(self.dev)

    def _in(self, a):
        """A read-only input of the configuration on the device, uploaded once (a slice of it: a view of that upload)."""
        if a is None:
            return None
        for full in (self.inp.x, self.inp.px, self.inp.td, self.inp.ptd, self.inp.b):
            if full is not None and (a is full or a.base is full):
                key = id(full)
                if key not in self._const:
                    self._const[key] = self._up(full)
                return self._const[key][:a.shape[0]]
        return self._up(a)

    def _down(self, t):
        return None if t is None else t.cpu().numpy()

    # facts
    def reports(self, key):
        return True

    def supports(self, op):
        return op not in self.cfg.exclude

    def stat(self, key):
        return self.plan.stat(key)

    def nnz(self):
        return self.plan.nnz()

    def label(self, kind):
        if kind == "forward":
            return self.plan.kernel_name
        if kind == "dense_wgrad":
            return "mfma"
        try:
            return "kernel %d" % self.plan.stat("bwd_data_kernel" if kind == "dgrad" else "wgrad_kernel")
        except self.pkg.EscoinError:      # an empty plan's gradient launches nothing: no kernel is on record
            return "kernel -"

    kernel_name = property(lambda self: self.plan.kernel_name)
    tiling_info = property(lambda self: self.plan.tiling_info)
    workspace_bytes = property(lambda self: self.plan.workspace_bytes)

    def get_csr(self):
        return self.plan.get_csr()

    def close(self):
        self.plan.close()

    def fresh(self, csr):
        return type(self)(self.pkg, self.dev, self.cfg, self.inp, csr)

    def accounting(self):
        """What workspace_bytes is the sum of, and the kernels the backward state chose (for a failure's message)."""
        out = {}
        for k in ("device_bytes", "bwd_device_bytes", "upd_device_bytes", "dwg_device_bytes", "update_destinations", "bwd_data_kernel",
                  "wgrad_kernel"):
            try:
                out[k] = self.plan.stat(k)
            except self.pkg.EscoinError:
                out[k] = None
        return out

    # computing ops
    def forward(self, x, b, prefill=None, full=None):
        torch = self.torch
        xd, bd = self._in(x).contiguous(), self._in(b)
        if prefill is None:
            top = self.plan.forward(xd, bd)
        else:
            oh, ow = self.plan.out_hw
            top = torch.full((full, self.inp.s.M, oh, ow), prefill, dtype=self.tdt, device=self.dev)
            self.plan.forward(xd, bd, top[:x.shape[0]])
        torch.cuda.synchronize()
        return self._down(top)

    def backward(self, td, x, top, data, wgrad, bias, base=None):
        acc = True if base is None else self._up(base)
        bd, wd, bsd = self.plan.backward(self._in(td).contiguous(), bottom=self._in(x).contiguous(), top=self._up(top),
                                         bottom_diff=True if data else None,
                                         weight_diff=acc if wgrad == "dense" else None, values_diff=acc if wgrad == "compact" else None,
                                         bias_diff=True if bias else None)
        self.torch.cuda.synchronize()
        return self._down(bd), self._down(wd), self._down(bsd)

    def dense_wgrad(self, td, x, top):
        out = self.plan.dense_wgrad(self._in(td).contiguous(), self._in(x).contiguous(), self._up(top))
        self.torch.cuda.synchronize()
        return self._down(out)

    # mutating ops
    def _source(self, a, source):
        return self._up(a) if source == "device" else np.ascontiguousarray(a, self.dt)

    def update_values(self, w, source):
        keep = self._source(w, source)
        self.plan.update_values(keep)
        self.torch.cuda.synchronize()

    def set_values(self, v, source):
        keep = self._source(v, source)
        self.plan.set_values(keep)
        self.torch.cuda.synchronize()

    def _zeros(self, n):
        return self.torch.zeros(n, dtype=self.tdt, device=self.dev)

    def solver_step(self, g, hyper, own_histories=False):
        adam = hyper["type"] == sc.ADAM
        n = self.plan.nnz()
        if own_histories:
            h, h2 = self._zeros(n), (self._zeros(n) if adam else None)
        else:
            if self.h is None:
                self.h = self._zeros(n)
            if adam and self.h2 is None:
                self.h2 = self._zeros(n)
            h, h2 = self.h, (self.h2 if adam else None)
        gd = self._up(g)
        self.plan.solver_step(gd, h, h2, **hyper)
        self.torch.cuda.synchronize()

    def histories(self):
        self.torch.cuda.synchronize()
        return self._down(self.h), self._down(self.h2)

    def compact_histories(self, entry_map):
        n = self.plan.nnz()
        m = self.torch.from_numpy(np.ascontiguousarray(entry_map, np.int32)).to(self.dev)
        if self.h is not None:
            self.h = self.pkg.compact_entries(m, self.h, out=self._zeros(n))
        if self.h2 is not None:
            self.h2 = self.pkg.compact_entries(m, self.h2, out=self._zeros(n))
        self.torch.cuda.synchronize()

    def prune(self, keep=None, threshold=None, score=None):
        return self._down(self.plan.prune(keep=keep, threshold=threshold, score=self._up(score)))

    def rewire(self, grow, score, init=None, drop_keep=None, drop_threshold=None, drop_score=None):
        m, grown = self.plan.rewire(grow, self._up(score), init=self._up(init), drop_keep=drop_keep, drop_threshold=drop_threshold,
                                    drop_score=self._up(drop_score))
        return self._down(m), self._down(grown)

    def export_import(self, fresh):
        """export_aligned -> import_aligned into the same plan, or into a new plan with the same options that replaces it.
        Returns stat import_fast."""
        blob = self.plan.export_aligned()
        target = self.plan
        if fresh:
            target = self._new_plan()
            if self.mode is not None:
                target.set_option("conv_mode", getattr(self.pkg, "CONV_MODE_" + self.mode))
        fast = target.import_aligned(blob)
        if fresh:
            self.plan.close()
            self.plan = target
        return fast

    def flip(self, mode):
        """conv_mode to LOWERED_SPARSE / LOWERED_GEMM, or (None) back to the configuration's own."""
        self.plan.set_option("conv_mode", getattr(self.pkg, "CONV_MODE_" + (mode or "SCONV_PAR")))
        self.mode = mode
