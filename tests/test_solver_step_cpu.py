"""escoin_solver_step_cpu / escoin_solver_array_step_cpu (no GPU needed): the solver's rule fused into the weight update, on
plans that live on the host.  The yardstick is solver_common.step -- numpy, op by op in the case's dtype -- and every
comparison is bit equality: values, histories, the forward against a second plan brought to the same values by
escoin_update_values_cpu."""
import ctypes as C

import numpy as np
import pytest

import solver_common as sc
from plan_model import positions
from upd_common import new_weights, values_at

HYPER = dict(rate=0.01, momentum=0.9, momentum2=0.999, delta=1e-8, decay=5e-4)
SCALE = 1.0 / 3.0


def _shapes(synth):
    return {"lenet_conv2": synth.lenet_conv2(N=2)[0],
            "group2_3x3": synth.shape("mixed_g2", 2, 64, 14, 14, 64, 3, pad=1, group=2, sparsity=0.7)}


class Twin(object):
    """A CPU-aligned plan whose pattern holds explicit zeros (one of them -0.0), a second plan that follows it through
    escoin_update_values_cpu, and the restatement's copy of the state."""

    def __init__(self, pkg, synth, s, dt, rule):
        self.pkg, self.s, self.dt = pkg, s, dt
        w0 = synth.pruned_weights(s, 7).astype(dt)
        self.mask = w0 != 0
        w1, _ = new_weights(w0, 8)                 # a few kept weights exactly 0, one -0.0: explicit zeros of the pattern
        b = synth.bias_vector(s, 9)
        self.b = None if b is None else b.astype(dt)
        self.x = synth.activations(s, 10).astype(dt)
        self.desc = pkg.ConvDesc.from_shape(s)
        self.plan, self.other = pkg.Plan(self.desc), pkg.Plan(self.desc)
        for p in (self.plan, self.other):
            p.weight_align_cpu(w0)
            p.update_values_cpu(w1)
        rp, ci, va, ng = self.plan.get_csr()
        self.pos = positions(self.desc, rp, ci, ng)
        self.w = va.copy()
        assert sc.bits_equal(self.w, values_at(self.plan, w1)[2])
        assert np.count_nonzero(self.w == 0) >= 4 and np.any(np.signbit(self.w) & (self.w == 0))
        n = self.w.size
        self.h, self.want_h = np.zeros(n, dt), np.zeros(n, dt)
        adam = rule == sc.ADAM
        self.h2, self.want_h2 = (np.zeros(n, dt), np.zeros(n, dt)) if adam else (None, None)
        self.shape = w0.shape

    def dense(self, compact, fill):
        out = np.full(int(np.prod(self.shape)), fill, self.dt)
        out[self.pos] = compact
        return out.reshape(self.shape)

    def check(self, step):
        va = self.plan.get_csr()[2]
        assert sc.bits_equal(va, self.w), step
        assert sc.bits_equal(self.h, self.want_h), step
        assert self.h2 is None or sc.bits_equal(self.h2, self.want_h2), step
        self.other.update_values_cpu(self.dense(self.w, np.nan))
        got, want = self.plan.forward_cpu(self.x, self.b, n_threads=2), self.other.forward_cpu(self.x, self.b, n_threads=2)
        assert np.array_equal(got, want) and np.all(np.isfinite(got)), step

    def close(self):
        self.plan.close()
        self.other.close()


@pytest.mark.parametrize("variant", ["compact", "scaled_cleared_rate_ptr", "dense_layout"])
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["float", "double"])
@pytest.mark.parametrize("reg", ["none", "L2", "L1"])
@pytest.mark.parametrize("rule", ["sgd", "nesterov", "adam"])
@pytest.mark.parametrize("shape", ["lenet_conv2", "group2_3x3"])
def test_three_steps_equal_the_restatement(pkg, synth, shape, rule, reg, dt, variant):
    """Three consecutive steps with seeded gradients.  compact: values_diff, no scale, diff kept.  scaled_cleared_rate_ptr:
    diff_scale = 1/3, clear_diff, and the rate read through rate_dev (desc.rate holds a decoy).  dense_layout: diff and
    dense_w are blobs_[0]-shaped with NaN outside the pattern, which is neither read nor written."""
    t = Twin(pkg, synth, _shapes(synth)[shape], dt, sc.RULES[rule])
    hyper = dict(HYPER, type=sc.RULES[rule], regularization=sc.REGS[reg])
    n = t.w.size
    rate_cell = np.zeros(1, dt)
    for k in range(3):
        g = sc.seeded_values(n, 100 + k, dt)
        rate = HYPER["rate"] * (0.5 ** k)
        scale = SCALE if variant == "scaled_cleared_rate_ptr" else 1.0
        t.w, t.want_h, t.want_h2 = sc.step(t.w, g, t.want_h, t.want_h2, **dict(hyper, rate=rate, diff_scale=scale))
        kw = dict(hyper, rate=rate)
        if variant == "compact":
            diff = g.copy()
            t.plan.solver_step_cpu(diff, t.h, t.h2, **kw)
            assert sc.bits_equal(diff, g)
        elif variant == "scaled_cleared_rate_ptr":
            diff = g.copy()
            rate_cell[0] = rate
            t.plan.solver_step_cpu(diff, t.h, t.h2, **dict(kw, rate=123.0, rate_dev=rate_cell, diff_scale=scale, clear_diff=1))
            assert sc.bits_equal(diff, np.zeros(n, dt))          # +0 everywhere, -0.0 gradients included
        else:
            diff, dense_w = t.dense(g, np.nan), np.full(t.shape, np.nan, dt)
            clear = k % 2
            t.plan.solver_step_cpu(diff, t.h, t.h2, dense_w=dense_w, **dict(kw, diff_is_dense=1, clear_diff=clear))
            assert sc.bits_equal(diff, t.dense(np.zeros(n, dt) if clear else g, np.nan))
            assert sc.bits_equal(dense_w, t.dense(t.w, np.nan))
        t.check(k)
    assert t.plan.stat("update_count") == 4      # (the constructor's update_values_cpu and three steps)
    t.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["float", "double"])
@pytest.mark.parametrize("reg", ["none", "L2", "L1"])
@pytest.mark.parametrize("rule", ["sgd", "nesterov", "adam"])
def test_array_step_cpu(pkg, rule, reg, dt):
    for n in (1, 255, 257):
        w = sc.seeded_values(n, 1, dt)
        h, h2 = np.zeros(n, dt), (np.zeros(n, dt) if rule == "adam" else None)
        data, hh, hh2 = w.copy(), h.copy(), None if h2 is None else h2.copy()
        for k in range(3):
            g = sc.seeded_values(n, 20 + k, dt)
            hyper = dict(HYPER, type=sc.RULES[rule], regularization=sc.REGS[reg], diff_scale=SCALE if k == 1 else 1.0)
            w, h, h2 = sc.step(w, g, h, h2, **hyper)
            diff = g.copy()
            pkg.solver_array_step_cpu(data, diff, hh, hh2, clear_diff=int(k == 2), diff_is_dense=1, **hyper)
            assert sc.bits_equal(data, w) and sc.bits_equal(hh, h) and (h2 is None or sc.bits_equal(hh2, h2)), (n, k)
            assert sc.bits_equal(diff, np.zeros(n, dt) if k == 2 else g)


def test_solver_step_errors(pkg):
    L = pkg.lib()
    d = pkg.ConvDesc(1, 2, 5, 5, 2, 3, 3, 1, 1, 1, 1, 1, 1, 1, 0, 0)
    w = np.zeros((2, 2, 3, 3), np.float32)
    w[0, 0, 1, 1] = 1.0
    w[1, 1, 0, 2] = -2.0
    plan = pkg.Plan(d)
    a32, a64 = np.zeros(2, np.float32), np.zeros(2, np.float64)
    p32, p64 = a32.ctypes.data_as(C.c_void_p), a64.ctypes.data_as(C.c_void_p)
    sgd, adam = pkg.SolverDesc.make(type="sgd", rate=0.1), pkg.SolverDesc.make(type="adam", rate=0.1)
    EINVAL, ESTATE, ENODEVICE = -1, -4, -5
    assert L.escoin_solver_step_cpu(plan._h, C.byref(sgd), p32, p32, None, None) == ESTATE       # before an align
    plan.weight_align_cpu(w)
    assert L.escoin_solver_step_cpu(plan._h, None, p32, p32, None, None) == EINVAL
    assert L.escoin_solver_step_cpu(plan._h, C.byref(sgd), None, p32, None, None) == EINVAL
    assert L.escoin_solver_step_cpu(plan._h, C.byref(sgd), p32, None, None, None) == EINVAL
    assert L.escoin_solver_step_cpu(None, C.byref(sgd), p32, p32, None, None) == EINVAL
    assert L.escoin_solver_step_cpu(plan._h, C.byref(adam), p32, p32, None, None) == EINVAL      # Adam without history2
    assert "history2" in L.escoin_last_error().decode()
    assert L.escoin_solver_step_cpu(plan._h, C.byref(pkg.SolverDesc.make(type=3)), p32, p32, None, None) == EINVAL
    assert L.escoin_solver_step_cpu(plan._h, C.byref(pkg.SolverDesc.make(regularization=3)), p32, p32, None, None) == EINVAL
    assert L.escoin_solver_step_cpu_f64(plan._h, C.byref(sgd), p64, p64, None, None) == ESTATE   # the other Dtype
    assert plan.stat("update_count") == 0
    assert L.escoin_solver_step_cpu(plan._h, C.byref(sgd), p32, p32, None, None) == 0
    assert plan.stat("update_count") == 1
    for fn in (L.escoin_solver_array_step_cpu, L.escoin_solver_array_step):
        extra = (None,) if fn is L.escoin_solver_array_step else ()
        assert fn(None, 2, p32, p32, p32, None, *extra) == EINVAL
        assert fn(C.byref(sgd), 2, None, p32, p32, None, *extra) == EINVAL
        assert fn(C.byref(sgd), 2, p32, None, p32, None, *extra) == EINVAL
        assert fn(C.byref(sgd), 2, p32, p32, None, None, *extra) == EINVAL
        assert fn(C.byref(sgd), -1, p32, p32, p32, None, *extra) == EINVAL
        assert fn(C.byref(adam), 2, p32, p32, p32, None, *extra) == EINVAL
    assert L.escoin_solver_array_step_cpu(C.byref(sgd), 0, p32, p32, p32, None) == 0
    # the device entry points: bad arguments are refused first; without a device they say so and compute nothing
    assert L.escoin_solver_step(plan._h, None, p32, p32, None, None, None) == EINVAL
    assert L.escoin_solver_step(plan._h, C.byref(sgd), None, p32, None, None, None) == EINVAL
    assert L.escoin_solver_step(plan._h, C.byref(adam), p32, p32, None, None, None) == EINVAL
    if pkg.device_count() == 0:
        assert L.escoin_solver_step(plan._h, C.byref(sgd), p32, p32, None, None, None) == ENODEVICE
        assert "no HIP device" in L.escoin_last_error().decode()
        assert L.escoin_solver_step_f64(plan._h, C.byref(sgd), p64, p64, None, None, None) == ENODEVICE
        assert L.escoin_solver_array_step(C.byref(sgd), 2, p32, p32, p32, None, None) == ENODEVICE
        assert L.escoin_solver_array_step_f64(C.byref(sgd), 2, p64, p64, p64, None, None) == ENODEVICE
    else:
        assert L.escoin_solver_step(plan._h, C.byref(sgd), p32, p32, None, None, None) == ESTATE   # a CPU-aligned plan has no device side
    assert plan.stat("update_count") == 1 and plan.workspace_bytes == 0
    plan.close()


def test_a_layer_without_nonzeros_steps_to_nothing(pkg):
    d = pkg.ConvDesc(1, 2, 5, 5, 2, 3, 3, 1, 1, 1, 1, 1, 1, 1, 0, 0)
    plan = pkg.Plan(d)
    plan.weight_align_cpu(np.zeros((2, 2, 3, 3), np.float32))
    one = np.ones(1, np.float32)
    assert pkg.lib().escoin_solver_step_cpu(plan._h, C.byref(pkg.SolverDesc.make(rate=0.1)), one.ctypes.data_as(C.c_void_p),
                                            one.ctypes.data_as(C.c_void_p), None, None) == 0
    assert one[0] == 1.0 and plan.nnz() == 0
    plan.close()
