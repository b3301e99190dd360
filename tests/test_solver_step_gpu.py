"""escoin_solver_step on the MI355X: the solver's rule and the in-place weight update in one launch.  Two yardsticks, both
bit equality: the values and histories against solver_common.step (numpy, op by op in the case's dtype), and the plan's
forward / data gradient against a fresh plan aligned (set_csr) on the new values at the old pattern.  The oracle is
consulted once per case on the forward (<= 1e-4).  A device result that differs from the restatement is a finding about
rounding on the device, not a reason for a tolerance."""
import ctypes as C

import numpy as np
import pytest

import solver_common as sc
from conftest import rel_err
from plan_model import positions
from test_update_values_gpu import Layer, _mixed_weights, _oracle_forward, _seeded
from upd_common import new_weights, values_at

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
TOL = 1e-4
HYPER = dict(rate=0.01, momentum=0.9, momentum2=0.999, delta=1e-8, decay=5e-4)


@pytest.fixture(scope="module")
def dev(pkg):
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        pytest.fail("no HIP device visible (these tests run on the MI355X)")
    return torch.device("cuda:0")


class Stepper(object):
    """A Layer (test_update_values_gpu), its histories on the device and the restatement's copy of values and histories."""

    def __init__(self, layer, rule, reg, layout, explicit_zeros=False, **more):
        self.layer, self.layout = layer, layout
        self.hyper = dict(HYPER, type=sc.RULES[rule], regularization=sc.REGS[reg], **more)
        plan, dev, dt = layer.plan, layer.dev, layer.dt
        if explicit_zeros:
            # a few weights of the pattern become exactly 0, one -0.0 (L1's sign(0) = 0) -- through update_values, so
            # that the first solver step finds an update state without the entry-major view
            w_new, w_nan = new_weights(layer.w, 45, mask=layer.mask)
            plan.update_values(torch.from_numpy(w_nan).to(dev))
            layer.w = w_new
        rp, ci, va, ng = plan.get_csr()
        self.pos = positions(plan.desc, rp, ci, ng)
        self.w = va.copy()
        assert sc.bits_equal(self.w, values_at(plan, layer.w)[2])
        n = self.w.size
        self.h, self.want_h = torch.zeros(n, dtype=layer.xd.dtype, device=dev), np.zeros(n, dt)
        adam = sc.RULES[rule] == sc.ADAM
        self.h2, self.want_h2 = (torch.zeros(n, dtype=layer.xd.dtype, device=dev), np.zeros(n, dt)) if adam else (None, None)

    def dense(self, compact, fill):
        out = np.full(self.layer.w.size, fill, self.layer.dt)
        out[self.pos] = compact
        return out.reshape(self.layer.w.shape)

    def step(self, seed, fast=1):
        """One solver step with a seeded gradient; values and histories are held against the restatement."""
        layer, dev, dt, n = self.layer, self.layer.dev, self.layer.dt, self.w.size
        g = sc.seeded_values(n, seed, dt)
        self.w, self.want_h, self.want_h2 = sc.step(self.w, g, self.want_h, self.want_h2, **self.hyper)
        if self.layout == "dense":
            diff = torch.from_numpy(self.dense(g, np.nan)).to(dev)
            dense_w = torch.full(layer.w.shape, float("nan"), dtype=diff.dtype, device=dev)
            layer.plan.solver_step(diff, self.h, self.h2, dense_w=dense_w, diff_is_dense=1, clear_diff=1, **self.hyper)
        else:
            diff, dense_w = torch.from_numpy(g).to(dev), None
            layer.plan.solver_step(diff, self.h, self.h2, **self.hyper)
        assert layer.plan.stat("update_fast") == fast
        torch.cuda.synchronize()
        if self.layout == "dense":
            assert sc.bits_equal(diff.cpu().numpy(), self.dense(np.zeros(n, dt), np.nan))
            assert sc.bits_equal(dense_w.cpu().numpy(), self.dense(self.w, np.nan))
        else:
            assert sc.bits_equal(diff.cpu().numpy(), g)
        got_h = self.h.cpu().numpy()
        if not sc.bits_equal(got_h, self.want_h):
            bad = np.flatnonzero(got_h != self.want_h)
            print("history differs at %d of %d entries, first: got %r want %r" % (bad.size, n, got_h[bad[:1]], self.want_h[bad[:1]]))
        assert sc.bits_equal(got_h, self.want_h)
        assert self.h2 is None or sc.bits_equal(self.h2.cpu().numpy(), self.want_h2)
        va = layer.plan.get_csr()[2]
        if not sc.bits_equal(va, self.w):
            bad = np.flatnonzero(va != self.w)
            print("values differ at %d of %d entries, first: got %r want %r" % (bad.size, n, va[bad[:1]], self.w[bad[:1]]))
        assert sc.bits_equal(va, self.w)
        layer.w = self.dense(self.w, 0)

    def compare_with_fresh(self, oracle=None, td=None):
        """The forward (and with td the data gradient) against a fresh set_csr plan on the current values."""
        layer = self.layer
        ref = layer.fresh(layer.w)
        assert ref.kernel_name == layer.plan.kernel_name and ref.tiling_info == layer.plan.tiling_info
        got = layer.forward()
        assert np.array_equal(got, layer.forward(ref)), (layer.s.name, layer.plan.kernel_name)
        if oracle is not None:
            err = rel_err(got, _oracle_forward(oracle, layer.s, layer.x, layer.w, layer.b, layer.relu, layer.dt))
            print("%s via %s: vs fresh plan equal, vs oracle rel_err=%.3g" % (layer.s.name, layer.plan.kernel_name, err))
            assert err <= (1e-12 if layer.dt == np.float64 else TOL)
        if td is not None:
            a, b = _data_gradient(layer, layer.plan, td), _data_gradient(layer, ref, td)
            assert np.array_equal(a, b)
        ref.close()


def _data_gradient(layer, plan, td):
    bd, _, _ = plan.backward(td, bottom=layer.xd)
    torch.cuda.synchronize()
    return bd.cpu().numpy()


def _kinds(pkg, synth):
    """id -> (shape, Layer options, check(plan), rule, regularization, layout of diff, explicit zeros first, backward first)"""
    K = pkg
    res5 = synth.resnet50_3x3(N=2)[3]
    res4 = synth.resnet50_3x3(N=2)[2]
    goog = synth.shape("goog14", 3, 480, 14, 14, 192, 1, sparsity=0.95)
    grouped = synth.shape("mixed_g2", 2, 64, 14, 14, 64, 3, pad=1, group=2, sparsity=0.7)
    strided = synth.shape("s2", 2, 16, 15, 15, 24, 3, pad=1, stride=2, sparsity=0.8)
    stat = lambda key, val: (lambda p: p.stat(key) == val)
    return {
        "generic": (synth.lenet_conv2(N=2)[0], dict(kernel=K.KERNEL_GENERIC), stat("kernel_choice", K.KERNEL_GENERIC), "sgd", "L2", "compact", True, False),
        "jit_lines_3x3": (res5, dict(kernel=K.KERNEL_JIT, tiling_batch=256),
                          lambda p: p.stat("kernel_choice") == K.KERNEL_JIT and p.stat("code_direct") == 1 and "jit" in p.kernel_name,
                          "adam", "none", "dense", False, False),
        "jit_literals_1x1": (goog, dict(kernel=K.KERNEL_JIT, tiling_batch=256),
                             lambda p: p.stat("kernel_choice") == K.KERNEL_JIT and p.stat("code_direct") == 1, "nesterov", "L1", "compact", True, False),
        "dense": (res4, dict(kernel=K.KERNEL_DENSE), stat("kernel_choice", K.KERNEL_DENSE), "adam", "L2", "compact", False, False),
        "mixed_groups": (grouped, dict(dense_threshold_pct=30, tiling_batch=256, w="mixed"),
                         lambda p: " + " in p.kernel_name and p.stat("kernel_choice") == K.KERNEL_JIT, "sgd", "L1", "dense", True, False),
        "double": (synth.alexnet(N=2)[1], dict(dt=np.float64), lambda p: p.stat("is_f64") == 1 and "f64" in p.kernel_name,
                   "adam", "L2", "dense", True, False),
        "bwd_transposed_jit": (res5, dict(kernel=K.KERNEL_JIT, backward_kernel=K.KERNEL_JIT, tiling_batch=256),
                               lambda p: p.stat("bwd_data_kernel") == K.KERNEL_JIT, "nesterov", "L2", "compact", False, True),
        "bwd_gather_strided": (strided, dict(), lambda p: p.stat("bwd_data_kernel") == K.KERNEL_GENERIC, "adam", "L1", "dense", True, True),
    }


KIND_IDS = ["generic", "jit_lines_3x3", "jit_literals_1x1", "dense", "mixed_groups", "double", "bwd_transposed_jit", "bwd_gather_strided"]


@pytest.mark.parametrize("kind", KIND_IDS)
def test_solver_step_equals_the_restatement_and_a_fresh_plan(pkg, dev, synth, oracle, kind):
    """One case per plan kind, each asserted to BE that kind and to take the in-place path.  A forward (and for the
    backward kinds a backward) runs first; two steps, because the first builds the entry-major view."""
    s, opts, check, rule, reg, layout, zeros, bwd = _kinds(pkg, synth)[kind]
    opts = dict(opts)
    if opts.get("w") == "mixed":
        opts["w"] = _mixed_weights(s, 5)
    layer = Layer(pkg, dev, synth, s, 40, **opts)
    layer.forward()
    td = None
    if bwd:
        td = torch.from_numpy(_seeded((s.N, s.M) + tuple(layer.plan.out_hw), 81, layer.dt)).to(dev)
        _data_gradient(layer, layer.plan, td)        # builds the backward state
        assert layer.plan.stat("bwd_device_bytes") > 0
    assert check(layer.plan), (layer.plan.kernel_name, layer.plan.tiling_info)
    st = Stepper(layer, rule, reg, layout, explicit_zeros=zeros, diff_scale=(0.125 if kind == "mixed_groups" else 1.0 / 3.0 if kind == "dense" else 1.0))
    count0, upd0 = layer.plan.stat("update_count"), layer.plan.stat("upd_device_bytes")
    st.step(50)
    assert layer.plan.stat("update_count") == count0 + 1 and layer.plan.stat("upd_device_bytes") > upd0
    st.compare_with_fresh(oracle, td)
    ws1 = layer.plan.workspace_bytes
    st.step(51)
    assert layer.plan.workspace_bytes == ws1 and check(layer.plan)
    st.compare_with_fresh(None, td)
    # a plain update afterwards keeps the view; the next step allocates nothing
    layer.plan.set_values(torch.from_numpy(st.w).to(dev))
    assert layer.plan.workspace_bytes == ws1
    layer.plan.close()


def test_fallback_kinds_step_and_rebuild(pkg, dev, synth, oracle):
    """Code the module loader placed, and a plan restored by the fast import: the kernel writes the value array alone,
    the plan is rebuilt from it (update_fast == 0) and ends with the same bits; the imported plan's next step is in place."""
    s = synth.resnet50_3x3(N=2)[3]
    layer = Layer(pkg, dev, synth, s, 70, kernel=pkg.KERNEL_JIT, tiling_batch=256, code_loader=1)
    assert layer.plan.stat("code_direct") == 0
    layer.forward()
    st = Stepper(layer, "adam", "L2", "dense")
    for k in range(2):
        st.step(71 + k, fast=0)
        st.compare_with_fresh(oracle if k == 0 else None)
    layer.plan.close()

    src = Layer(pkg, dev, synth, s, 75, kernel=pkg.KERNEL_JIT, tiling_batch=256)
    blob = src.plan.export_aligned()
    layer = Layer(pkg, dev, synth, s, 75, kernel=pkg.KERNEL_JIT, tiling_batch=256)
    assert layer.plan.import_aligned(blob) and layer.plan.stat("import_fast") == 1
    layer.forward()
    st = Stepper(layer, "nesterov", "L1", "compact")
    st.step(76, fast=0)
    st.compare_with_fresh(oracle)
    st.step(77, fast=1)
    st.compare_with_fresh()
    layer.plan.close()
    src.plan.close()


def test_training_step_graph_capture_equals_eager_steps(pkg, dev, synth):
    """forward, backward_values and solver_step (Adam, rate through rate_dev, clear_diff) captured into one graph and
    replayed three times with the rate rewritten in between, against three eager steps on a second plan that go through
    the restatement and a host-source set_values."""
    s = synth.resnet50_3x3(N=2)[3]
    w0 = synth.pruned_weights(s, 90)
    x = torch.from_numpy(synth.activations(s, 91)).to(dev)
    rates = [1e-3, 5e-4, 2.5e-4]
    hyper = dict(HYPER, type=sc.ADAM, regularization=sc.REG_L2)
    opts = dict(kernel=pkg.KERNEL_JIT, backward_kernel=pkg.KERNEL_JIT, tiling_batch=256)

    def make():
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s), **opts)
        plan.weight_align(w0)
        oh, ow = plan.out_hw
        n = plan.nnz()
        u = dict(y=torch.zeros((s.N, s.M, oh, ow), device=dev), td=torch.zeros((s.N, s.M, oh, ow), device=dev),
                 bd=torch.zeros((s.N, s.C, s.H, s.W), device=dev), vd=torch.zeros(n, device=dev),
                 m=torch.zeros(n, device=dev), v=torch.zeros(n, device=dev), rate=torch.zeros(1, device=dev))
        return plan, u

    def fwd_bwd(plan, u):          # forward, top_diff = top, backward with the compact weight gradient (+=)
        plan.forward(x, None, u["y"])
        u["td"].copy_(u["y"])
        plan.backward(u["td"], bottom=x, bottom_diff=u["bd"], values_diff=u["vd"])

    def fused(plan, u):
        fwd_bwd(plan, u)
        plan.solver_step(u["vd"], u["m"], u["v"], rate_dev=u["rate"], clear_diff=1, **dict(hyper, rate=77.0))

    # eager: the restatement on the host, then a host-source set_values
    ref, ru = make()
    w = ref.get_csr()[2].copy()
    v0 = w.copy()
    m, v = np.zeros_like(w), np.zeros_like(w)
    ref_tops = []
    for k in range(3):
        fwd_bwd(ref, ru)
        torch.cuda.synchronize()
        ref_tops.append(ru["y"].cpu().numpy())
        w, m, v = sc.step(w, ru["vd"].cpu().numpy(), m, v, **dict(hyper, rate=rates[k]))
        ru["vd"].zero_()
        ref.set_values(w)

    plan, u = make()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        u["rate"].fill_(rates[0])
        fused(plan, u)             # warm-up outside the capture: builds the backward state and the update state
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert plan.stat("update_fast") == 1 and plan.stat("upd_device_bytes") > 0
    assert np.all(u["vd"].cpu().numpy() == 0)

    def restart():
        plan.set_values(torch.from_numpy(v0).to(dev))
        u["m"].zero_()
        u["v"].zero_()
        torch.cuda.synchronize()

    restart()
    ws1 = plan.workspace_bytes
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fused(plan, u)
    assert plan.workspace_bytes == ws1
    restart()
    for k in range(3):
        u["rate"].fill_(rates[k])
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(u["y"].cpu().numpy(), ref_tops[k]), k
    assert plan.workspace_bytes == ws1
    assert sc.bits_equal(u["m"].cpu().numpy(), m) and sc.bits_equal(u["v"].cpu().numpy(), v)
    rp, ci, va, ng = plan.get_csr()
    assert sc.bits_equal(va, w) and not np.array_equal(va, v0)
    fresh = pkg.Plan(pkg.ConvDesc.from_shape(s), **opts)
    fresh.set_csr(rp, ci, w, ng)
    got = plan.get_csr()
    for a, b in zip(got, fresh.get_csr()):
        assert np.array_equal(a, b)
    assert sc.bits_equal(got[2], fresh.get_csr()[2])
    assert plan.export_aligned().tobytes() == fresh.export_aligned().tobytes()
    assert np.array_equal(va, ref.get_csr()[2])
    for p in (plan, ref, fresh):
        p.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["float", "double"])
@pytest.mark.parametrize("rule", ["sgd", "nesterov", "adam"])
def test_array_step_on_the_device(pkg, dev, rule, dt):
    reg = {"sgd": "L1", "nesterov": "L2", "adam": "none"}[rule]
    for n in (1, 255, 257):
        w = sc.seeded_values(n, 1, dt)
        h, h2 = np.zeros(n, dt), (np.zeros(n, dt) if rule == "adam" else None)
        data, hh = torch.from_numpy(w).to(dev), torch.from_numpy(h).to(dev)
        hh2 = None if h2 is None else torch.from_numpy(h2).to(dev)
        for k in range(3):
            g = sc.seeded_values(n, 20 + k, dt)
            hyper = dict(HYPER, type=sc.RULES[rule], regularization=sc.REGS[reg], diff_scale=1.0 / 3.0 if k == 1 else 1.0)
            w, h, h2 = sc.step(w, g, h, h2, **hyper)
            diff = torch.from_numpy(g).to(dev)
            pkg.solver_array_step(data, diff, hh, hh2, clear_diff=int(k == 2), **hyper)
            torch.cuda.synchronize()
            assert sc.bits_equal(data.cpu().numpy(), w) and sc.bits_equal(hh.cpu().numpy(), h), (n, k)
            assert h2 is None or sc.bits_equal(hh2.cpu().numpy(), h2)
            assert sc.bits_equal(diff.cpu().numpy(), np.zeros(n, dt) if k == 2 else g)


def test_solver_step_errors_on_the_device(pkg, dev, synth):
    L = pkg.lib()
    s = synth.lenet_conv2(N=1)[0]
    w = synth.pruned_weights(s, 1)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
    n = int(np.count_nonzero(w))
    t32, t64 = torch.zeros(n, device=dev), torch.zeros(n, device=dev, dtype=torch.float64)
    p32, p64 = C.c_void_p(t32.data_ptr()), C.c_void_p(t64.data_ptr())
    h32 = np.zeros(n, np.float32).ctypes.data_as(C.c_void_p)
    sgd, adam = pkg.SolverDesc.make(type="sgd", rate=0.1), pkg.SolverDesc.make(type="adam", rate=0.1)
    assert L.escoin_solver_step(plan._h, C.byref(sgd), p32, p32, None, None, None) == -4       # before an align
    plan.weight_align(w)
    assert L.escoin_solver_step(plan._h, None, p32, p32, None, None, None) == -1
    assert L.escoin_solver_step(plan._h, C.byref(sgd), None, p32, None, None, None) == -1
    assert L.escoin_solver_step(plan._h, C.byref(sgd), p32, None, None, None, None) == -1
    assert L.escoin_solver_step(plan._h, C.byref(adam), p32, p32, None, None, None) == -1
    assert L.escoin_solver_step(plan._h, C.byref(pkg.SolverDesc.make(type=7)), p32, p32, None, None, None) == -1
    assert L.escoin_solver_step_f64(plan._h, C.byref(sgd), p64, p64, None, None, None) == -4   # the other Dtype's entry point
    assert L.escoin_solver_step_cpu(plan._h, C.byref(sgd), h32, h32, None, None) == -4         # a device-aligned plan
    assert plan.stat("update_count") == 0
    plan.close()
