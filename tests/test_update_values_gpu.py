"""escoin_update_values / escoin_plan_set_values on the MI355X: new weights at the old pattern, in place.  The reference
point of every comparison is a fresh plan with the same options aligned (set_csr) on the new values at the old pattern,
and the requirement is np.array_equal -- no tolerance.  The oracle is consulted once per case on top (<= 1e-4) so that
"both wrong in the same way" cannot pass.  New weights: every nonzero replaced by a seeded random value, a few of them
exactly 0 and one -0.0; device-source updates read a blob whose positions outside the pattern are NaN."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_err
from seq_common import mixed_weights as _mixed_weights
from upd_common import new_weights, same_bits, values_at

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module")
def dev(pkg):
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        pytest.fail("no HIP device visible (these tests run on the MI355X)")
    return torch.device("cuda:0")


def _seeded(shape, seed, dt=np.float32):
    return np.random.RandomState(seed).uniform(-1, 1, shape).astype(dt)


def _geom(oracle, s):
    return oracle.geom(s.C, s.H, s.W, s.M, s.KH, s.KW, s.pad_h, s.pad_w, s.stride_h, s.stride_w, s.dil_h, s.dil_w, s.group)


def _oracle_forward(oracle, s, x, w, b, relu, dt):
    if dt == np.float64:
        return oracle.conv_forward_f64(_geom(oracle, s), x, w, b, relu=relu)
    return oracle.conv_forward(_geom(oracle, s), x, w, b, relu=relu, gate=False, threads=4)


def _apply(plan, dev, w_nan, vals, source, form):
    """One update: source "device" | "host", form "dense" (update_values on the blob) | "values" (set_values)."""
    a = w_nan if form == "dense" else vals
    if source == "device":
        a = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    (plan.update_values if form == "dense" else plan.set_values)(a)
    return a      # (kept alive by the caller until the stream is synchronised)


class Layer(object):
    """A plan aligned on seeded weights, its inputs on the device, and what a case needs to update and compare."""

    def __init__(self, pkg, dev, synth, s, seed, dt=np.float32, relu=False, w=None, **opts):
        self.pkg, self.dev, self.s, self.dt, self.relu, self.opts = pkg, dev, s, dt, relu, opts
        self.w = (synth.pruned_weights(s, seed) if w is None else w).astype(dt)
        b = synth.bias_vector(s, seed + 1)
        self.b = None if b is None else b.astype(dt)
        self.x = (synth.activations(s, seed + 2) / (3.0 if dt == np.float64 else 1.0)).astype(dt)
        self.mask = self.w != 0          # the pattern: later values may be explicit zeros
        self.desc = pkg.ConvDesc.from_shape(s, fuse_relu=relu)
        self.plan = pkg.Plan(self.desc, **opts)
        self.plan.weight_align(self.w)
        self.xd = torch.from_numpy(self.x).to(dev)
        self.bd = None if self.b is None else torch.from_numpy(self.b).to(dev)

    def forward(self, plan=None):
        top = (plan or self.plan).forward(self.xd, self.bd)
        torch.cuda.synchronize()
        return top.cpu().numpy()

    def fresh(self, w_new, **more):
        """A new plan with the same options, aligned on w_new's values at THIS plan's pattern (explicit zeros kept)."""
        rp, ci, vals, ng = values_at(self.plan, w_new)
        p = self.pkg.Plan(self.desc, **dict(self.opts, **more))
        p.set_csr(rp, ci, vals, ng)
        return p

    def update_and_compare(self, oracle, seed, source, form, fast=1):
        """Updates the plan to new weights and holds its forward against a fresh plan's (bits) and the oracle's."""
        w_new, w_nan = new_weights(self.w, seed, mask=self.mask)
        vals = values_at(self.plan, w_new)[2]
        keep = _apply(self.plan, self.dev, w_nan, vals, source, form)
        assert self.plan.stat("update_fast") == fast, (source, form)
        got = self.forward()
        del keep
        ref = self.fresh(w_new)
        assert ref.kernel_name == self.plan.kernel_name and ref.tiling_info == self.plan.tiling_info
        want = self.forward(ref)
        assert np.array_equal(got, want), (self.s.name, source, form, self.plan.kernel_name)
        err = rel_err(got, _oracle_forward(oracle, self.s, self.x, w_new, self.b, self.relu, self.dt))
        print("%s %s/%s via %s: vs fresh plan equal, vs oracle rel_err=%.3g" % (self.s.name, source, form, self.plan.kernel_name, err))
        assert err <= (1e-12 if self.dt == np.float64 else TOL)
        self.w = w_new
        return ref, w_new


def _kinds(pkg, synth):
    """(id, shape, Layer options, check(plan), source, form): one case per plan kind."""
    K = pkg
    res5 = synth.resnet50_3x3(N=2)[3]
    res4 = synth.resnet50_3x3(N=2)[2]
    goog = synth.shape("goog14", 3, 480, 14, 14, 192, 1, sparsity=0.95)
    half = synth.shape("half_wg", 5, 192, 28, 28, 64, 1, sparsity=0.95)
    grouped = synth.shape("mixed_g2", 2, 64, 14, 14, 64, 3, pad=1, group=2, sparsity=0.7)
    stat = lambda key, val: (lambda p: p.stat(key) == val)
    return [
        ("generic", synth.lenet_conv2(N=2)[0], dict(kernel=K.KERNEL_GENERIC), stat("kernel_choice", K.KERNEL_GENERIC), "device", "dense"),
        ("tiled", res5, dict(kernel=K.KERNEL_TILED, tiling_batch=256), stat("kernel_choice", K.KERNEL_TILED), "device", "values"),
        ("jit_lines_3x3", res5, dict(kernel=K.KERNEL_JIT, tiling_batch=256),
         lambda p: p.stat("kernel_choice") == K.KERNEL_JIT and p.stat("code_direct") == 1 and "jit" in p.kernel_name, "device", "dense"),
        ("jit_literals_1x1", goog, dict(kernel=K.KERNEL_JIT, tiling_batch=256),
         lambda p: p.stat("kernel_choice") == K.KERNEL_JIT and p.stat("code_direct") == 1, "host", "dense"),
        ("jit_half_workgroups", half, dict(tiling_batch=256),
         lambda p: p.stat("kernel_choice") == K.KERNEL_JIT and "oc_waves=4 pix_waves=1" in p.tiling_info, "device", "dense"),
        ("dense", res4, dict(kernel=K.KERNEL_DENSE), stat("kernel_choice", K.KERNEL_DENSE), "host", "values"),
        ("mixed_groups", grouped, dict(dense_threshold_pct=30, tiling_batch=256, w="mixed"),
         lambda p: " + " in p.kernel_name and p.stat("kernel_choice") == K.KERNEL_JIT, "device", "dense"),
        ("lowered_gemm", res4, dict(conv_mode=K.CONV_MODE_LOWERED_GEMM), stat("kernel_choice", K.KERNEL_DENSE), "device", "values"),
        ("lowered_sparse", res5, dict(conv_mode=K.CONV_MODE_LOWERED_SPARSE, tiling_batch=256),
         lambda p: "lowered" in p.kernel_name or "csrmm" in p.kernel_name, "device", "dense"),
        ("sub_batch_launches", synth.resnet50_3x3(N=6)[3], dict(kernel=K.KERNEL_JIT, tiling_batch=256, max_launch_bytes=2 * 512 * 49 * 4),
         stat("kernel_choice", K.KERNEL_JIT), "host", "dense"),
        ("fuse_relu", synth.shape("relu3x3", 2, 16, 12, 12, 24, 3, pad=1, sparsity=0.7), dict(relu=True, tiling_batch=256),
         stat("kernel_choice", K.KERNEL_JIT), "device", "dense"),
        ("double", synth.alexnet(N=2)[1], dict(dt=np.float64), lambda p: p.stat("is_f64") == 1 and "f64" in p.kernel_name, "device", "dense"),
        ("double_host_values", synth.lenet_conv2(N=2)[0], dict(dt=np.float64), stat("is_f64", 1), "host", "values"),
    ]


KIND_IDS = ["generic", "tiled", "jit_lines_3x3", "jit_literals_1x1", "jit_half_workgroups", "dense", "mixed_groups", "lowered_gemm",
            "lowered_sparse", "sub_batch_launches", "fuse_relu", "double", "double_host_values"]


@pytest.mark.parametrize("kind", KIND_IDS)
def test_update_in_place_equals_a_fresh_plan(pkg, dev, synth, oracle, kind):
    """One case per plan kind, each asserted to BE that kind and to take the in-place path; a forward runs before the
    update (the caches then hold the old code and weights), the first update and a second one are both compared."""
    name, s, opts, check, source, form = [k for k in _kinds(pkg, synth) if k[0] == kind][0]
    opts = dict(opts)
    if opts.get("w") == "mixed":
        opts["w"] = _mixed_weights(s, 5)
    layer = Layer(pkg, dev, synth, s, 40, **opts)
    assert check(layer.plan), (layer.plan.kernel_name, layer.plan.tiling_info)
    assert layer.plan.stat("upd_device_bytes") == 0 and layer.plan.stat("update_count") == 0
    layer.forward()
    ws0 = layer.plan.workspace_bytes       # (after the forward: the lowering comparator grows its column buffer there)
    ref, _ = layer.update_and_compare(oracle, 50, source, form)
    ref.close()
    assert layer.plan.stat("update_destinations") >= layer.plan.nnz() > 0
    assert layer.plan.workspace_bytes == ws0 + layer.plan.stat("upd_device_bytes") and layer.plan.stat("upd_device_bytes") > 0
    ws1 = layer.plan.workspace_bytes
    # the other source and the other form on the same plan, then the update state is what it was
    ref, _ = layer.update_and_compare(oracle, 51, "host" if source == "device" else "device", "values" if form == "dense" else "dense")
    ref.close()
    assert layer.plan.workspace_bytes == ws1 and layer.plan.stat("update_count") == 2 and check(layer.plan)
    layer.plan.close()


def test_conv_mode_flip_after_a_device_source_update_sees_the_new_values(pkg, dev, synth, oracle):
    """The rebuild a flip to LOWERED_GEMM (and back) does reads the host CSR: after a device-source update the values must
    have come back first.  LOWERED_SPARSE in between reads the updated value array."""
    s = synth.resnet50_3x3(N=2)[3]
    layer = Layer(pkg, dev, synth, s, 60, kernel=pkg.KERNEL_AUTO, tiling_batch=256)
    layer.forward()
    ref, w_new = layer.update_and_compare(oracle, 61, "device", "dense")
    want = _oracle_forward(oracle, s, layer.x, w_new, layer.b, False, np.float32)
    for mode in (pkg.CONV_MODE_LOWERED_SPARSE, pkg.CONV_MODE_LOWERED_GEMM, pkg.CONV_MODE_SCONV):
        layer.plan.set_option("conv_mode", mode)
        ref.set_option("conv_mode", mode)
        assert layer.plan.kernel_name == ref.kernel_name
        got = layer.forward()
        assert np.array_equal(got, layer.forward(ref)), mode
        assert rel_err(got, want) <= TOL
    # ... and the rebuilt plan updates in place again
    ref.close()
    ref, _ = layer.update_and_compare(oracle, 62, "device", "values")
    ref.close()
    layer.plan.close()


def test_fallback_kinds_rebuild_and_say_so(pkg, dev, synth, oracle):
    """Code the HIP module loader placed, and a plan restored by the fast import (code without a value map): the update
    rebuilds the device side (update_fast == 0); the imported plan's rebuild produces the map, its second update is fast."""
    s = synth.resnet50_3x3(N=2)[3]
    layer = Layer(pkg, dev, synth, s, 70, kernel=pkg.KERNEL_JIT, tiling_batch=256, code_loader=1)
    assert layer.plan.stat("code_direct") == 0
    layer.forward()
    for k, (source, form) in enumerate([("device", "dense"), ("host", "values")]):
        ref, _ = layer.update_and_compare(oracle, 71 + k, source, form, fast=0)
        ref.close()
    layer.plan.close()

    src = Layer(pkg, dev, synth, s, 75, kernel=pkg.KERNEL_JIT, tiling_batch=256)
    blob = src.plan.export_aligned()
    layer = Layer(pkg, dev, synth, s, 75, kernel=pkg.KERNEL_JIT, tiling_batch=256)
    assert layer.plan.import_aligned(blob) and layer.plan.stat("import_fast") == 1
    layer.forward()
    ref, _ = layer.update_and_compare(oracle, 76, "device", "dense", fast=0)
    ref.close()
    ref, _ = layer.update_and_compare(oracle, 77, "device", "dense", fast=1)
    ref.close()
    layer.plan.close()
    src.plan.close()


def _backward(layer, plan, td):
    bd, wd, _ = plan.backward(td, bottom=layer.xd, top=None, weight_diff=True)
    torch.cuda.synchronize()
    return bd.cpu().numpy(), wd.cpu().numpy()


@pytest.mark.parametrize("kind", ["transposed_jit", "transposed_dense", "gather_strided", "gather_double"])
def test_backward_after_update_equals_a_fresh_plan(pkg, dev, synth, oracle, kind):
    """The data gradient reads the backward state's own copies of the weights (the transposed plan's code / matrix, or
    the gather kernel's value array): updated in place, the state itself kept."""
    s, opts, want_kernel = {
        "transposed_jit": (synth.resnet50_3x3(N=2)[3], dict(backward_kernel=pkg.KERNEL_JIT, tiling_batch=256), pkg.KERNEL_JIT),
        "transposed_dense": (synth.resnet50_3x3(N=2)[2], dict(backward_kernel=pkg.KERNEL_DENSE), pkg.KERNEL_DENSE),
        "gather_strided": (synth.shape("s2", 2, 16, 15, 15, 24, 3, pad=1, stride=2, sparsity=0.8), dict(), pkg.KERNEL_GENERIC),
        "gather_double": (synth.shape("d64", 2, 12, 9, 9, 16, 3, pad=1, sparsity=0.7), dict(dt=np.float64), pkg.KERNEL_GENERIC),
    }[kind]
    layer = Layer(pkg, dev, synth, s, 80, **opts)
    td = torch.from_numpy(_seeded((s.N, s.M) + tuple(layer.plan.out_hw), 81, layer.dt)).to(dev)
    _backward(layer, layer.plan, td)                       # builds the backward state
    assert layer.plan.stat("bwd_data_kernel") == want_kernel
    us, nbytes = layer.plan.stat("bwd_align_us"), layer.plan.stat("bwd_device_bytes")
    assert nbytes > 0
    ref, _ = layer.update_and_compare(oracle, 82, "device", "dense")
    assert layer.plan.stat("bwd_align_us") == us and layer.plan.stat("bwd_device_bytes") == nbytes
    got, want = _backward(layer, layer.plan, td), _backward(layer, ref, td)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert layer.plan.stat("bwd_align_us") == us and layer.plan.stat("bwd_data_kernel") == want_kernel
    ref.close()
    # a host-source update reaches the backward state as well
    ref, _ = layer.update_and_compare(oracle, 83, "host", "values")
    got, want = _backward(layer, layer.plan, td), _backward(layer, ref, td)
    assert np.array_equal(got[0], want[0])
    ref.close()
    layer.plan.close()

    # a backward state first built AFTER a device-source update is built from the new values; the next update covers it
    layer = Layer(pkg, dev, synth, s, 84, **opts)
    layer.forward()
    ref, _ = layer.update_and_compare(oracle, 85, "device", "dense")
    n_dst = layer.plan.stat("update_destinations")
    got, want = _backward(layer, layer.plan, td), _backward(layer, ref, td)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    ref.close()
    ref, _ = layer.update_and_compare(oracle, 86, "device", "values")
    assert layer.plan.stat("update_destinations") > n_dst
    got, want = _backward(layer, layer.plan, td), _backward(layer, ref, td)
    assert np.array_equal(got[0], want[0])
    ref.close()
    layer.plan.close()


def test_training_step_graph_capture_equals_eager_realign(pkg, dev, synth):
    """forward + backward + an SGD step on the blob + update_values captured into one graph (single stream), replayed
    three times, against three eager steps that re-align: outputs and final weights equal, pruned positions exactly 0.
    The update state is allocated by the first update and by no later one."""
    s = synth.resnet50_3x3(N=2)[3]
    w0 = synth.pruned_weights(s, 90)
    x = torch.from_numpy(synth.activations(s, 91)).to(dev)
    lr = 1e-3

    def make():
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s), kernel=pkg.KERNEL_JIT, backward_kernel=pkg.KERNEL_JIT, tiling_batch=256)
        plan.weight_align(w0)
        oh, ow = plan.out_hw
        u = dict(W=torch.from_numpy(w0).to(dev), y=torch.zeros((s.N, s.M, oh, ow), device=dev),
                 td=torch.zeros((s.N, s.M, oh, ow), device=dev), bd=torch.zeros((s.N, s.C, s.H, s.W), device=dev),
                 wd=torch.zeros((s.M, s.C // s.group, s.KH, s.KW), device=dev))
        return plan, u

    def compute(plan, u):          # forward, top_diff = top, ClearParamDiffs, backward, SGD
        plan.forward(x, None, u["y"])
        u["td"].copy_(u["y"])
        u["wd"].zero_()
        plan.backward(u["td"], bottom=x, bottom_diff=u["bd"], weight_diff=u["wd"])
        u["W"].add_(u["wd"], alpha=-lr)

    # eager reference: re-align after every step
    ref, ru = make()
    ref_tops = []
    for _ in range(3):
        compute(ref, ru)
        ref.weight_align(ru["W"])
        torch.cuda.synchronize()
        ref_tops.append(ru["y"].cpu().numpy())
    nnz0 = ref.nnz()

    plan, u = make()
    ws0 = plan.workspace_bytes
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        compute(plan, u)           # warm-up outside the capture: builds the backward state ...
        plan.update_values(u["W"])     # ... and the update state
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ws1 = plan.workspace_bytes
    assert plan.stat("update_fast") == 1
    assert ws1 == ws0 + plan.stat("bwd_device_bytes") + plan.stat("upd_device_bytes") and plan.stat("upd_device_bytes") > 0
    u["W"].copy_(torch.from_numpy(w0))
    plan.update_values(u["W"])         # back to the start; allocates nothing
    torch.cuda.synchronize()
    assert plan.workspace_bytes == ws1
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        compute(plan, u)
        plan.update_values(u["W"])
    assert plan.workspace_bytes == ws1
    u["W"].copy_(torch.from_numpy(w0))
    plan.update_values(u["W"])
    torch.cuda.synchronize()
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(u["y"].cpu().numpy(), ref_tops[k]), k
    w_graph, w_eager = u["W"].cpu().numpy(), ru["W"].cpu().numpy()
    assert np.array_equal(w_graph, w_eager)
    assert np.all(w_graph[w0 == 0] == 0) and not np.array_equal(w_graph, w0)
    assert plan.workspace_bytes == ws1
    # host mirrors after the replays: the device is authoritative, get_csr reads the values back
    rp, ci, va, ng = plan.get_csr()
    assert same_bits(va, values_at(plan, w_graph)[2]) and plan.nnz() == nnz0
    assert np.array_equal(va, ref.get_csr()[2])
    plan.close()
    ref.close()


def test_host_mirrors_follow_device_source_updates(pkg, dev, synth, oracle):
    """After device-source updates get_csr returns the blob's values at the pattern (explicit zeros included), the CPU
    entry points compute with them, and export_aligned -> import_aligned into a new plan reproduces the forward."""
    s = synth.resnet50_3x3(N=2)[3]
    layer = Layer(pkg, dev, synth, s, 100, kernel=pkg.KERNEL_JIT, tiling_batch=256)
    rp0, ci0, _, ng0 = layer.plan.get_csr()
    ref, w_new = layer.update_and_compare(oracle, 101, "device", "dense")
    rp, ci, va, ng = layer.plan.get_csr()
    assert np.array_equal(rp, rp0) and np.array_equal(ci, ci0) and np.array_equal(ng, ng0)
    assert same_bits(va, values_at(layer.plan, w_new)[2]) and np.count_nonzero(va == 0) >= 4 and np.any(np.signbit(va) & (va == 0))
    assert np.array_equal(layer.plan.forward_cpu(layer.x, layer.b, n_threads=4), ref.forward_cpu(layer.x, layer.b, n_threads=4))
    blob = layer.plan.export_aligned()
    assert blob.tobytes() == ref.export_aligned().tobytes()          # code section and content tags carry the new values
    other = pkg.Plan(layer.desc, kernel=pkg.KERNEL_JIT, tiling_batch=256)
    assert other.import_aligned(blob)
    assert np.array_equal(layer.forward(other), layer.forward())
    other.close()
    ref.close()
    # a second device-source update after the read-back, then the host CPU backward
    ref, w_new = layer.update_and_compare(oracle, 102, "device", "values")
    td = _seeded((s.N, s.M) + tuple(layer.plan.out_hw), 103)
    a = layer.plan.backward_cpu(td, bottom=layer.x, weight_diff=True, n_threads=4)
    b = ref.backward_cpu(td, bottom=layer.x, weight_diff=True, n_threads=4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    ref.close()
    layer.plan.close()


def test_code_address_reuse_with_an_update_in_between(pkg, dev, synth, oracle):
    """The pattern of test_code_address_reuse_runs_the_new_code with an update in between: destroy, new plan (the
    allocator hands the same code range back), update, forward -- against the oracle every round."""
    for s in (synth.shape("r14", 40, 40, 14, 14, 96, 1, sparsity=0.95, group=2),
              synth.shape("r7k3", 24, 64, 7, 7, 64, 3, pad=1, sparsity=0.9, bias=False)):
        for it in range(4):
            layer = Layer(pkg, dev, synth, s, 200 + 3 * it, kernel=pkg.KERNEL_JIT, tiling_batch=256)
            assert layer.plan.stat("code_direct") == 1
            if it % 2 == 0:
                layer.forward()            # (odd rounds: the first launch of this plan already runs patched code)
            w_new, w_nan = new_weights(layer.w, 300 + it, mask=layer.mask)
            keep = _apply(layer.plan, dev, w_nan, None, "device", "dense")
            assert layer.plan.stat("update_fast") == 1
            want = _oracle_forward(oracle, s, layer.x, w_new, layer.b, False, np.float32)
            for n in (s.N, 3):
                got = layer.plan.forward(layer.xd[:n].contiguous(), layer.bd).cpu().numpy()
                assert rel_err(got, want[:n]) <= TOL, (s.name, it, n)
            del keep
            layer.plan.close()


def test_update_errors_on_the_device(pkg, dev, synth):
    L = pkg.lib()
    s = synth.lenet_conv2(N=1)[0]
    w = synth.pruned_weights(s, 1)
    p32, p64 = w.ctypes.data_as(C.c_void_p), w.astype(np.float64).ctypes.data_as(C.c_void_p)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
    assert L.escoin_update_values(plan._h, p32, 0, None) == -4           # before an align
    plan.weight_align(w)
    assert L.escoin_update_values(plan._h, None, 0, None) == -1
    assert L.escoin_update_values_f64(plan._h, p64, 0, None) == -4       # the other Dtype's entry point
    assert L.escoin_plan_set_values_f64(plan._h, p64, 0, None) == -4
    assert L.escoin_update_values_cpu(plan._h, p32) == -4                # a device-aligned plan: the GPU entry point updates both
    assert "w_on_device = 0" in L.escoin_last_error().decode()
    assert L.escoin_update_values(plan._h, p32, 0, None) == 0
    plan.weight_align_cpu(w)                                             # host only again
    assert L.escoin_update_values(plan._h, p32, 0, None) == -4
    assert L.escoin_update_values_cpu(plan._h, p32) == 0
    plan.close()
