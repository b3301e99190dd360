"""Plan option "b2s" driven through the op-sequence suite (seq_common.run_sequence, unchanged): an inner-product layer whose
forward, whole backward, updates, solver steps, prunes, rewires, imports and conv_mode flips are compared with
plan_model.PlanModel after every op -- the check that every copy of the weights (the value array, the inner plan's forward
copies, the inner backward state's) is found in every order of calls.  seq_common's tables name convolution layers only, so
the configurations and their inputs are made here, the way seq_common.make_inputs makes its own."""
import time

import numpy as np
import pytest

import errbound as eb
import seq_common as sq
from seq_backends import GpuBackend

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
# 70 images: two inner images under the rule, the second with 6 of its 64 positions used; group 2
LAYER = ("seq_ip", (70, 48, 1, 1, 26, 1), dict(group=2, sparsity=0.6))
CONFIGS = [
    sq.Config("b2s_inner", "IP", dict(b2s=1, kernel="KERNEL_JIT", tiling_batch=4096, backward_kernel="KERNEL_JIT"), True, False, "pruned",
              dict(name=("escoin_b2s_pack_kernel", "jit"), b2s=1, kernel_choice="KERNEL_JIT", bwd_data_kernel="KERNEL_JIT"), {}),
    sq.Config("b2s_inner_dense", "IP", dict(b2s=1, kernel="KERNEL_DENSE", backward_kernel="KERNEL_DENSE", wgrad_kernel="WGRAD_MFMA"), False,
              False, "pruned", dict(name=("escoin_b2s_pack_kernel",), b2s=1, kernel_choice="KERNEL_DENSE", bwd_data_kernel="KERNEL_DENSE",
                                    wgrad_kernel="WGRAD_MFMA"), {}),
    sq.Config("b2s_inner_generic", "IP", dict(b2s=1, kernel="KERNEL_GENERIC", backward_kernel="KERNEL_GENERIC", wgrad_kernel="WGRAD_ENTRY"),
              False, False, "pruned", dict(name=("escoin_b2s_pack_kernel",), b2s=1, bwd_data_kernel="KERNEL_GENERIC", wgrad_kernel="WGRAD_ENTRY"), {}),
]
BY_ID = {c.id: c for c in CONFIGS}
SEEDS = (1, 2)
_INPUTS = {}


@pytest.fixture(scope="module")
def dev(pkg):
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        pytest.fail("no HIP device visible (these tests run on the MI355X)")
    return torch.device("cuda:0")


def _inputs(synth, cfg):
    if cfg.id not in _INPUTS:
        name, dims, kw = LAYER
        s = synth.shape(name, *dims, **kw)
        k = sum(map(ord, cfg.id))
        w = synth.pruned_weights(s, k)
        x, b = synth.activations(s, k + 1), synth.bias_vector(s, k + 2)
        td = np.random.RandomState(k + 3).uniform(-1, 1, (s.N, s.M, 1, 1)).astype(np.float32)
        sk = eb.skew(s, w, x, b, k + 4, top_diff=td)
        c = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)  # noqa: E731
        px = synth.activations(s, k + 5)
        ptd = (np.random.RandomState(k + 6).uniform(-1, 1, td.shape) / 16).astype(np.float32)
        _INPUTS[cfg.id] = sq.Inputs(s, np.float32, c(sk.w), c(sk.x), c(sk.b), c(sk.top_diff), c(px), c(ptd), sk.row_exp)
    return _INPUTS[cfg.id]


def _run(pkg, dev, synth, cfg, hyper, ops, what, check=None):
    inp = _inputs(synth, cfg)
    backend = GpuBackend(pkg, dev, cfg, inp, sq.initial_model(cfg, inp).csr())
    worst, t0 = {}, time.time()
    try:
        drv = sq.run_sequence(backend, cfg, inp, hyper, sq.supported(cfg, ops) + [sq.BWD], seed=what, worst=worst)
        if check:
            check(drv)
        print("\nsequence %s %s: %.2f s; %s" % (cfg.id, what, time.time() - t0, backend.plan.kernel_name))
        for kernel, ratio in sorted(worst.items()):
            print("    %-78s worst err/bound %.3g" % (kernel, ratio))
    finally:
        backend.close()


@pytest.mark.parametrize("cid", [c.id for c in CONFIGS])
def test_each_configuration_runs_the_kernels_it_names(pkg, dev, synth, cid):
    import solver_common as sc
    cfg = BY_ID[cid]
    inp = _inputs(synth, cfg)
    backend = GpuBackend(pkg, dev, cfg, inp, sq.initial_model(cfg, inp).csr())
    try:
        sq.run_sequence(backend, cfg, inp, dict(type=sc.SGD, rate=1e-2), [sq.BWD], seed="kernels", finish=False)
        plan = backend.plan
        for key, want in cfg.expect.items():
            if key == "name":
                assert any(t in plan.kernel_name for t in want), (cid, plan.kernel_name)
            else:
                assert plan.stat(key) == (getattr(pkg, want) if isinstance(want, str) else want), (cid, key, plan.stat(key))
    finally:
        backend.close()


CASES = [(c.id, seed) for c in CONFIGS for seed in SEEDS]


@pytest.mark.parametrize("cid,seed", CASES, ids=["%s-%d" % c for c in CASES])
def test_random_sequences(pkg, dev, synth, cid, seed):
    cfg = BY_ID[cid]
    hyper, ops = sq.generate(cfg, seed)
    _run(pkg, dev, synth, cfg, hyper, ops, "seed %d" % seed)


@pytest.mark.parametrize("cid", [c.id for c in CONFIGS])
def test_host_and_device_sources_alternate_with_a_host_reader_between(pkg, dev, synth, cid):
    """seq_common.SOURCES_AND_READERS: updates from both sources around get_csr, an import, a prune and conv_mode flips, each of
    which tears the inner plan down and builds it anew."""
    import solver_common as sc
    hyper = dict(type=sc.ADAM, regularization=sc.REG_NONE, rate=1e-3, momentum=0.9, momentum2=0.999, delta=1e-8)
    _run(pkg, dev, synth, BY_ID[cid], hyper, sq.SOURCES_AND_READERS, "sources and readers")


@pytest.mark.parametrize("cid", [c.id for c in CONFIGS])
def test_the_update_list_follows_the_inner_backward_state_and_the_solver(pkg, dev, synth, cid):
    """seq_common.list_lifecycle: set_values before the first backward; the backward, which builds the INNER plan's state (the
    outer plan has none); set_values again (the list grows by that state's copy); a solver step and updates from both sources."""
    import solver_common as sc
    seen = {}

    def first(drv):
        seen["n"] = drv.b.stat("update_destinations")
        assert seen["n"] >= 2 * drv.m.nnz > 0 and drv.b.stat("bwd_device_bytes") == 0

    def grown(drv):
        assert drv.b.stat("update_destinations") > seen["n"] and drv.b.stat("bwd_device_bytes") > 0
        seen["grown"] = drv.b.stat("update_destinations")

    def same(drv):
        assert drv.b.stat("update_destinations") == seen["grown"] and drv.b.stat("update_fast") == 1

    hyper = dict(type=sc.SGD, regularization=sc.REG_L2, rate=1e-2, momentum=0.9, decay=1e-3)
    _run(pkg, dev, synth, BY_ID[cid], hyper, sq.list_lifecycle(first, grown, same), "update list")
