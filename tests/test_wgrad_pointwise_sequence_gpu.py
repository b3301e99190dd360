"""Plan option "wgrad_pointwise" driven through the op-sequence suite (seq_common.run_sequence, unchanged): a pointwise layer
of pw_straddle's size whose forward, whole backward, updates, solver steps, prunes, rewires, imports and conv_mode flips are
compared with plan_model.PlanModel after every op -- the check that the pointwise kernel's tables follow the pattern through
every order of calls.  seq_common's tables hold no layer of this size, so the configuration and its inputs are made here,
the way seq_common.make_inputs makes its own."""
import time

import numpy as np
import pytest

import errbound as eb
import seq_common as sq
import wgrad_pointwise_common as pc
from seq_backends import GpuBackend

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
LAYER = ("seq_pw",) + pc.CONV["pw_straddle"]       # name, six dimensions, synth.shape's keywords
CONFIGS = [
    sq.Config("pw_wgrad", "PW", dict(wgrad_pointwise=1), False, False, "pruned", dict(wgrad_kernel="WGRAD_POINTWISE"), {}),
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
        s = synth.shape(LAYER[0], *LAYER[1:7], **LAYER[7])
        k = sum(map(ord, cfg.id))
        w = synth.pruned_weights(s, k)
        x, b = synth.activations(s, k + 1), synth.bias_vector(s, k + 2)
        td = np.random.RandomState(k + 3).uniform(-1, 1, (s.N, s.M) + synth.out_hw(s)).astype(np.float32)
        sk = eb.skew(s, w, x, b, k + 4, top_diff=td)
        c = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)  # noqa: E731
        px = synth.activations(s, k + 5)
        ptd = (np.random.RandomState(k + 6).uniform(-1, 1, td.shape) / 16).astype(np.float32)
        _INPUTS[cfg.id] = sq.Inputs(s, np.float32, c(sk.w), c(sk.x), c(sk.b), c(sk.top_diff), c(px), c(ptd), sk.row_exp)
    return _INPUTS[cfg.id]


def _run(pkg, dev, synth, cfg, hyper, ops, what):
    inp = _inputs(synth, cfg)
    backend = GpuBackend(pkg, dev, cfg, inp, sq.initial_model(cfg, inp).csr())
    worst, t0 = {}, time.time()
    try:
        sq.run_sequence(backend, cfg, inp, hyper, sq.supported(cfg, ops) + [sq.BWD], seed=what, worst=worst)
        # every checked weight / bias gradient of the sequence came from the pointwise kernel (seq_backends labels a
        # gradient with the stat "wgrad_kernel" it read right after the call; "kernel -": an empty plan launched nothing)
        wgrads = [k for k in worst if k.split()[0] in ("values_diff", "weight_diff", "bias_diff")]
        assert wgrads and all(k.endswith("kernel %d" % pkg.WGRAD_POINTWISE) or k.endswith("kernel -") for k in wgrads), wgrads
        assert any(k.endswith("kernel 4") for k in wgrads), wgrads
        print("\nsequence %s %s: %.2f s; %s" % (cfg.id, what, time.time() - t0, backend.plan.kernel_name))
        for kernel, ratio in sorted(worst.items()):
            print("    %-78s worst err/bound %.3g" % (kernel, ratio))
    finally:
        backend.close()


def test_the_configuration_runs_the_pointwise_kernel(pkg, dev, synth):
    import solver_common as sc
    cfg = CONFIGS[0]
    inp = _inputs(synth, cfg)
    backend = GpuBackend(pkg, dev, cfg, inp, sq.initial_model(cfg, inp).csr())
    try:
        sq.run_sequence(backend, cfg, inp, dict(type=sc.SGD, rate=1e-2), [sq.BWD], seed="kernels", finish=False)
        assert backend.plan.stat("wgrad_kernel") == pkg.WGRAD_POINTWISE == 4
        assert 0 < backend.plan.stat("wgrad_lds_bytes") <= pc.LDS_BUDGET
    finally:
        backend.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_random_sequences(pkg, dev, synth, seed):
    cfg = CONFIGS[0]
    hyper, ops = sq.generate(cfg, seed)
    _run(pkg, dev, synth, cfg, hyper, ops, "seed %d" % seed)


def test_host_and_device_sources_alternate_with_a_host_reader_between(pkg, dev, synth):
    """seq_common.SOURCES_AND_READERS: updates from both sources around get_csr, an import, a prune and conv_mode flips."""
    import solver_common as sc
    hyper = dict(type=sc.ADAM, regularization=sc.REG_NONE, rate=1e-3, momentum=0.9, momentum2=0.999, delta=1e-8)
    _run(pkg, dev, synth, CONFIGS[0], hyper, sq.SOURCES_AND_READERS, "sources and readers")
