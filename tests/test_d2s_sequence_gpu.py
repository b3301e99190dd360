"""Plan option "deconv" driven through the op-sequence suite on the MI355X (seq_common.run_sequence, the Driver and its checks
unchanged; d2s_seq_common.py has the layers, the configurations and the backend): a Deconvolution layer whose forward, whole
backward, updates from both sources, solver steps, host reads, imports and conv_mode flips are compared with
plan_model.DeconvModel after every op -- the check that every copy of the weights (the outer value array, the inner plan's
forward copies, the inner backward state's, which the carry kernel reads through the entry map) is found in every order of
calls -- and at the end with a fresh plan: bits, states and workspace_bytes."""
import time

import pytest

import d2s_seq_common as ds
import seq_common as sq

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(pkg):
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        pytest.fail("no HIP device visible (these tests run on the MI355X)")
    return torch.device("cuda:0")


def _backend(pkg, dev, synth, cfg):
    inp = ds.make_inputs(cfg)
    model = ds.initial_model(synth, cfg, inp)
    return inp, model, ds.DeconvGpuBackend(pkg, dev, cfg, inp, model.csr())


def _run(pkg, dev, synth, cfg, hyper, ops, what):
    inp, model, backend = _backend(pkg, dev, synth, cfg)
    worst, t0 = {}, time.time()
    try:
        drv = sq.run_sequence(backend, cfg, inp, hyper, sq.supported(cfg, ops) + [sq.BWD], seed=what, worst=worst, model=model)
        print("\nsequence %s %s: %.2f s; %s" % (cfg.id, what, time.time() - t0, backend.plan.kernel_name))
        for kernel, ratio in sorted(worst.items()):
            print("    %-78s worst err/bound %.3g" % (kernel, ratio))
        return drv
    finally:
        backend.close()


def _named(pkg, cfg, plan):
    """The kernels the configuration names ran: the name ends in the unpack kernel and holds the inner kernel's substring;
    the stats are the inner plan's."""
    for key, want in cfg.expect.items():
        if key == "name":
            assert any(plan.kernel_name.endswith(t) for t in want), (cfg.id, plan.kernel_name)
        elif key == "inner":
            assert any(t in plan.kernel_name.lower() for t in want), (cfg.id, plan.kernel_name)
        else:
            assert plan.stat(key) == (getattr(pkg, want) if isinstance(want, str) else want), (cfg.id, key, plan.stat(key))


@pytest.mark.parametrize("cid", [c.id for c in ds.CONFIGS])
def test_each_configuration_runs_the_kernels_it_names(pkg, dev, synth, cid):
    import solver_common as sc
    cfg = ds.BY_ID[cid]
    inp, model, backend = _backend(pkg, dev, synth, cfg)
    try:
        sq.run_sequence(backend, cfg, inp, dict(type=sc.SGD, rate=1e-2), [sq.BWD], seed="kernels", model=model, finish=False)
        _named(pkg, cfg, backend.plan)
        print("\n%s: %s; backward kernels %d / %d" % (cid, backend.plan.kernel_name, backend.plan.stat("bwd_data_kernel"),
                                                      backend.plan.stat("wgrad_kernel")))
    finally:
        backend.close()


CASES = [(c.id, seed) for c in ds.CONFIGS for seed in ds.SEEDS[c.id]]


@pytest.mark.parametrize("cid,seed", CASES, ids=["%s-%d" % c for c in CASES])
def test_random_sequences(pkg, dev, synth, cid, seed):
    cfg = ds.BY_ID[cid]
    hyper, ops = sq.generate(cfg, seed)
    _run(pkg, dev, synth, cfg, hyper, ops, "seed %d" % seed)


@pytest.mark.parametrize("cid", [c.id for c in ds.CONFIGS])
def test_host_and_device_sources_alternate_with_a_host_reader_between(pkg, dev, synth, cid):
    """seq_common.SOURCES_AND_READERS without its prune: updates from both sources around get_csr, an import and conv_mode
    flips, each of which tears the inner plan down and builds it anew."""
    import solver_common as sc
    hyper = dict(type=sc.ADAM, regularization=sc.REG_NONE, rate=1e-3, momentum=0.9, momentum2=0.999, delta=1e-8)
    _run(pkg, dev, synth, ds.BY_ID[cid], hyper, sq.SOURCES_AND_READERS, "sources and readers")


@pytest.mark.parametrize("cid", [c.id for c in ds.CONFIGS])
def test_the_update_list_follows_the_inner_backward_state_and_the_solver(pkg, dev, synth, cid):
    """seq_common.list_lifecycle: set_values before the first backward; the backward, which builds the INNER plan's state (the
    outer plan has none); set_values again (the list grows by that state's copies); a solver step and updates from both
    sources."""
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
    _run(pkg, dev, synth, ds.BY_ID[cid], hyper, sq.list_lifecycle(first, grown, same), "update list")


@pytest.mark.parametrize("cid", ["deconv_jit", "deconv_auto"])
def test_a_flip_under_a_forced_inner_kernel_leaves_the_plan_aligned(pkg, dev, synth, cid):
    """seq_common.FLIP_UNDER_A_FORCED_INNER_KERNEL: the flip to LOWERED_SPARSE and back, on the configuration whose forced
    kernel exists for the inner layer only."""
    import solver_common as sc
    _run(pkg, dev, synth, ds.BY_ID[cid], dict(type=sc.SGD, rate=1e-2), sq.FLIP_UNDER_A_FORCED_INNER_KERNEL, "flip under a forced kernel")


@pytest.mark.parametrize("cid", ["deconv_jit", "deconv_g2_auto"])
def test_every_point_at_which_the_inner_plan_is_rebuilt(pkg, dev, synth, cid):
    """seq_common.derived_plan_lifecycle, filtered by the vocabulary: of its points the first backward, the conv_mode flips with
    an update between two of them and both imports remain (the prunes and rewires are refused on a deconv plan).  After every
    op the plan is still a deconv plan whose name ends in the unpack kernel.
    (seq_common.STEP_ON_NOTHING is not run: without its prune it is two solver steps, which every sequence here holds.)"""
    import solver_common as sc
    cfg = ds.BY_ID[cid]

    def check(drv):
        assert drv.b.stat("deconv") == 1 and drv.b.stat("deconv_scratch_bytes") > 0
        if drv.b.mode is None:
            assert drv.b.kernel_name.endswith("escoin_d2s_unpack_kernel"), drv.b.kernel_name

    hyper = dict(type=sc.NESTEROV, regularization=sc.REG_L1, rate=1e-2, momentum=0.9, decay=1e-3)
    ops = sq.supported(cfg, sq.derived_plan_lifecycle(check))
    assert [op for op, _ in ops if op != "check"].count("flip") == 3 and {"import_same", "import_fresh"} <= {op for op, _ in ops}
    _run(pkg, dev, synth, cfg, hyper, ops, "inner plan lifecycle")
