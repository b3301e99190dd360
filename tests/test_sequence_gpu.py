"""Plans on the MI355X driven through sequences of operations against plan_model.PlanModel, a float64-bounded model that keeps
the values bit-exact (seq_common.py: vocabulary, configurations, generator, driver; test_sequence_cpu.py proves model and
driver on the _cpu twins and checks the generator's coverage).  This is the check of "every copy of a plan's weights is
found, in every order of calls" (update_values.hip, for_each_copy): a stale copy gives a forward or a data gradient computed
from old weights, finite and plausible, which only a comparison with the model after every op notices.

Per configuration: the kernels the configuration is meant to run are asserted; a few seeded random sequences; one directed
sequence per transition the single-op tests leave unasserted.  Every case prints the kernels that ran and the worst
err / bound per kernel (pytest -s; profiles/sequence_fuzz.md)."""
import time

import pytest

import seq_common as sq
import solver_common as sc
from seq_backends import GpuBackend
from test_errbound_gpu import DIL, G5X5, L3X3, PW_B, STR2

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
IDS = [c.id for c in sq.CONFIGS]
FLOAT_IDS = [c.id for c in sq.CONFIGS if not c.f64]
# jit_loader has no in-place path (code the HIP module loader placed): every update rebuilds the plan, so the two directed
# sequences about the in-place list and the value map are not about it; it runs every other one
IN_PLACE_IDS = [c.id for c in sq.CONFIGS if not c.options.get("code_loader")]
# the configurations whose plan runs generated code and loads a persisted code object as it is (stat import_fast == 1)
FAST_IMPORT_IDS = ["jit_3x3", "mixed_groups", "pointwise"]
# the configurations whose plan runs through an inner plan (options "s2d" and "s2b")
DERIVED_IDS = [c.id for c in sq.CONFIGS if c.options.get("s2d") or c.options.get("s2b")]


@pytest.fixture(scope="module")
def dev(pkg):
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        pytest.fail("no HIP device visible (these tests run on the MI355X)")
    return torch.device("cuda:0")


def _backend(pkg, dev, synth, cfg):
    inp = sq.make_inputs(synth, cfg)
    return inp, GpuBackend(pkg, dev, cfg, inp, sq.initial_model(cfg, inp).csr())


def _kernels(backend):
    # ("kernel -": the end-of-sequence comparison's last call rebuilt the plan, and no backward has run since)
    return "%s | data gradient %s, weight gradient %s" % (backend.plan.kernel_name, backend.label("dgrad"), backend.label("wgrad"))


def _report(cid, what, backend, worst, t0):
    print("\nsequence %s %s: %.2f s; %s" % (cid, what, time.time() - t0, _kernels(backend)))
    for kernel, ratio in sorted(worst.items()):
        print("    %-78s worst err/bound %.3g" % (kernel, ratio))


def _run(pkg, dev, synth, cid, hyper, ops, what, after=None):
    """One sequence on a new plan of the configuration; ends with a backward so that the kernels' stats exist."""
    cfg = sq.BY_ID[cid]
    inp, backend = _backend(pkg, dev, synth, cfg)
    worst, t0 = {}, time.time()
    try:
        drv = sq.run_sequence(backend, cfg, inp, hyper, sq.supported(cfg, ops) + [sq.BWD], seed=what, worst=worst)
        if after:
            after(drv)
        _report(cid, what, backend, worst, t0)
    finally:
        backend.close()


def test_the_layers_are_the_error_bound_suites():
    assert [sq.LAYERS[k] for k in ("L3X3", "PW_B", "G5X5", "STR2", "DIL")] == [L3X3, PW_B, G5X5, STR2, DIL] and len(sq.LAYERS) == 5


@pytest.mark.parametrize("cid", IDS)
def test_each_configuration_runs_the_kernels_it_names(pkg, dev, synth, cid):
    """The forward, data-gradient and weight-gradient kernels of the configuration table, by kernel_name and stats, on the
    layer the sequences use."""
    cfg = sq.BY_ID[cid]
    inp, backend = _backend(pkg, dev, synth, cfg)
    try:
        sq.run_sequence(backend, cfg, inp, dict(type=sc.SGD, rate=1e-2), [sq.BWD], seed="kernels", finish=False)
        plan = backend.plan
        print("\nconfiguration %s: %s" % (cid, _kernels(backend)))
        for key, want in cfg.expect.items():
            if key == "name":
                assert any(t in plan.kernel_name for t in want), (cid, plan.kernel_name)
            else:
                assert plan.stat(key) == (getattr(pkg, want) if isinstance(want, str) else want), (cid, key, plan.stat(key))
        assert plan.stat("is_f64") == int(cfg.f64)
    finally:
        backend.close()


CASES = [(c.id, seed) for c in sq.CONFIGS for seed in sq.SEEDS[c.id]]


@pytest.mark.parametrize("cid,seed", CASES, ids=["%s-%d" % c for c in CASES])
def test_random_sequences(pkg, dev, synth, cid, seed):
    hyper, ops = sq.generate(sq.BY_ID[cid], seed)
    _run(pkg, dev, synth, cid, hyper, ops, "seed %d" % seed)


# ---- directed sequences ---------------------------------------------------------------------------------------------------------
SGD = dict(type=sc.SGD, regularization=sc.REG_L2, rate=1e-2, momentum=0.9, decay=1e-3)
ADAM = dict(type=sc.ADAM, regularization=sc.REG_NONE, rate=1e-3, momentum=0.9, momentum2=0.999, delta=1e-8)


@pytest.mark.parametrize("cid", IN_PLACE_IDS)
def test_the_update_list_follows_the_backward_state_and_the_solver(pkg, dev, synth, cid):
    """set_values before the first backward; the backward, whose state holds a copy of the weights; set_values again (the
    list grows by that copy); a solver step (the list is rebuilt for the entry view) and updates from both sources (it
    stays put); after each, the forward and the data gradient against the model."""
    seen = {}

    def first(drv):
        seen["n"] = drv.b.stat("update_destinations")
        assert seen["n"] >= drv.m.nnz > 0 and drv.b.stat("bwd_device_bytes") == 0

    def grown(drv):
        assert drv.b.stat("update_destinations") > seen["n"], (seen, drv.b.stat("update_destinations"))
        seen["n"] = drv.b.stat("update_destinations")

    def same(drv):
        assert drv.b.stat("update_destinations") == seen["n"] and drv.b.stat("update_fast") == 1, (seen, drv.b.stat("update_destinations"))

    _run(pkg, dev, synth, cid, SGD, sq.list_lifecycle(first, grown, same), "list lifecycle")


@pytest.mark.parametrize("cid", IDS)
def test_host_and_device_sources_alternate_with_a_host_reader_between(pkg, dev, synth, cid):
    _run(pkg, dev, synth, cid, ADAM, sq.SOURCES_AND_READERS, "sources and readers")


@pytest.mark.parametrize("cid", [c for c in FLOAT_IDS if c in IN_PLACE_IDS])
def test_updates_and_solver_steps_after_an_import(pkg, dev, synth, cid):
    """export_aligned -> import_aligned, then an update, a solver step, a prune and an update again.  Where the import is
    fast (generated code loaded as it is, no value map): import_fast == 1, the update after it rebuilds (update_fast 0),
    so does a solver step (on the values-only list), and after a prune the update is in place again (1).  Elsewhere the
    import re-aligns and every update is in place."""
    fast = cid in FAST_IMPORT_IDS

    def is_fast(drv):
        assert drv.b.stat("import_fast") == int(fast), (cid, drv.b.stat("import_fast"))

    def fast0(drv):
        assert drv.b.stat("update_fast") == (0 if fast else 1), cid

    def fast1(drv):
        assert drv.b.stat("update_fast") == 1, cid

    _run(pkg, dev, synth, cid, SGD, sq.fast_import(is_fast, fast0, fast1), "import")


@pytest.mark.parametrize("cid", FLOAT_IDS)
def test_a_rigl_schedule(pkg, dev, synth, cid):
    """dense_wgrad -> rewire -> compact_entries -> solver_step repeated, with prunes in between."""
    _run(pkg, dev, synth, cid, ADAM, sq.RIGL, "RigL")


@pytest.mark.parametrize("cid", IDS)
def test_an_emptied_plan_grows_again(pkg, dev, synth, cid):
    """A prune to an empty pattern (the forward is then the bias, exactly), a solver step and an update that find nothing to
    do, a rewire that grows from nothing, then steps: the grown entries' gradients within bound, the values the model's."""
    def after(drv):
        assert drv.m.stats["rewire_last_grown"] == drv.m.nnz > 8 and drv.b.stat("update_fast") == int(cid in IN_PLACE_IDS)

    _run(pkg, dev, synth, cid, dict(type=sc.NESTEROV, regularization=sc.REG_NONE, rate=1e-2, momentum=0.9),
         sq.empty_then_grow(sq.empty_forward_is_the_bias), "emptied", after)


@pytest.mark.parametrize("cid", DERIVED_IDS)
def test_a_derived_plan_is_rebuilt_at_every_point_that_tears_it_down(pkg, dev, synth, cid):
    """seq_common.derived_plan_lifecycle on the plans that run through an inner plan.  After every op, in the plan's own
    conv_mode: the option is active and kernel_name has the option's parts around the inner plan's name; the scratch is
    the size it had at the first check (a rebuild allocates it again, never a second one); workspace_bytes is the sum of the
    four states' bytes.  The driver's forward after every mutating op and its comparison with a fresh plan do the rest."""
    opt = "s2b" if cid.startswith("s2b") else "s2d"
    seen = {}

    def check(drv):
        plan = drv.b.plan
        name = plan.kernel_name
        assert drv.b.mode is None and plan.stat(opt) == 1 and plan.stat("s2d" if opt == "s2b" else "s2b") == 0, (cid, name)
        parts = name.split(" + ")
        if opt == "s2b":
            assert len(parts) >= 3 and parts[0] == "escoin_s2b_pack_kernel" and parts[-1] == "escoin_s2b_unpack_kernel", name
            inner = parts[1:-1]
        else:
            assert len(parts) >= 2 and parts[0] == "escoin_s2d_pack_kernel", name
            inner = parts[1:]
        assert all(p.startswith("escoin_") and "_s2" not in p for p in inner), name
        scratch = plan.stat(opt + "_scratch_bytes")
        assert scratch > 0 and seen.setdefault("scratch", scratch) == scratch, (cid, seen, scratch)
        assert plan.stat("device_bytes") > scratch
        assert plan.workspace_bytes == sum(plan.stat(k + "device_bytes") for k in ("", "bwd_", "upd_", "dwg_")), (cid, drv.b.accounting())

    _run(pkg, dev, synth, cid, SGD, sq.derived_plan_lifecycle(check), "derived plan lifecycle")


@pytest.mark.parametrize("cid", ["s2b_inner_jit"])
def test_a_flip_to_lowered_sparse_under_a_forced_inner_kernel(pkg, dev, synth, cid):
    """The shortest sequence of the one refusal the "s2b" configurations found (seq_common has it): the flip aligns the
    plan on its dilated geometry, where no generated code exists, and back in its own mode the inner plan runs it again."""
    def check(drv):
        plan = drv.b.plan
        assert plan.stat("s2b") == 1 and "jit" in plan.kernel_name and plan.stat("bwd_data_kernel") == pkg.KERNEL_JIT, plan.kernel_name

    _run(pkg, dev, synth, cid, SGD, sq.FLIP_UNDER_A_FORCED_INNER_KERNEL + [sq.BWD, ("check", dict(fn=check))], "flip under a forced inner kernel")


@pytest.mark.parametrize("cid", IDS)
def test_a_solver_step_on_a_plan_pruned_to_nothing(pkg, dev, synth, cid):
    """Plan.solver_step and compact_entries with the tensors a training loop then holds: of 0 elements, whose data_ptr() is
    null.  The step launches nothing, counts as an update and leaves update_fast as the last real update set it."""
    def after(drv):
        assert drv.m.nnz == 0 and drv.b.nnz() == 0 and drv.b.stat("update_count") == 2
        assert drv.b.stat("update_fast") == int(cid in IN_PLACE_IDS)
        h, h2 = drv.b.histories()
        assert h.size == 0 and (h2 is None or h2.size == 0)

    cfg = sq.BY_ID[cid]
    inp, backend = _backend(pkg, dev, synth, cfg)
    try:
        after(sq.run_sequence(backend, cfg, inp, ADAM, sq.STEP_ON_NOTHING, seed="step on nothing", finish=False))
    finally:
        backend.close()
