"""Random sequences of plan operations on the _cpu twins against plan_model.PlanModel (seq_common.py has the vocabulary, the
generator and the driver; test_sequence_gpu.py runs the same driver over the device entry points).  Needs no GPU: it proves
the model and the driver right before a device is involved.

Also here: the generator's coverage assertion (no library at all), and the driver's self-check in the style of errbound's
corruptions -- three wrapper backends, each wrong in one way, on which the driver must fail AT THE STEP where the fault
happens, not merely at the end."""
import numpy as np
import pytest

import prune_common as pc
import rewire_common as rc
import seq_common as sq
import solver_common as sc
from seq_backends import CpuBackend


# ---- the generator: no library ---------------------------------------------------------------------------------------------
def test_generator_coverage():
    """Per configuration every op of its vocabulary occurs at least twice over its seeds; over the device suite every
    ordered pair of distinct mutating ops occurs adjacently (forwards, backwards and reads in between ignored)."""
    counts, pairs = sq.coverage(sq.CONFIGS)
    for cfg in sq.CONFIGS:
        assert set(counts[cfg.id]) == set(sq.vocabulary(cfg)) and not set(cfg.exclude) & set(counts[cfg.id])
        short = {op: n for op, n in counts[cfg.id].items() if n < 2}
        assert not short, (cfg.id, short)
    want = {(a, b) for a in sq.MUTATING_CLASSES for b in sq.MUTATING_CLASSES if a != b}
    assert want - pairs == set(), sorted(want - pairs)
    cpu_counts, _ = sq.coverage(sq.CPU_CONFIGS)
    for cfg in sq.CPU_CONFIGS:
        short = {op: n for op, n in cpu_counts[cfg.id].items() if n < 2}
        assert not short, (cfg.id, short)


def test_generated_sequences_are_a_function_of_the_seed_alone():
    cfg = sq.BY_ID["jit_3x3"]
    assert sq.generate(cfg, 5) == sq.generate(cfg, 5) and sq.generate(cfg, 5) != sq.generate(cfg, 6)
    assert all(op in sq.vocabulary(sq.BY_ID["double"]) for op, _ in sq.generate(sq.BY_ID["double"], 1, 200)[1])
    for c in sq.CONFIGS + sq.CPU_CONFIGS:
        assert len(sq.SEEDS[c.id]) >= 2 and all(op in sq.OPS and why for op, why in c.exclude.items())


# ---- random sequences over the CPU twins --------------------------------------------------------------------------------------
def _backend(pkg, synth, cfg):
    inp = sq.make_inputs(synth, cfg)
    return inp, CpuBackend(pkg, cfg, inp, sq.initial_model(cfg, inp).csr())


CPU_CASES = [(c.id, seed) for c in sq.CPU_CONFIGS for seed in sq.SEEDS[c.id]]


@pytest.mark.parametrize("cid,seed", CPU_CASES, ids=["%s-%d" % c for c in CPU_CASES])
def test_random_sequences_on_the_cpu_twins(pkg, synth, cid, seed):
    cfg = sq.BY_ID[cid]
    inp, backend = _backend(pkg, synth, cfg)
    hyper, ops = sq.generate(cfg, seed)
    worst = {}
    try:
        sq.run_sequence(backend, cfg, inp, hyper, ops, seed=seed, worst=worst)
    finally:
        backend.close()
    for kernel, ratio in sorted(worst.items()):
        print("sequence %-16s seed %d  %-40s worst err/bound %.3g" % (cid, seed, kernel, ratio))


# ---- directed: a RigL schedule, and a prune to nothing followed by a rewire that grows from nothing ---------------------------
@pytest.mark.parametrize("cid", [c.id for c in sq.CPU_CONFIGS])
@pytest.mark.parametrize("rule", ["sgd", "adam"])
def test_a_rigl_schedule_on_the_cpu_twins(pkg, synth, cid, rule):
    cfg = sq.BY_ID[cid]
    inp, backend = _backend(pkg, synth, cfg)
    hyper = dict(type=sc.RULES[rule], regularization=sc.REG_L2, rate=1e-2, momentum=0.9, decay=1e-3)
    try:
        sq.run_sequence(backend, cfg, inp, hyper, sq.RIGL, seed="rigl")
    finally:
        backend.close()


@pytest.mark.parametrize("cid", [c.id for c in sq.CPU_CONFIGS])
def test_an_emptied_plan_grows_again_on_the_cpu_twins(pkg, synth, cid):
    cfg = sq.BY_ID[cid]
    inp, backend = _backend(pkg, synth, cfg)
    hyper = dict(type=sc.NESTEROV, regularization=sc.REG_NONE, rate=1e-2, momentum=0.9)
    try:
        drv = sq.run_sequence(backend, cfg, inp, hyper, sq.empty_then_grow(sq.empty_forward_is_the_bias), seed="empty")
        assert drv.m.stats["rewire_last_grown"] == drv.m.nnz > 8 and drv.m.stats["prune_last_dropped"] > 0
    finally:
        backend.close()


def test_arrays_of_no_elements_may_be_null(pkg, synth):
    """The C entry points on a plan of 0 entries: diff and the histories may be NULL (an empty tensor's pointer), Adam
    included; compact_entries takes a NULL destination of 0 elements, and its host route refuses one when the map keeps an
    entry.  With entries, NULL is refused as before."""
    import ctypes as C
    L = pkg.lib()
    cfg = sq.BY_ID["cpu_stride2_f32"]
    inp, backend = _backend(pkg, synth, cfg)
    plan = backend.plan
    adam = pkg.SolverDesc.make(type="adam", rate=1e-3)
    n = plan.nnz()
    assert n > 0 and L.escoin_solver_step_cpu(plan._h, C.byref(adam), None, None, None, None) == -1
    entry_map = plan.prune_cpu(keep=0)
    assert plan.nnz() == 0 and np.all(entry_map == -1)
    count = plan.stat("update_count")
    assert L.escoin_solver_step_cpu(plan._h, C.byref(adam), None, None, None, None) == 0
    assert plan.stat("update_count") == count + 1
    src = np.arange(n, dtype=np.float32)
    args = (entry_map.ctypes.data_as(C.c_void_p), n, 4, src.ctypes.data_as(C.c_void_p), None, 0, None)
    assert L.escoin_compact_entries(*args) == 0
    entry_map[n // 2] = 0
    assert L.escoin_compact_entries(*args) == -1 and "dst is NULL" in L.escoin_last_error().decode()
    backend.close()
    for cid in ("cpu_3x3_f32", "cpu_groups_f64"):       # ... and through the driver, histories and all
        cfg = sq.BY_ID[cid]
        inp, backend = _backend(pkg, synth, cfg)
        hyper = dict(type=sc.ADAM, regularization=sc.REG_NONE, rate=1e-3, momentum=0.9, momentum2=0.999, delta=1e-8)
        drv = sq.run_sequence(backend, cfg, inp, hyper, sq.STEP_ON_NOTHING, seed="step on nothing", finish=False)
        assert drv.m.nnz == 0 and backend.nnz() == 0
        backend.close()


# ---- the driver's self-check: three backends that are each wrong in one way --------------------------------------------------------
class _Wrapper(object):
    def __init__(self, inner):
        self._inner = inner

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def fresh(self, csr):
        return self._inner.fresh(csr)


class DropsOneSetValues(_Wrapper):
    """The second set_values never reaches the plan (a stale copy of the weights)."""
    calls = 0

    def set_values(self, v, source):
        self.calls += 1
        if self.calls != 2:
            self._inner.set_values(v, source)


class CarriesHistoryUncompacted(_Wrapper):
    """After a prune the history keeps its old order: the first new-nnz elements instead of the kept ones."""

    def compact_histories(self, entry_map):
        n = self._inner.plan.nnz()
        for name in ("h", "h2"):
            if getattr(self._inner, name) is not None:
                setattr(self._inner, name, np.array(getattr(self._inner, name)[:n]))


class GrowTieToTheHigherPosition(_Wrapper):
    """Among the candidates that tie at the grow boundary, the last one the rule grows is passed over for the first one it
    does not: the tie resolved to the higher position."""

    def rewire(self, grow, score, init=None, **drop):
        s = self._inner.inp.s
        rp, ci, _, ng = self._inner.plan.get_csr()
        cand = rc.candidates(rc.dense_size(s), sq.positions(s, rp, ci, ng))
        k = pc.keys(score[cand])
        order = np.argsort(np.iinfo(k.dtype).max - k, kind="stable")
        assert 0 < grow < cand.size and k[order[grow - 1]] == k[order[grow]], "the self-check needs a tie at the boundary"
        last_in, first_out = cand[order[grow - 1]], cand[order[grow]]
        assert first_out > last_in
        score = score.copy()
        score[last_in] = np.nextafter(score[last_in], score.dtype.type(0))       # a hair smaller: first_out now outranks it
        return self._inner.rewire(grow, score, init=init, **drop)


SELF_CHECKS = {
    "drops_a_set_values": (DropsOneSetValues, 3,
                           [("set_values", dict(source="host", seed=1)), sq.BWD, sq.STEP, ("set_values", dict(source="device", seed=3)),
                            ("forward", dict(bias=True, partial=False)),
                            ("prune", dict(mode="keep", frac=0.8, seed=4)), ("get_csr", {})]),
    "history_not_compacted": (CarriesHistoryUncompacted, 2,
                              [sq.STEP, ("solver_step", dict(partial=True)), ("prune", dict(mode="keep", frac=0.7, seed=5)), sq.STEP,
                               ("get_csr", {})]),
    "grow_tie_to_the_higher_position": (GrowTieToTheHigherPosition, 1,
                                        [("update_values", dict(source="host", seed=6)),
                                         ("rewire", dict(drop="keep", drop_frac=0.9, grow_frac=0.2, init=True, score="ties", seed=7)),
                                         ("solver_step", dict(partial=False)), ("get_csr", {})]),
}


@pytest.mark.parametrize("cid", ["cpu_3x3_f32", "cpu_groups_f64"])
@pytest.mark.parametrize("name", sorted(SELF_CHECKS))
def test_the_driver_fails_at_the_step_where_a_backend_goes_wrong(pkg, synth, capsys, cid, name):
    wrapper, at, ops = SELF_CHECKS[name]
    cfg = sq.BY_ID[cid]
    hyper = dict(type=sc.ADAM, regularization=sc.REG_NONE, rate=1e-3, momentum=0.9, momentum2=0.999, delta=1e-8)
    inp, backend = _backend(pkg, synth, cfg)
    sq.run_sequence(backend, cfg, inp, hyper, ops, seed=name)          # the honest backend passes the same ops
    backend.close()
    inp, backend = _backend(pkg, synth, cfg)
    with pytest.raises(sq.SequenceError) as e:
        sq.run_sequence(wrapper(backend), cfg, inp, hyper, ops, seed=name)
    backend.close()
    assert e.value.index == at, (name, e.value.index, str(e.value.cause))
    out = capsys.readouterr().out            # the failure names the configuration, the seed, every op and the failing index
    assert "configuration %s, seed %r, op %d of %d" % (cid, name, at, len(ops)) in out and out.count("\n    (") == len(ops)
    assert "<-- failed here" in [l for l in out.splitlines() if l.startswith("    (")][at]
