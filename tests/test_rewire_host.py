"""escoin_plan_rewire_cpu without a GPU: plans aligned by weight_align_cpu, float and double.  Every comparison is exact:
the feature is two selections, a merge and a re-index.  The yardstick is rewire_common's numpy restatement of the rule (a
stable sort on the integer keys over the candidates); the library's host code selects without a sort."""
import ctypes as C

import numpy as np
import pytest

import prune_common as pc
import rewire_common as rc
import solver_common as sc
from test_prune_host import cpu_plan, _codes, _inputs
from upd_common import same_bits

DTYPES = [np.float32, np.float64]
HYPER = dict(rate=0.01, momentum=0.9, momentum2=0.999, delta=1e-8, decay=5e-4)


def _shape(synth, kind):
    if kind == "kh3_kw2":
        return synth.shape("rewire_3x2", 2, 8, 6, 6, 12, 3, KW=2, pad=1, sparsity=0.5)            # D = 576
    return synth.shape("rewire_g2", 2, 16, 6, 6, 12, 3, pad=1, group=2, sparsity=0.5)               # D = 864


def _positions(desc, n, seed):
    return np.sort(np.random.RandomState(seed).permutation(rc.dense_size(desc))[:n])


def check_rewired(plan, want, got_map, got_grown):
    """Both maps, the stats and the plan's CSR against the reference."""
    assert got_map.dtype == np.int32 and got_grown.dtype == np.int32
    assert np.array_equal(got_map, want["entry_map"]) and np.array_equal(got_grown, want["grown"])
    assert plan.nnz() == want["pos"].size
    got = plan.get_csr()
    w_rp, w_ci, w_va, w_ng = want["csr"]
    assert np.array_equal(got[0], w_rp) and np.array_equal(got[1], w_ci) and same_bits(got[2], w_va) and np.array_equal(got[3], w_ng)
    assert plan.stat("rewire_last_dropped") == int((want["entry_map"] < 0).sum())
    assert plan.stat("rewire_last_grown") == want["grown"].size
    assert plan.stat("prune_count") == 0 and plan.stat("prune_last_dropped") == 0


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["kh3_kw2", "group2"])
def test_rewire_equals_the_reference_rule(pkg, synth, dt, kind):
    """Every score case over the D positions, every grow count (0, 1, a tie boundary, D - nnz, more), without and with a
    drop."""
    desc = pkg.ConvDesc.from_shape(_shape(synth, kind))
    D = rc.dense_size(desc)
    n = D // 3
    pos = _positions(desc, n, 3)
    values = sc.seeded_values(n, 4, dt)
    for name, score in rc.score_cases(D, dt, 7).items():
        poisoned = score.copy()
        poisoned[pos[::5]] = np.nan                                # read only at candidate positions
        for grow in rc.grow_counts(score, pos):
            for drop_keep in (None, n // 2):
                plan = cpu_plan(pkg, desc, pos, values)
                want = rc.ref_rewire(desc, plan.get_csr(), grow, score, drop_keep=drop_keep)
                assert want["grown"].size == min(grow, D - n)
                got_map, got_grown = plan.rewire_cpu(grow, poisoned, drop_keep=drop_keep)
                check_rewired(plan, want, got_map, got_grown)
                assert plan.stat("rewire_count") == 1, (name, grow, drop_keep)
                plan.close()


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_init_values_and_the_drop_variants(pkg, synth, dt):
    desc = pkg.ConvDesc.from_shape(_shape(synth, "group2"))
    D = rc.dense_size(desc)
    n = 300
    pos = _positions(desc, n, 5)
    values = sc.seeded_values(n, 6, dt)
    cases = rc.score_cases(D, dt, 8)
    init = np.random.RandomState(9).uniform(-1, 1, D).astype(dt)
    init[::7] = -0.0                                               # bits, not values
    init[3::11] = np.nan
    drop_score = pc.score_cases(n, dt, 10)["ties"]
    thr = float(np.median(np.abs(values)))
    for kw in (dict(), dict(drop_keep=pc.tie_boundary_keep(drop_score, n // 2), drop_score=drop_score), dict(drop_threshold=thr),
               dict(drop_keep=0)):
        plan = cpu_plan(pkg, desc, pos, values)
        want = rc.ref_rewire(desc, plan.get_csr(), 200, cases["specials"], init=init, **kw)
        got_map, got_grown = plan.rewire_cpu(200, cases["specials"], init=init, **kw)
        check_rewired(plan, want, got_map, got_grown)
        plan.close()
    # sparsity is a keep count over the dense size, as for a prune
    plan = cpu_plan(pkg, desc, pos, values)
    want = rc.ref_rewire(desc, plan.get_csr(), 50, cases["ties"], drop_keep=int(round(0.1 * D)))
    got_map, got_grown = plan.rewire_cpu(50, cases["ties"], drop_sparsity=0.9)
    check_rewired(plan, want, got_map, got_grown)
    with pytest.raises(pkg.EscoinError):
        plan.rewire_cpu(1, cases["ties"], drop_keep=3, drop_sparsity=0.5)
    plan.close()


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_an_empty_plan_grows_and_a_full_plan_does_not(pkg, synth, dt):
    s = _shape(synth, "kh3_kw2")
    desc = pkg.ConvDesc.from_shape(s)
    D = rc.dense_size(desc)
    score = rc.score_cases(D, dt, 11)["specials"]
    empty = pkg.Plan(desc)
    empty.weight_align_cpu(np.zeros((desc.M, desc.C // desc.group, desc.KH, desc.KW), dt))
    assert empty.nnz() == 0
    want = rc.ref_rewire(desc, empty.get_csr(), 100, score)
    got_map, got_grown = empty.rewire_cpu(100, score)
    assert got_map.size == 0
    check_rewired(empty, want, got_map, got_grown)
    assert np.all(empty.get_csr()[2] == 0) and not np.any(np.signbit(empty.get_csr()[2]))
    # ... the NaN score was grown first
    assert np.flatnonzero(np.isnan(score))[0] in want["grown_pos"]
    x, b = _inputs(s, dt, 12)
    top = empty.forward_cpu(x, b)
    assert np.array_equal(top, np.broadcast_to(b[None, :, None, None], top.shape))     # explicit zeros: forward = bias
    empty.close()
    full = cpu_plan(pkg, desc, np.arange(D), sc.seeded_values(D, 13, dt))
    before, align_us = full.get_csr(), full.stat("align_us")
    got_map, got_grown = full.rewire_cpu(5, score)
    assert np.array_equal(got_map, np.arange(D, dtype=np.int32)) and got_grown.size == 0
    assert full.stat("align_us") == align_us and all(same_bits(a, c) for a, c in zip(before, full.get_csr()))
    # a full plan with a drop: the dropped positions are no candidates in the same call
    want = rc.ref_rewire(desc, before, 5, score, drop_keep=D - 9)
    got_map, got_grown = full.rewire_cpu(5, score, drop_keep=D - 9)
    assert got_grown.size == 0
    check_rewired(full, want, got_map, got_grown)
    full.close()


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_nothing_dropped_and_nothing_grown_leaves_the_plan_untouched(pkg, synth, dt):
    desc = pkg.ConvDesc.from_shape(_shape(synth, "group2"))
    D, n = rc.dense_size(desc), 250
    plan = cpu_plan(pkg, desc, _positions(desc, n, 14), pc.score_cases(n, dt, 15)["specials"])
    score = rc.score_cases(D, dt, 16)["ties"]
    before, align_us = plan.get_csr(), plan.stat("align_us")
    for grow, s, kw in ((0, None, dict()), (0, score, dict()), (0, None, dict(drop_keep=n)), (0, score, dict(drop_keep=n + 5)),
                        (0, None, dict(drop_threshold=0.0))):
        got_map, got_grown = plan.rewire_cpu(grow, s, **kw)
        assert np.array_equal(got_map, np.arange(n, dtype=np.int32)) and got_grown.size == 0
        assert plan.stat("rewire_last_dropped") == 0 and plan.stat("rewire_last_grown") == 0 and plan.stat("align_us") == align_us
        assert all(same_bits(a, c) for a, c in zip(before, plan.get_csr()))
    assert plan.stat("rewire_count") == 5
    # every output pointer may be NULL; new_nnz and n_grown report the counts
    sc_arr = np.ascontiguousarray(score)
    d = pkg.RewireDesc(None, 10, sc_arr.ctypes.data, None)
    new_nnz, n_grown = C.c_long(-1), C.c_long(-1)
    L = pkg.lib()
    assert L.escoin_plan_rewire_cpu(plan._h, C.byref(d), None, None, C.byref(new_nnz), C.byref(n_grown)) == 0
    assert new_nnz.value == n + 10 and n_grown.value == 10 and plan.nnz() == n + 10
    assert L.escoin_plan_rewire_cpu(plan._h, C.byref(d), None, None, None, None) == 0 and plan.nnz() == n + 20
    plan.close()


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_grow_zero_with_a_drop_equals_prune_cpu(pkg, synth, dt):
    desc = pkg.ConvDesc.from_shape(_shape(synth, "group2"))
    n = 400
    pos = _positions(desc, n, 17)
    for name, values in pc.score_cases(n, dt, 18).items():
        keep = pc.tie_boundary_keep(values, n // 2)
        for kw_r, kw_p in ((dict(drop_keep=keep), dict(keep=keep)), (dict(drop_threshold=0.5), dict(threshold=0.5))):
            a, b = cpu_plan(pkg, desc, pos, values), cpu_plan(pkg, desc, pos, values)
            got_map, got_grown = a.rewire_cpu(0, None, **kw_r)
            want_map = b.prune_cpu(**kw_p)
            assert np.array_equal(got_map, want_map) and got_grown.size == 0, name
            assert all(same_bits(x, y) for x, y in zip(a.get_csr(), b.get_csr()))
            assert a.stat("rewire_last_dropped") == b.stat("prune_last_dropped") and a.stat("prune_count") == 0
            a.close(), b.close()


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["kh3_kw2", "group2"])
def test_forward_and_backward_equal_a_fresh_plan(pkg, synth, dt, kind):
    """get_csr / forward_cpu / backward_cpu after a rewire against fresh plans: one aligned by weight_align_cpu on the
    dense weights (grown entries initialised nonzero), one holding the same CSR with explicit zeros (grown entries +0)."""
    s = _shape(synth, kind)
    desc = pkg.ConvDesc.from_shape(s)
    D, n = rc.dense_size(desc), 260
    pos = _positions(desc, n, 19)
    values = sc.seeded_values(n, 20, dt, zeros=False)
    score = np.random.RandomState(21).uniform(-1, 1, D).astype(dt)
    init = sc.seeded_values(D, 22, dt, zeros=False)
    x, b = _inputs(s, dt, 23)
    for use_init in (True, False):
        plan = cpu_plan(pkg, desc, pos, values)
        plan.forward_cpu(x, b)                       # (the offsets of the old pattern exist when the rewire comes)
        want = rc.ref_rewire(desc, plan.get_csr(), 90, score, init=init if use_init else None, drop_keep=n - 80)
        got_map, got_grown = plan.rewire_cpu(90, score, init=init if use_init else None, drop_keep=n - 80)
        check_rewired(plan, want, got_map, got_grown)
        if use_init:
            fresh = pkg.Plan(desc)
            fresh.weight_align_cpu(pc.masked_dense(desc, *want["csr"]))
        else:
            fresh = cpu_plan(pkg, desc, want["pos"], want["csr"][2])
        assert all(same_bits(a, c) for a, c in zip(plan.get_csr(), fresh.get_csr()))
        top, want_top = plan.forward_cpu(x, b), fresh.forward_cpu(x, b)
        assert same_bits(top, want_top) and np.abs(top).max() > 0
        td = np.random.RandomState(24).uniform(-1, 1, top.shape).astype(dt)
        got = plan.backward_cpu(td, bottom=x, values_diff=True, bias_diff=True)
        ref = fresh.backward_cpu(td, bottom=x, values_diff=True, bias_diff=True)
        assert all(same_bits(a, c) for a, c in zip(got, ref))
        assert got[1].size == n + 10 and np.any(got[1][got_grown] != 0)      # the grown entries receive a gradient
        plan.close(), fresh.close()


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("rule", ["sgd", "nesterov", "adam"])
def test_training_continues_with_carried_histories(pkg, synth, dt, rule):
    got = continuity_cpu(pkg, synth, dt, rule)
    assert got["new_nnz"] == got["pos"].size - got["dropped"] + got["grow"]


def continuity_cpu(pkg, synth, dt, rule):
    """Two solver steps, a rewire, compact_entries over the histories into zeros, one more step: equal, bit for bit, to the
    same step on a fresh plan given numpy-re-indexed histories.  Returns what the device twin compares with."""
    desc = pkg.ConvDesc.from_shape(_shape(synth, "group2"))
    D, n, keep, grow = rc.dense_size(desc), 400, 310, 120
    hyper = dict(HYPER, type=sc.RULES[rule], regularization=sc.REG_L2)
    w0 = sc.seeded_values(n, 31, dt, zeros=False)
    pos = _positions(desc, n, 32)
    plan = cpu_plan(pkg, desc, pos, w0)
    adam = rule == "adam"
    h, h2 = np.zeros(n, dt), (np.zeros(n, dt) if adam else None)
    grads = [sc.seeded_values(n, 33 + k, dt) for k in range(2)]
    for k in range(2):
        plan.solver_step_cpu(grads[k].copy(), h, h2, **hyper)
    score = np.random.RandomState(36).uniform(-1, 1, D).astype(dt)
    before = tuple(a.copy() for a in plan.get_csr())
    want = rc.ref_rewire(desc, before, grow, score, drop_keep=keep)
    entry_map, grown = plan.rewire_cpu(grow, score, drop_keep=keep)
    check_rewired(plan, want, entry_map, grown)
    new_nnz = plan.nnz()
    h_new = pkg.compact_entries(entry_map, h, out=np.zeros(new_nnz, dt))
    h2_new = pkg.compact_entries(entry_map, h2, out=np.zeros(new_nnz, dt)) if adam else None
    assert same_bits(h_new, rc.reindex(entry_map, new_nnz, h)) and np.any(h_new != 0) and np.all(h_new[grown] == 0)
    g_new = sc.seeded_values(new_nnz, 37, dt)
    fresh = cpu_plan(pkg, desc, want["pos"], want["csr"][2])
    fh, fh2 = rc.reindex(entry_map, new_nnz, h), (rc.reindex(entry_map, new_nnz, h2) if adam else None)
    fh_in, fh2_in = fh.copy(), (fh2.copy() if adam else None)
    plan.solver_step_cpu(g_new.copy(), h_new, h2_new, **hyper)
    fresh.solver_step_cpu(g_new.copy(), fh, fh2, **hyper)
    out, ref = plan.get_csr(), fresh.get_csr()
    assert all(same_bits(a, c) for a, c in zip(out, ref))
    assert same_bits(h_new, fh) and (not adam or same_bits(h2_new, fh2))
    # ... and the restatement agrees with both
    w3, wh, _ = sc.step(want["csr"][2], g_new, fh_in, fh2_in, **hyper)
    assert same_bits(out[2], w3) and same_bits(h_new, wh)
    res = dict(values=out[2].copy(), h=h_new.copy(), h2=None if h2_new is None else h2_new.copy(), map=entry_map, grown=grown,
               new_nnz=new_nnz, dropped=n - keep, grow=grow, keep=keep, pos=pos, w0=w0, grads=grads, g_new=g_new, score=score,
               hyper=hyper, desc=desc)
    plan.close(), fresh.close()
    return res


def test_errors(pkg, synth):
    codes = _codes()
    L = pkg.lib()
    desc = pkg.ConvDesc.from_shape(_shape(synth, "kh3_kw2"))
    D, n = rc.dense_size(desc), 50
    plan = cpu_plan(pkg, desc, _positions(desc, n, 41), sc.seeded_values(n, 42, np.float32))
    score = np.ones(D, np.float32)
    sp = score.ctypes.data

    def rewire(d, p=plan):
        return L.escoin_plan_rewire_cpu(p._h, None if d is None else C.byref(d), None, None, None, None)

    def drop(*a):
        return C.pointer(pkg.PruneDesc(*a))

    assert rewire(None) == codes["ESCOIN_EINVAL"]
    assert L.escoin_plan_rewire_cpu(None, C.byref(pkg.RewireDesc(None, 0, None, None)), None, None, None, None) == codes["ESCOIN_EINVAL"]
    assert rewire(pkg.RewireDesc(None, -1, sp, None)) == codes["ESCOIN_EINVAL"]
    assert rewire(pkg.RewireDesc(None, 1, None, None)) == codes["ESCOIN_EINVAL"]
    assert rewire(pkg.RewireDesc(drop(7, 1, 0.0, None), 1, sp, None)) == codes["ESCOIN_EINVAL"]
    assert rewire(pkg.RewireDesc(drop(pkg.PRUNE_KEEP, -1, 0.0, None), 1, sp, None)) == codes["ESCOIN_EINVAL"]
    assert rewire(pkg.RewireDesc(drop(pkg.PRUNE_THRESHOLD, 0, -1.0, None), 0, None, None)) == codes["ESCOIN_EINVAL"]
    assert rewire(pkg.RewireDesc(drop(pkg.PRUNE_THRESHOLD, 0, float("nan"), None), 0, None, None)) == codes["ESCOIN_EINVAL"]
    assert plan.nnz() == n and plan.stat("rewire_count") == 0         # a refused call changes nothing
    ok = pkg.RewireDesc(None, 3, sp, None)
    unaligned = pkg.Plan(desc)
    assert rewire(ok, unaligned) == codes["ESCOIN_ESTATE"]
    # D >= 2^31 is refused from the descriptor alone (the plan is only created: nothing of that size is ever allocated)
    huge = pkg.Plan(pkg.ConvDesc.from_shape(synth.shape("rewire_huge", 1, 16384, 1, 2, 65536, 1, KW=2)))
    assert rewire(pkg.RewireDesc(None, 0, None, None), huge) == codes["ESCOIN_EINVAL"]
    assert L.escoin_plan_rewire(huge._h, C.byref(pkg.RewireDesc(None, 0, None, None)), None, None, None, None, None) == codes["ESCOIN_EINVAL"]
    huge.close()
    # the device entry point: EINVAL for the descriptor first; then no device (here), or a plan without a device side
    assert L.escoin_plan_rewire(plan._h, None, None, None, None, None, None) == codes["ESCOIN_EINVAL"]
    assert L.escoin_plan_rewire(plan._h, C.byref(pkg.RewireDesc(None, -1, sp, None)), None, None, None, None, None) == codes["ESCOIN_EINVAL"]
    assert L.escoin_plan_rewire(plan._h, C.byref(pkg.RewireDesc(None, 1, None, None)), None, None, None, None, None) == codes["ESCOIN_EINVAL"]
    want = codes["ESCOIN_ENODEVICE"] if pkg.device_count() < 1 else codes["ESCOIN_ESTATE"]
    assert L.escoin_plan_rewire(plan._h, C.byref(ok), None, None, None, None, None) == want
    assert L.escoin_plan_rewire(unaligned._h, C.byref(ok), None, None, None, None, None) == want
    assert rewire(ok) == 0 and plan.nnz() == n + 3 and plan.stat("rewire_count") == 1
    plan.close(), unaligned.close()
