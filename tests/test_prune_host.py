"""escoin_plan_prune_cpu / escoin_compact_entries without a GPU: plans aligned by weight_align_cpu, float and double.
Every comparison is exact: the feature is a selection and a re-index.  The yardstick is prune_common's numpy restatement
of the rule (a stable sort on the integer keys); the library's host code selects without a sort."""
import ctypes as C

import numpy as np
import pytest

import prune_common as pc
import solver_common as sc
from upd_common import same_bits

DTYPES = [np.float32, np.float64]
HYPER = dict(rate=0.01, momentum=0.9, momentum2=0.999, delta=1e-8, decay=5e-4)


def _codes():
    import os
    import re
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(here, "include", "escoin.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (ESCOIN_E\w+) \(?(-?\d+)\)?", text)}


def _shape(synth, kind):
    if kind == "plain":
        return synth.shape("prune_plain", 2, 8, 6, 6, 12, 3, pad=1, sparsity=0.5)
    if kind == "group2":
        return synth.shape("prune_g2", 2, 16, 6, 6, 12, 3, pad=1, group=2, sparsity=0.5)
    return synth.shape("prune_dw", 2, 8, 6, 6, 8, 3, pad=1, group=8, sparsity=0.5)


def _positions(desc, n, seed):
    total = desc.M * (desc.C // desc.group) * desc.KH * desc.KW
    return np.sort(np.random.RandomState(seed).permutation(total)[:n])


def cpu_plan(pkg, desc, positions, values):
    """A host-aligned plan whose CSR holds exactly `positions` with `values` (explicit zeros, NaN, ... included): aligned
    on ones, then updated in place."""
    w = np.zeros(desc.M * (desc.C // desc.group) * desc.KH * desc.KW, values.dtype)
    w[positions] = 1
    shape = (desc.M, desc.C // desc.group, desc.KH, desc.KW)
    plan = pkg.Plan(desc)
    plan.weight_align_cpu(w.reshape(shape))
    w[positions] = values
    plan.update_values_cpu(w.reshape(shape))
    assert plan.nnz() == positions.size and same_bits(plan.get_csr()[2], values)
    return plan


def check_pruned(plan, before, want_map, got_map):
    """The map, the new nnz and the plan's CSR against the reference."""
    rp, ci, va, ng = before
    assert got_map.dtype == np.int32 and np.array_equal(got_map, want_map)
    w_rp, w_ci, w_va, w_ng = pc.ref_csr(plan.desc, rp, ci, va, ng, want_map)
    g_rp, g_ci, g_va, g_ng = plan.get_csr()
    assert plan.nnz() == int((want_map >= 0).sum())
    assert np.array_equal(g_rp, w_rp) and np.array_equal(g_ci, w_ci) and same_bits(g_va, w_va) and np.array_equal(g_ng, w_ng)
    assert plan.stat("prune_last_dropped") == int((want_map < 0).sum())


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["plain", "group2", "depthwise"])
def test_keep_equals_the_reference_rule(pkg, synth, dt, kind):
    desc = pkg.ConvDesc.from_shape(_shape(synth, kind))
    n = 600 if kind != "depthwise" else 60
    pos = _positions(desc, n, 3)
    for name, score in pc.score_cases(n, dt, 7).items():
        tie = pc.tie_boundary_keep(score, n // 2)
        for keep in (0, 1, tie, n - 1, n, n + 5):
            plan = cpu_plan(pkg, desc, pos, score)
            before = plan.get_csr()
            got = plan.prune_cpu(keep=keep)
            want = pc.ref_map(score, keep=keep)
            assert int((want >= 0).sum()) == min(keep, n)
            check_pruned(plan, before, want, got)
            assert plan.stat("prune_count") == 1, (name, keep)
            plan.close()


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_threshold_and_score_array(pkg, synth, dt):
    desc = pkg.ConvDesc.from_shape(_shape(synth, "group2"))
    n = 500
    pos = _positions(desc, n, 4)
    cases = pc.score_cases(n, dt, 8)
    for name, score in cases.items():
        finite = np.abs(score[np.isfinite(score)])
        thresholds = [0.0, float(np.median(finite)), float(finite.max()), float(np.nextafter(dt(np.median(finite)), dt(np.inf))), np.inf]
        for thr in thresholds:
            plan = cpu_plan(pkg, desc, pos, score)
            before = plan.get_csr()
            got = plan.prune_cpu(threshold=thr)
            want = pc.ref_map(score, threshold=dt(thr))
            check_pruned(plan, before, want, got)
            if thr == 0.0:
                assert (want >= 0).all() and plan.stat("prune_last_dropped") == 0
            plan.close()
    # a score array decides instead of the values (which then only travel); a negative score ranks by its magnitude
    values = np.random.RandomState(9).uniform(-1, 1, n).astype(dt)
    for name in ("ties", "specials", "byte0"):
        plan = cpu_plan(pkg, desc, pos, values)
        before = plan.get_csr()
        keep = pc.tie_boundary_keep(cases[name], n // 3)
        got = plan.prune_cpu(keep=keep, score=cases[name])
        check_pruned(plan, before, pc.ref_map(cases[name], keep=keep), got)
        plan.close()


def test_sparsity_is_a_keep_count_over_the_dense_size(pkg, synth):
    desc = pkg.ConvDesc.from_shape(_shape(synth, "plain"))
    total = desc.M * desc.C * desc.KH * desc.KW
    n = 700
    score = np.random.RandomState(1).uniform(-1, 1, n).astype(np.float32)
    plan = cpu_plan(pkg, desc, _positions(desc, n, 5), score)
    got = plan.prune_cpu(sparsity=0.9)
    keep = int(round(0.1 * total))
    assert np.array_equal(got, pc.ref_map(score, keep=keep)) and plan.nnz() == keep
    with pytest.raises(pkg.EscoinError):
        plan.prune_cpu(keep=3, sparsity=0.5)
    plan.close()


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_nothing_dropped_leaves_the_plan_untouched(pkg, synth, dt):
    desc = pkg.ConvDesc.from_shape(_shape(synth, "plain"))
    n = 300
    score = pc.score_cases(n, dt, 2)["specials"]
    plan = cpu_plan(pkg, desc, _positions(desc, n, 6), score)
    before, align_us = plan.get_csr(), plan.stat("align_us")
    for kw in (dict(keep=n), dict(keep=n + 5), dict(threshold=0.0)):
        got = plan.prune_cpu(**kw)
        assert np.array_equal(got, np.arange(n, dtype=np.int32))
        assert plan.stat("prune_last_dropped") == 0 and plan.stat("align_us") == align_us
        after = plan.get_csr()
        assert all(same_bits(a, b) for a, b in zip(before, after))
    assert plan.stat("prune_count") == 3
    # NULL map and NULL new_nnz are allowed; new_nnz reports the kept count
    d = pkg.PruneDesc(pkg.PRUNE_KEEP, 10, 0.0, None)
    new_nnz = C.c_long(-1)
    assert pkg.lib().escoin_plan_prune_cpu(plan._h, C.byref(d), None, C.byref(new_nnz)) == 0 and new_nnz.value == 10
    assert pkg.lib().escoin_plan_prune_cpu(plan._h, C.byref(d), None, None) == 0 and plan.nnz() == 10
    plan.close()


def _inputs(s, dt, seed):
    rs = np.random.RandomState(seed)
    x = rs.uniform(-1, 1, (s.N, s.C, s.H, s.W)).astype(dt)
    b = rs.uniform(-1, 1, s.M).astype(dt)
    return x, b


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["plain", "group2"])
def test_forward_and_backward_equal_a_fresh_plan(pkg, synth, dt, kind):
    """forward_cpu / backward_cpu after a prune against a plan aligned by weight_align_cpu on the masked weights."""
    s = _shape(synth, kind)
    desc = pkg.ConvDesc.from_shape(s)
    n = 500
    score = np.random.RandomState(11).uniform(-1, 1, n).astype(dt)
    score[score == 0] = 0.5
    plan = cpu_plan(pkg, desc, _positions(desc, n, 12), score)
    x, b = _inputs(s, dt, 13)
    plan.forward_cpu(x, b)                       # (the offsets of the old pattern exist when the prune comes)
    plan.prune_cpu(keep=n // 4)
    fresh = pkg.Plan(desc)
    fresh.weight_align_cpu(pc.masked_dense(desc, *plan.get_csr()))
    assert all(same_bits(a, c) for a, c in zip(plan.get_csr(), fresh.get_csr()))
    top, want_top = plan.forward_cpu(x, b), fresh.forward_cpu(x, b)
    assert same_bits(top, want_top) and np.abs(top).max() > 0
    td = np.random.RandomState(14).uniform(-1, 1, top.shape).astype(dt)
    got = plan.backward_cpu(td, bottom=x, values_diff=True, bias_diff=True)
    want = fresh.backward_cpu(td, bottom=x, values_diff=True, bias_diff=True)
    assert all(same_bits(a, c) for a, c in zip(got, want))
    plan.close(), fresh.close()


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("rule", ["sgd", "nesterov", "adam"])
def test_training_continues_with_compacted_histories(pkg, synth, dt, rule):
    """Two solver steps, a prune, compact_entries over the histories, one more step: equal, bit for bit, to the same step
    on a fresh plan given numpy-compacted histories."""
    got = continuity_cpu(pkg, synth, dt, rule)
    assert got["new_nnz"] == got["keep"]


def continuity_cpu(pkg, synth, dt, rule):
    """The sequence of the test above; returns what its device twin (test_prune_gpu.py) compares with."""
    desc = pkg.ConvDesc.from_shape(_shape(synth, "group2"))
    n, keep = 500, 137
    hyper = dict(HYPER, type=sc.RULES[rule], regularization=sc.REG_L2)
    w0 = sc.seeded_values(n, 21, dt, zeros=False)
    pos = _positions(desc, n, 22)
    plan = cpu_plan(pkg, desc, pos, w0)
    adam = rule == "adam"
    h, h2 = np.zeros(n, dt), (np.zeros(n, dt) if adam else None)
    grads = [sc.seeded_values(n, 23 + k, dt) for k in range(3)]
    for k in range(2):
        plan.solver_step_cpu(grads[k].copy(), h, h2, **hyper)
    w2 = plan.get_csr()[2].copy()
    entry_map = plan.prune_cpu(keep=keep)
    assert np.array_equal(entry_map, pc.ref_map(w2, keep=keep))
    kept = entry_map >= 0
    h_new = pkg.compact_entries(entry_map, h)
    h2_new = pkg.compact_entries(entry_map, h2) if adam else None
    g_new = pkg.compact_entries(entry_map, grads[2])
    assert same_bits(h_new, h[kept]) and same_bits(g_new, grads[2][kept]) and (not adam or same_bits(h2_new, h2[kept]))
    assert np.any(h_new != 0)                     # compacted, not cleared
    # the fresh plan: aligned on the kept entries, numpy-compacted histories
    rp, ci, va, ng = plan.get_csr()
    fresh = cpu_plan(pkg, desc, pos[kept], w2[kept])
    fh, fh2, fg = h[kept].copy(), (h2[kept].copy() if adam else None), grads[2][kept].copy()
    plan.solver_step_cpu(g_new, h_new, h2_new, **hyper)
    fresh.solver_step_cpu(fg, fh, fh2, **hyper)
    out, want = plan.get_csr(), fresh.get_csr()
    assert all(same_bits(a, c) for a, c in zip(out, want))
    assert same_bits(h_new, fh) and (not adam or same_bits(h2_new, fh2))
    # ... and the restatement agrees with both
    w3, wh, wh2 = sc.step(w2[kept], grads[2][kept], h[kept], h2[kept] if adam else None, **hyper)
    assert same_bits(out[2], w3) and same_bits(h_new, wh)
    res = dict(values=out[2].copy(), h=h_new.copy(), h2=None if h2_new is None else h2_new.copy(), map=entry_map,
               new_nnz=plan.nnz(), keep=keep, pos=pos, w0=w0, grads=grads, hyper=hyper, desc=desc)
    plan.close(), fresh.close()
    return res


@pytest.mark.parametrize("elem", [np.float32, np.float64, np.int32])
def test_compact_entries_on_the_host(pkg, elem):
    n = 1000
    rs = np.random.RandomState(31)
    entry_map = pc.ref_map(rs.uniform(-1, 1, n).astype(np.float32), keep=333)
    src = rs.uniform(-100, 100, n).astype(elem)
    out = np.full(400, 7, elem)
    got = pkg.compact_entries(entry_map, src, out=out)
    assert got is out and same_bits(out[:333], src[entry_map >= 0]) and np.all(out[333:] == 7)
    assert same_bits(pkg.compact_entries(entry_map, src), src[entry_map >= 0])
    assert pkg.compact_entries(np.zeros(0, np.int32), np.zeros(0, elem)).size == 0


def test_errors(pkg, synth):
    codes = _codes()
    L = pkg.lib()
    desc = pkg.ConvDesc.from_shape(_shape(synth, "plain"))
    n = 50
    plan = cpu_plan(pkg, desc, _positions(desc, n, 41), sc.seeded_values(n, 42, np.float32))
    m = np.zeros(n, np.int32)
    mp = m.ctypes.data_as(C.c_void_p)

    def prune(d, p=plan):
        return L.escoin_plan_prune_cpu(p._h, None if d is None else C.byref(d), mp, None)

    assert prune(None) == codes["ESCOIN_EINVAL"]
    assert prune(pkg.PruneDesc(7, 1, 0.0, None)) == codes["ESCOIN_EINVAL"]
    assert prune(pkg.PruneDesc(pkg.PRUNE_KEEP, -1, 0.0, None)) == codes["ESCOIN_EINVAL"]
    assert prune(pkg.PruneDesc(pkg.PRUNE_THRESHOLD, 0, -1.0, None)) == codes["ESCOIN_EINVAL"]
    assert prune(pkg.PruneDesc(pkg.PRUNE_THRESHOLD, 0, -0.0, None)) == codes["ESCOIN_EINVAL"]
    assert prune(pkg.PruneDesc(pkg.PRUNE_THRESHOLD, 0, float("nan"), None)) == codes["ESCOIN_EINVAL"]
    assert plan.nnz() == n and plan.stat("prune_count") == 0        # a refused call changes nothing
    unaligned = pkg.Plan(desc)
    ok = pkg.PruneDesc(pkg.PRUNE_KEEP, 5, 0.0, None)
    assert prune(ok, unaligned) == codes["ESCOIN_ESTATE"]
    # the device entry point: EINVAL for the descriptor first; then no device (here), or a plan without a device side
    assert L.escoin_plan_prune(plan._h, None, None, None, None) == codes["ESCOIN_EINVAL"]
    want = codes["ESCOIN_ENODEVICE"] if pkg.device_count() < 1 else codes["ESCOIN_ESTATE"]
    assert L.escoin_plan_prune(plan._h, C.byref(ok), None, None, None) == want
    assert L.escoin_plan_prune(unaligned._h, C.byref(ok), None, None, None) == want
    # compact_entries
    src, dst = np.zeros(n, np.float32), np.zeros(n, np.float32)
    sp, dp = src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p)
    assert L.escoin_compact_entries(mp, n, 2, sp, dp, 0, None) == codes["ESCOIN_EINVAL"]
    assert L.escoin_compact_entries(mp, n, 16, sp, dp, 0, None) == codes["ESCOIN_EINVAL"]
    assert L.escoin_compact_entries(mp, -1, 4, sp, dp, 0, None) == codes["ESCOIN_EINVAL"]
    assert L.escoin_compact_entries(mp, n, 4, sp, sp, 0, None) == codes["ESCOIN_EINVAL"]
    assert L.escoin_compact_entries(mp, n, 4, sp, dp, 0, None) == 0
    if pkg.device_count() < 1:
        assert L.escoin_compact_entries(mp, n, 4, sp, dp, 1, None) == codes["ESCOIN_ENODEVICE"]
    assert plan.stat("prune_tile_entries") >= 64 and plan.stat("prune_tile_entries") % 64 == 0
    plan.close(), unaligned.close()


def test_everything_dropped_leaves_an_empty_aligned_plan(pkg, synth):
    """keep = 0 on a host-aligned plan: what weight_align_cpu leaves on all-zero weights -- nnz 0, forward = bias."""
    s = _shape(synth, "group2")
    desc = pkg.ConvDesc.from_shape(s)
    n = 200
    plan = cpu_plan(pkg, desc, _positions(desc, n, 51), sc.seeded_values(n, 52, np.float32, zeros=False))
    got = plan.prune_cpu(keep=0)
    assert np.all(got == -1) and plan.nnz() == 0 and plan.stat("prune_last_dropped") == n
    x, b = _inputs(s, np.float32, 53)
    fresh = pkg.Plan(desc)
    fresh.weight_align_cpu(np.zeros((desc.M, desc.C // desc.group, desc.KH, desc.KW), np.float32))
    top = plan.forward_cpu(x, b)
    assert same_bits(top, fresh.forward_cpu(x, b)) and np.array_equal(top, np.broadcast_to(b[None, :, None, None], top.shape))
    # pruning the empty plan again is a no-op
    assert plan.prune_cpu(keep=0).size == 0 and plan.stat("prune_last_dropped") == 0
    plan.close(), fresh.close()
