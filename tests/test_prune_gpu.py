"""escoin_plan_prune / escoin_compact_entries on the MI355X.  Every comparison is exact.  Two yardsticks: the entry map
against prune_common's numpy restatement of the rule, and the pruned plan against a fresh plan with the same options
aligned (set_csr) on the kept entries.  The oracle is consulted once per plan kind on top (<= 1e-4).  Plans of the
selection cases are built with set_csr, so that nnz is exact and explicit zeros, NaN and infinities are entries."""
import ctypes as C

import numpy as np
import pytest

import prune_common as pc
import solver_common as sc
from conftest import rel_err
from test_prune_host import continuity_cpu
from test_update_values_gpu import Layer, _mixed_weights, _oracle_forward
from upd_common import same_bits

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
TOL = 1e-4
DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def dev(pkg):
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        pytest.fail("no HIP device visible (these tests run on the MI355X)")
    return torch.device("cuda:0")


def _sel_desc(pkg, synth):
    """32 x 16 x 3 x 3 = 4608 positions on a 4 x 4 image: room for 3 T + 1 entries, an align that costs nothing."""
    return pkg.ConvDesc.from_shape(synth.shape("prune_sel", 1, 16, 4, 4, 32, 3, pad=1))


def _positions(desc, n, seed):
    total = desc.M * (desc.C // desc.group) * desc.KH * desc.KW
    return np.sort(np.random.RandomState(seed).permutation(total)[:n])


def gpu_plan(pkg, desc, positions, values, **opts):
    rp, ci, ng = pc.pattern_csr(desc, positions)
    plan = pkg.Plan(desc, **opts)
    plan.set_csr(rp, ci, values, ng)
    assert plan.nnz() == positions.size
    return plan


def check_pruned(plan, before, want_map, got_map):
    rp, ci, va, ng = before
    got = got_map.cpu().numpy()
    assert got.dtype == np.int32
    if not np.array_equal(got, want_map):
        bad = np.flatnonzero(got != want_map)
        print("map differs at %d of %d entries, first %d: got %d want %d" % (bad.size, got.size, bad[0], got[bad[0]], want_map[bad[0]]))
    assert np.array_equal(got, want_map)
    w_rp, w_ci, w_va, w_ng = pc.ref_csr(plan.desc, rp, ci, va, ng, want_map)
    g_rp, g_ci, g_va, g_ng = plan.get_csr()
    assert plan.nnz() == int((want_map >= 0).sum()) and plan.stat("prune_last_dropped") == int((want_map < 0).sum())
    assert np.array_equal(g_rp, w_rp) and np.array_equal(g_ci, w_ci) and same_bits(g_va, w_va) and np.array_equal(g_ng, w_ng)


SIZES = ["1", "2", "63", "64", "65", "T-1", "T", "T+1", "3T+1"]


def _size(tile, name):
    return {"T-1": tile - 1, "T": tile, "T+1": tile + 1, "3T+1": 3 * tile + 1}.get(name) or int(name)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("size", SIZES)
def test_device_selection_equals_the_host_rule(pkg, dev, synth, dt, size):
    """The entry map of every score case (prune_common.score_cases: ties of both signs across the boundary, +-0, NaN,
    +-inf, denormals, a deciding difference in each key byte in turn, all keys equal) at a tie boundary, by KEEP on the
    plan's values; then one THRESHOLD at an existing magnitude and one KEEP on a score array."""
    desc = _sel_desc(pkg, synth)
    probe = gpu_plan(pkg, desc, _positions(desc, 1, 1), np.ones(1, dt), kernel=pkg.KERNEL_GENERIC)
    tile = probe.stat("prune_tile_entries")
    probe.close()
    n = _size(tile, size)
    pos = _positions(desc, n, 100 + n)
    cases = pc.score_cases(n, dt, 200 + n)
    for name, score in cases.items():
        keep = pc.tie_boundary_keep(score, max(n // 2, 1) if n > 1 else 0)
        plan = gpu_plan(pkg, desc, pos, score, kernel=pkg.KERNEL_GENERIC)
        before = plan.get_csr()
        got = plan.prune(keep=keep)
        check_pruned(plan, before, pc.ref_map(score, keep=keep), got)
        assert plan.stat("prune_count") == 1
        plan.close()
    values = np.random.RandomState(300 + n).uniform(-1, 1, n).astype(dt)
    score = cases["ties"]
    plan = gpu_plan(pkg, desc, pos, score, kernel=pkg.KERNEL_GENERIC)
    before = plan.get_csr()
    thr = float(np.abs(score[n // 2]))
    check_pruned(plan, before, pc.ref_map(score, threshold=dt(thr)), plan.prune(threshold=thr))
    plan.close()
    for name in ("specials", "byte%d" % (np.dtype(dt).itemsize - 1)):
        plan = gpu_plan(pkg, desc, pos, values, kernel=pkg.KERNEL_GENERIC)
        before = plan.get_csr()
        keep = pc.tie_boundary_keep(cases[name], (n + 2) // 3)
        got = plan.prune(keep=keep, score=torch.from_numpy(cases[name]).to(dev))
        check_pruned(plan, before, pc.ref_map(cases[name], keep=keep), got)
        plan.close()


def test_more_tiles_than_the_scanning_workgroup_is_wide(pkg, dev, synth):
    """512 x 512 x 3 x 3 fully populated: 2304 tiles for a scanning workgroup of 256 lanes.  KEEP on a tie boundary that
    lies in the last tile: the ranks there carry the sums of every tile before it."""
    desc = pkg.ConvDesc.from_shape(synth.shape("prune_big", 1, 512, 4, 4, 512, 3, pad=1))
    n = 512 * 512 * 9
    rs = np.random.RandomState(5)
    mags = (np.arange(16, dtype=np.float32) + 1) / 16
    score = (mags[rs.randint(0, 16, n)] * rs.choice(np.array([-1, 1], np.float32), n)).astype(np.float32)
    plan = gpu_plan(pkg, desc, np.arange(n), score, kernel=pkg.KERNEL_GENERIC)
    tile = plan.stat("prune_tile_entries")
    tiles = (n + tile - 1) // tile
    assert tiles > 256
    k = pc.keys(score)
    t_key = pc.keys(mags[7:8])[0]
    eq = np.flatnonzero(k == t_key)
    in_last = int((eq >= (tiles - 1) * tile).sum())
    assert in_last >= 4
    keep = int((k > t_key).sum()) + eq.size - in_last // 2
    want = pc.ref_map(score, keep=keep)
    dropped_ties = eq[want[eq] < 0]
    assert dropped_ties.size == in_last // 2 and dropped_ties.min() >= (tiles - 1) * tile        # the boundary is in the last tile
    before = plan.get_csr()
    got = plan.prune(keep=keep)
    check_pruned(plan, before, want, got)
    plan.close()


def _kinds(pkg, synth):
    """id -> (shape, Layer options, check(plan) before the prune)"""
    K = pkg
    res5 = synth.resnet50_3x3(N=2)[3]
    res4 = synth.resnet50_3x3(N=2)[2]
    goog = synth.shape("goog14", 3, 480, 14, 14, 192, 1, sparsity=0.95)
    grouped = synth.shape("mixed_g2", 2, 64, 14, 14, 64, 3, pad=1, group=2, sparsity=0.7)
    stat = lambda key, val: (lambda p: p.stat(key) == val)
    return {
        "generic": (synth.lenet_conv2(N=2)[0], dict(kernel=K.KERNEL_GENERIC), stat("kernel_choice", K.KERNEL_GENERIC)),
        "tiled": (res5, dict(kernel=K.KERNEL_TILED, tiling_batch=256), stat("kernel_choice", K.KERNEL_TILED)),
        "jit_lines_3x3": (res5, dict(kernel=K.KERNEL_JIT, tiling_batch=256),
                          lambda p: p.stat("kernel_choice") == K.KERNEL_JIT and p.stat("code_direct") == 1 and "jit" in p.kernel_name),
        "jit_literals_1x1": (goog, dict(kernel=K.KERNEL_JIT, tiling_batch=256),
                             lambda p: p.stat("kernel_choice") == K.KERNEL_JIT and p.stat("code_direct") == 1),
        "dense": (res4, dict(kernel=K.KERNEL_DENSE), stat("kernel_choice", K.KERNEL_DENSE)),
        "mixed_groups": (grouped, dict(dense_threshold_pct=30, tiling_batch=256, w="mixed"),
                         lambda p: " + " in p.kernel_name and p.stat("kernel_choice") == K.KERNEL_JIT),
        "lowered_sparse": (res5, dict(conv_mode=K.CONV_MODE_LOWERED_SPARSE, tiling_batch=256),
                           lambda p: "lowered" in p.kernel_name or "csrmm" in p.kernel_name),
        "double": (synth.alexnet(N=2)[1], dict(dt=np.float64), lambda p: p.stat("is_f64") == 1 and "f64" in p.kernel_name),
    }


KIND_IDS = ["generic", "tiled", "jit_lines_3x3", "jit_literals_1x1", "dense", "mixed_groups", "lowered_sparse", "double"]


def _layer(pkg, dev, synth, kind, seed):
    s, opts, check = _kinds(pkg, synth)[kind]
    opts = dict(opts)
    if opts.get("w") == "mixed":
        opts["w"] = _mixed_weights(s, 5)
    layer = Layer(pkg, dev, synth, s, seed, **opts)
    assert check(layer.plan), (layer.plan.kernel_name, layer.plan.tiling_info)
    return layer


def _fresh(layer, csr):
    p = layer.pkg.Plan(layer.desc, **layer.opts)
    p.set_csr(*csr)
    return p


@pytest.mark.parametrize("kind", KIND_IDS)
def test_a_pruned_plan_equals_a_fresh_plan(pkg, dev, synth, oracle, kind):
    """One layer per plan kind: a forward (the caches hold the old code and weights), half of the entries pruned, then
    kernel, tiling and the forward's bits against a fresh set_csr plan on the kept entries; the same after a second prune."""
    layer = _layer(pkg, dev, synth, kind, 40)
    plan = layer.plan
    layer.forward()
    for rnd, frac in enumerate((0.5, 0.6)):
        before = plan.get_csr()
        keep = int(plan.nnz() * frac)
        got = plan.prune(keep=keep)
        want = pc.ref_map(before[2], keep=keep)
        check_pruned(plan, before, want, got)
        kept_csr = pc.ref_csr(plan.desc, *before, want)
        ref = _fresh(layer, kept_csr)
        assert ref.kernel_name == plan.kernel_name and ref.tiling_info == plan.tiling_info
        assert ref.stat("kernel_choice") == plan.stat("kernel_choice")
        top = layer.forward()
        assert np.array_equal(top, layer.forward(ref)), (kind, plan.kernel_name)
        w_kept = pc.masked_dense(plan.desc, *kept_csr)
        err = rel_err(top, _oracle_forward(oracle, layer.s, layer.x, w_kept, layer.b, layer.relu, layer.dt))
        print("%s prune %d via %s: vs fresh plan equal, vs oracle rel_err=%.3g" % (kind, rnd, plan.kernel_name, err))
        assert err <= (1e-12 if layer.dt == np.float64 else TOL)
        ref.close()
    assert plan.stat("prune_count") == 2
    plan.close()


@pytest.mark.parametrize("kind", ["generic", "jit_lines_3x3", "double"])
def test_backward_after_a_prune_equals_a_fresh_plan(pkg, dev, synth, kind):
    layer = _layer(pkg, dev, synth, kind, 41)
    plan = layer.plan
    td = torch.from_numpy(np.random.RandomState(42).uniform(-1, 1, (layer.s.N, layer.s.M) + tuple(plan.out_hw)).astype(layer.dt)).to(dev)
    plan.backward(td, bottom=layer.xd, values_diff=True)          # the backward state of the old pattern exists ...
    assert plan.stat("bwd_device_bytes") > 0
    before = plan.get_csr()
    keep = plan.nnz() // 3
    got = plan.prune(keep=keep)
    assert plan.stat("bwd_device_bytes") == 0                       # ... and is dropped, as on any align
    want = pc.ref_map(before[2], keep=keep)
    check_pruned(plan, before, want, got)
    ref = _fresh(layer, pc.ref_csr(plan.desc, *before, want))
    a = plan.backward(td, bottom=layer.xd, values_diff=True, bias_diff=True)
    b = ref.backward(td, bottom=layer.xd, values_diff=True, bias_diff=True)
    torch.cuda.synchronize()
    assert a[1].numel() == keep
    for x, y in zip(a, b):
        assert same_bits(x.cpu().numpy(), y.cpu().numpy())
    assert float(a[0].abs().max()) > 0 and float(a[1].abs().max()) > 0
    plan.close(), ref.close()


@pytest.mark.parametrize("kind", ["generic", "jit_lines_3x3"])
def test_the_values_on_the_device_are_the_ones_ranked(pkg, dev, synth, kind):
    """A device-source solver step on one stream (behind work that keeps it busy), no host read, and at once a prune on
    another stream: the map is the rule's on the values the step leaves, not on the host's stale copy."""
    layer = _layer(pkg, dev, synth, kind, 43)
    plan = layer.plan
    w0 = plan.get_csr()[2].copy()
    n = w0.size
    g = sc.seeded_values(n, 44, np.float32, zeros=False)
    hyper = dict(type=sc.SGD, rate=0.75, momentum=0.9)
    w1, _, _ = sc.step(w0, g, np.zeros(n, np.float32), None, **hyper)
    keep = n // 2
    want = pc.ref_map(w1, keep=keep)
    assert not np.array_equal(want, pc.ref_map(w0, keep=keep))       # the stale values would give another map
    gd, h = torch.from_numpy(g).to(dev), torch.zeros(n, dtype=torch.float32, device=dev)
    busy = torch.empty((4096, 4096), dtype=torch.float32, device=dev).normal_()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        for _ in range(4):
            busy = busy @ busy
            busy = busy / busy.abs().max()
        plan.solver_step(gd, h, None, **hyper)
    with torch.cuda.stream(s2):
        got = plan.prune(keep=keep)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    values = plan.get_csr()[2]                                          # read back at the end: the new values, compacted
    assert same_bits(values, w1[want >= 0])
    plan.close()


@pytest.mark.parametrize("rule,dt", [("sgd", np.float32), ("adam", np.float32), ("adam", np.float64)], ids=["sgd-f32", "adam-f32", "adam-f64"])
def test_training_continues_on_the_device(pkg, dev, synth, rule, dt):
    """The CPU test's sequence with device arrays and compact_entries on the device: bit-equal to a fresh plan given
    numpy-compacted histories, and to the CPU twin's result."""
    cpu = continuity_cpu(pkg, synth, dt, rule)
    desc, pos, grads, hyper, keep = cpu["desc"], cpu["pos"], cpu["grads"], cpu["hyper"], cpu["keep"]
    n = pos.size
    adam = rule == "adam"
    tdt = torch.float64 if dt == np.float64 else torch.float32
    plan = gpu_plan(pkg, desc, pos, cpu["w0"])
    h = torch.zeros(n, dtype=tdt, device=dev)
    h2 = torch.zeros(n, dtype=tdt, device=dev) if adam else None
    for k in range(2):
        plan.solver_step(torch.from_numpy(grads[k]).to(dev), h, h2, **hyper)
    entry_map = plan.prune(keep=keep)
    assert np.array_equal(entry_map.cpu().numpy(), cpu["map"])
    h_new = pkg.compact_entries(entry_map, h)
    h2_new = pkg.compact_entries(entry_map, h2) if adam else None
    g_new = pkg.compact_entries(entry_map, torch.from_numpy(grads[2]).to(dev))
    torch.cuda.synchronize()
    kept = cpu["map"] >= 0
    h_np, h2_np = h.cpu().numpy(), (h2.cpu().numpy() if adam else None)
    assert same_bits(h_new.cpu().numpy(), h_np[kept]) and np.any(h_np[kept] != 0) and same_bits(g_new.cpu().numpy(), grads[2][kept])
    # the fresh plan on the kept entries, numpy-compacted histories
    rp, ci, va, ng = plan.get_csr()
    fresh = pkg.Plan(desc)
    fresh.set_csr(rp, ci, va, ng)
    fh = torch.from_numpy(h_np[kept].copy()).to(dev)
    fh2 = torch.from_numpy(h2_np[kept].copy()).to(dev) if adam else None
    plan.solver_step(g_new, h_new, h2_new, **hyper)
    fresh.solver_step(torch.from_numpy(grads[2][kept].copy()).to(dev), fh, fh2, **hyper)
    torch.cuda.synchronize()
    out, want = plan.get_csr(), fresh.get_csr()
    assert all(same_bits(a, b) for a, b in zip(out, want))
    assert same_bits(h_new.cpu().numpy(), fh.cpu().numpy()) and (not adam or same_bits(h2_new.cpu().numpy(), fh2.cpu().numpy()))
    # the CPU twin
    assert same_bits(out[2], cpu["values"]) and same_bits(h_new.cpu().numpy(), cpu["h"])
    assert not adam or same_bits(h2_new.cpu().numpy(), cpu["h2"])
    plan.close(), fresh.close()


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["4B", "8B"])
def test_compact_entries_in_a_graph(pkg, dev, dt):
    n, keep = 5000, 1777
    rs = np.random.RandomState(61)
    m_np = pc.ref_map(rs.uniform(-1, 1, n).astype(np.float32), keep=keep)
    entry_map = torch.from_numpy(m_np).to(dev)
    src = torch.empty(n, dtype=dt, device=dev)
    out = torch.empty(keep + 3, dtype=dt, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pkg.compact_entries(entry_map, src, out=out)                  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pkg.compact_entries(entry_map, src, out=out)
    results = []
    for rnd in range(2):
        vals = rs.uniform(-1, 1, n)
        src.copy_(torch.from_numpy(vals).to(dev))
        want = src.cpu().numpy()[m_np >= 0]
        out.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert same_bits(got[:keep], want) and np.all(got[keep:] == 7), rnd
        results.append(got)
    assert not np.array_equal(results[0], results[1])
    # the same replay on the same input: the same bits
    out.fill_(7)
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy(), results[1])


def test_accounting_and_three_prunes_in_a_row(pkg, dev, synth):
    """workspace_bytes after prune, forward, backward and update equals the fresh plan's after the same calls (nothing of
    the old alignment or of the prune's workspace stays); the stats; 90 %, 95 %, 97 % one after the other."""
    s = synth.resnet50_3x3(N=2, sparsity=0.8)[3]
    layer = Layer(pkg, dev, synth, s, 70, tiling_batch=256)
    plan = layer.plan
    td = torch.from_numpy(np.random.RandomState(71).uniform(-1, 1, (s.N, s.M) + tuple(plan.out_hw)).astype(np.float32)).to(dev)

    def use(p):
        top = p.forward(layer.xd, layer.bd)
        bd, vd, _ = p.backward(td, bottom=layer.xd, values_diff=True)
        p.set_values(torch.from_numpy(p.get_csr()[2]).to(dev))
        torch.cuda.synchronize()
        return top.cpu().numpy(), bd.cpu().numpy(), vd.cpu().numpy()

    use(plan)
    total = s.M * (s.C // s.group) * s.KH * s.KW
    for k, sparsity in enumerate((0.90, 0.95, 0.97)):
        before = plan.get_csr()
        got = plan.prune(sparsity=sparsity)
        keep = int(round((1 - sparsity) * total))
        want = pc.ref_map(before[2], keep=keep)
        check_pruned(plan, before, want, got)
        assert plan.stat("prune_count") == k + 1 and plan.stat("prune_last_dropped") == before[2].size - keep
        assert plan.stat("bwd_device_bytes") == 0 and plan.stat("upd_device_bytes") == 0
        ref = _fresh(layer, pc.ref_csr(plan.desc, *before, want))
        assert plan.workspace_bytes == ref.workspace_bytes
        a, b = use(plan), use(ref)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        assert plan.workspace_bytes == ref.workspace_bytes and ref.kernel_name == plan.kernel_name
        ref.close()
    # nothing dropped: the states stay, the map is the identity
    ws, align_us = plan.workspace_bytes, plan.stat("align_us")
    got = plan.prune(keep=plan.nnz() + 5)
    assert np.array_equal(got.cpu().numpy(), np.arange(plan.nnz(), dtype=np.int32))
    assert plan.stat("prune_last_dropped") == 0 and plan.stat("prune_count") == 4
    assert plan.workspace_bytes == ws and plan.stat("align_us") == align_us and plan.stat("upd_device_bytes") > 0
    plan.close()


@pytest.mark.parametrize("kind", ["generic", "jit_lines_3x3", "double"])
def test_everything_dropped_is_set_csr_on_an_empty_csr(pkg, dev, synth, kind):
    """keep = 0: the plan is what escoin_plan_set_csr leaves on an empty CSR -- aligned, nnz 0, and its forward writes the
    bias (0 without one)."""
    layer = _layer(pkg, dev, synth, kind, 80)
    plan = layer.plan
    before = plan.get_csr()
    got = plan.prune(keep=0)
    assert np.all(got.cpu().numpy() == -1) and plan.nnz() == 0 and plan.stat("prune_last_dropped") == before[2].size
    ref = _fresh(layer, pc.ref_csr(plan.desc, *before, np.full(before[2].size, -1, np.int32)))
    assert ref.nnz() == 0 and ref.kernel_name == plan.kernel_name and ref.tiling_info == plan.tiling_info
    top = layer.forward()
    assert np.array_equal(top, layer.forward(ref))
    b = np.zeros(layer.s.M, layer.dt) if layer.b is None else layer.b
    assert np.array_equal(top, np.broadcast_to(b[None, :, None, None], top.shape))
    assert plan.prune(keep=0).numel() == 0 and plan.stat("prune_last_dropped") == 0      # the empty plan again: a no-op
    plan.close(), ref.close()


def test_device_errors(pkg, dev, synth):
    L = pkg.lib()
    desc = _sel_desc(pkg, synth)
    n = 100
    plan = gpu_plan(pkg, desc, _positions(desc, n, 91), sc.seeded_values(n, 92, np.float32), kernel=pkg.KERNEL_GENERIC)
    EINVAL, ESTATE = -1, -4
    m = torch.empty(n, dtype=torch.int32, device=dev)

    def prune(d, p=plan):
        return L.escoin_plan_prune(p._h, None if d is None else C.byref(d), C.c_void_p(m.data_ptr()), None, None)

    assert prune(None) == EINVAL
    assert prune(pkg.PruneDesc(2, 1, 0.0, None)) == EINVAL
    assert prune(pkg.PruneDesc(pkg.PRUNE_KEEP, -1, 0.0, None)) == EINVAL
    assert prune(pkg.PruneDesc(pkg.PRUNE_THRESHOLD, 0, -1.0, None)) == EINVAL
    assert prune(pkg.PruneDesc(pkg.PRUNE_THRESHOLD, 0, float("nan"), None)) == EINVAL
    assert plan.nnz() == n and plan.stat("prune_count") == 0
    ok = pkg.PruneDesc(pkg.PRUNE_KEEP, 5, 0.0, None)
    unaligned = pkg.Plan(desc)
    assert prune(ok, unaligned) == ESTATE
    host_only = pkg.Plan(desc)
    host_only.weight_align_cpu(np.ones((desc.M, desc.C, desc.KH, desc.KW), np.float32))
    assert prune(ok, host_only) == ESTATE
    assert L.escoin_plan_prune_cpu(plan._h, C.byref(ok), None, None) == ESTATE       # _cpu on a device-aligned plan
    # NULL map and NULL new_nnz on the device entry point
    new_nnz = C.c_long(-1)
    assert L.escoin_plan_prune(plan._h, C.byref(ok), None, C.byref(new_nnz), None) == 0 and new_nnz.value == 5 and plan.nnz() == 5
    src = torch.zeros(n, dtype=torch.float32, device=dev)
    p = C.c_void_p(src.data_ptr())
    assert L.escoin_compact_entries(C.c_void_p(m.data_ptr()), n, 4, p, p, 1, None) == EINVAL
    assert L.escoin_compact_entries(C.c_void_p(m.data_ptr()), n, 3, p, p, 1, None) == EINVAL
    plan.close(), unaligned.close(), host_only.close()
