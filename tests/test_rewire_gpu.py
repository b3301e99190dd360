"""escoin_plan_rewire on the MI355X.  Every comparison is exact.  Two yardsticks: both maps against rewire_common's numpy
restatement of the rule, and the rewired plan against a fresh plan with the same options aligned (set_csr) on the new
CSR.  The shapes are the smallest at which each kernel can go wrong (tile sizes read from csrc/prune_rules.h); images are
2 x 2 to 4 x 4 pixels, so an align costs next to nothing."""
import ctypes as C
import functools

import numpy as np
import pytest

import prune_common as pc
import rewire_common as rc
import solver_common as sc
from test_prune_gpu import _fresh, _layer, gpu_plan
from test_rewire_host import continuity_cpu
from upd_common import same_bits

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
DTYPES = {"f32": np.float32, "f64": np.float64}
TILE, SCAN_WIDTH, MAX_GRID = rc.tile_positions()


@pytest.fixture(scope="module")
def dev(pkg):
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        pytest.fail("no HIP device visible (these tests run on the MI355X)")
    return torch.device("cuda:0")


def _shapes(synth):
    """id -> (shape, density): D = 63, 64, 65 (partial and whole wave), 1025 (tile edge), 1152 (groups, a row boundary inside
    a tile), 262 656 (257 tiles: more than the scanning workgroup's step, last tile partial), 2 354 688 (more tiles than
    the grid cap: the grid-stride loops)."""
    S = synth.shape
    return {
        "D63": (S("rw63", 1, 9, 2, 2, 7, 1), 0.3),
        "D64": (S("rw64", 1, 8, 2, 2, 8, 1), 0.3),
        "D65": (S("rw65", 1, 13, 2, 2, 5, 1), 0.3),
        "D1025": (S("rw1025", 2, 41, 3, 3, 25, 1), 0.3),
        "D1152": (S("rw1152", 2, 24, 4, 4, 16, 3, KW=2, pad=1, group=2), 0.3),
        "D262656": (S("rw262656", 1, 513, 2, 2, 512, 1), 0.3),
        "D2354688": (S("rw2354688", 1, 511, 2, 2, 512, 3, pad=1), 0.05),
    }


SMALL = ["D63", "D64", "D65", "D1025", "D1152"]
BIG = ["D262656", "D2354688"]


def _case_names(dt):
    return ["ties", "specials"] + ["byte%d" % j for j in range(np.dtype(dt).itemsize)] + ["all_equal"]


@functools.lru_cache(maxsize=2)
def _cases(D, dt_name, seed):
    return rc.score_cases(D, DTYPES[dt_name], seed)


def _setup(pkg, synth, sid):
    s, density = _shapes(synth)[sid]
    desc = pkg.ConvDesc.from_shape(s)
    D = rc.dense_size(desc)
    assert D == int(sid[1:])
    n = int(D * density)
    pos = np.sort(np.random.RandomState(D % 1000).permutation(D)[:n])
    return s, desc, D, n, pos


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a).ravel()).to(dev)


def check_rewired(plan, want, got_map, got_grown):
    m, g = got_map.cpu().numpy(), got_grown.cpu().numpy()
    assert m.dtype == np.int32 and g.dtype == np.int32
    for name, a, b in (("entry_map", m, want["entry_map"]), ("grown", g, want["grown"])):
        if not np.array_equal(a, b):
            bad = np.flatnonzero(a != b) if a.shape == b.shape else np.zeros(1, int)
            print("%s differs (sizes %d / %d) at %d places, first %d" % (name, a.size, b.size, bad.size, bad[0]))
        assert np.array_equal(a, b), name
    got = plan.get_csr()
    w_rp, w_ci, w_va, w_ng = want["csr"]
    assert plan.nnz() == want["pos"].size
    assert np.array_equal(got[0], w_rp) and np.array_equal(got[1], w_ci) and same_bits(got[2], w_va) and np.array_equal(got[3], w_ng)
    assert plan.stat("rewire_last_dropped") == int((want["entry_map"] < 0).sum()) and plan.stat("rewire_last_grown") == want["grown"].size
    assert plan.stat("prune_count") == 0 and plan.stat("prune_last_dropped") == 0


def _one(pkg, dev, desc, pos, values, grow, score, init=None, **drop):
    plan = gpu_plan(pkg, desc, pos, values, kernel=pkg.KERNEL_GENERIC)
    want = rc.ref_rewire(desc, plan.get_csr(), grow, score, init=init, **drop)
    kw = dict(drop)
    if "drop_score" in kw:
        kw["drop_score"] = _dev(kw["drop_score"], dev)
    got_map, got_grown = plan.rewire(grow, _dev(score, dev), init=_dev(init, dev), **kw)
    check_rewired(plan, want, got_map, got_grown)
    assert plan.stat("rewire_count") == 1
    plan.close()
    return want


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("sid", SMALL)
def test_device_maps_equal_the_rule_on_small_layers(pkg, dev, synth, dt, sid):
    """Every score case over the D positions with a drop and a grow count on a tie boundary; every grow count (0, 1, a tie
    boundary, D - nnz, more) on the tie-heavy case without a drop; init values; a drop on a score array."""
    s, desc, D, n, pos = _setup(pkg, synth, sid)
    np_dt = DTYPES[dt]
    cases = _cases(D, dt, 100 + D % 97)
    values = pc.score_cases(n, np_dt, 3)["ties"]
    drop_keep = pc.tie_boundary_keep(values, n // 2)
    for name in _case_names(np_dt):
        score = cases[name].copy()
        cand = rc.candidates(D, pos)
        grow = pc.tie_boundary_keep(score[cand], max(cand.size // 2, 1))
        score[pos[::3]] = np.nan                                      # inside the pattern: never read
        want = _one(pkg, dev, desc, pos, values, grow, score, drop_keep=drop_keep)
        assert want["grown"].size == grow and int((want["entry_map"] >= 0).sum()) == drop_keep
    for grow in rc.grow_counts(cases["ties"], pos):
        _one(pkg, dev, desc, pos, values, grow, cases["ties"])
    init = np.random.RandomState(5).uniform(-1, 1, D).astype(np_dt)
    init[::5] = -0.0
    init[2::7] = np.nan
    drop_score = pc.score_cases(n, np_dt, 6)["specials"]
    _one(pkg, dev, desc, pos, values, D // 4, cases["specials"], init=init, drop_keep=n // 3, drop_score=drop_score)
    _one(pkg, dev, desc, pos, values, D // 4, cases["byte0"], init=init, drop_threshold=0.5)


BIG_PARAMS = [(sid, dt, name) for sid in BIG for dt in ("f32", "f64") for name in _case_names(DTYPES[dt])]


@pytest.mark.parametrize("sid,dt,name", BIG_PARAMS, ids=["%s-%s-%s" % p for p in BIG_PARAMS])
def test_device_maps_equal_the_rule_on_many_tiles(pkg, dev, synth, sid, dt, name):
    s, desc, D, n, pos = _setup(pkg, synth, sid)
    tiles = (D + TILE - 1) // TILE
    assert tiles > SCAN_WIDTH and D % TILE != 0 and (sid != "D2354688" or tiles > MAX_GRID)
    np_dt = DTYPES[dt]
    score = _cases(D, dt, 100 + D % 97)[name]
    values = sc.seeded_values(n, 7, np_dt)
    cand = rc.candidates(D, pos)
    # (a tie boundary; the scores of "specials" tie only among their zeros, at the very end of the order)
    grow = pc.tie_boundary_keep(score[cand], cand.size - 2 if name == "specials" else cand.size // 2)
    want = _one(pkg, dev, desc, pos, values, grow, score, drop_keep=n - n // 10)
    assert want["grown"].size == grow


def _rand_dense(D, dt, seed, zeros=False):
    v = np.random.RandomState(seed).uniform(-1, 1, D).astype(dt)
    if not zeros:
        v[v == 0] = 0.5
    return v


@pytest.mark.parametrize("kind", ["generic", "jit_lines_3x3", "double"])
def test_a_rewired_plan_equals_a_fresh_plan(pkg, dev, synth, kind):
    """One layer per plan kind: a forward and a backward (the caches and the backward state hold the old pattern), a tenth
    of the entries dropped and as many grown, then get_csr, the exported bytes, kernel, tiling, the forward in all four
    conv_modes and the Backward's three outputs against a fresh set_csr plan on the new CSR; a second round grows zeros."""
    layer = _layer(pkg, dev, synth, kind, 40)
    plan = layer.plan
    D = rc.dense_size(plan.desc)
    td = torch.from_numpy(np.random.RandomState(42).uniform(-1, 1, (layer.s.N, layer.s.M) + tuple(plan.out_hw)).astype(layer.dt)).to(dev)
    layer.forward()
    plan.backward(td, bottom=layer.xd, values_diff=True)
    assert plan.stat("bwd_device_bytes") > 0
    for rnd, use_init in enumerate((True, False)):
        before = plan.get_csr()
        n = before[2].size
        k = n // 10
        score = _rand_dense(D, layer.dt, 43 + rnd, zeros=True)
        init = _rand_dense(D, layer.dt, 45 + rnd) if use_init else None
        want = rc.ref_rewire(plan.desc, before, k, score, init=init, drop_keep=n - k)
        got_map, got_grown = plan.rewire(k, _dev(score, dev), init=_dev(init, dev), drop_keep=n - k)
        assert plan.stat("bwd_device_bytes") == 0 and plan.stat("upd_device_bytes") == 0       # dropped, as on any align
        check_rewired(plan, want, got_map, got_grown)
        ref = _fresh(layer, want["csr"])
        assert ref.kernel_name == plan.kernel_name and ref.tiling_info == plan.tiling_info
        assert ref.stat("kernel_choice") == plan.stat("kernel_choice")
        if layer.dt == np.float32:
            assert plan.export_aligned().tobytes() == ref.export_aligned().tobytes()
        a = plan.backward(td, bottom=layer.xd, values_diff=True, bias_diff=True)
        b = ref.backward(td, bottom=layer.xd, values_diff=True, bias_diff=True)
        torch.cuda.synchronize()
        assert a[1].numel() == n
        for x, y in zip(a, b):
            assert same_bits(x.cpu().numpy(), y.cpu().numpy())
        assert float(a[0].abs().max()) > 0 and float(a[1][got_grown.long()].abs().max()) > 0      # grown entries get a gradient
        for mode in (pkg.CONV_MODE_SCONV, pkg.CONV_MODE_LOWERED_SPARSE, pkg.CONV_MODE_LOWERED_GEMM, pkg.CONV_MODE_SCONV_PAR):
            plan.set_option("conv_mode", mode)
            ref.set_option("conv_mode", mode)
            assert plan.kernel_name == ref.kernel_name
            top = layer.forward()
            assert np.array_equal(top, layer.forward(ref)), (kind, mode, plan.kernel_name)
            assert np.abs(top).max() > 0
        ref.close()
    assert plan.stat("rewire_count") == 2
    plan.close()


@pytest.mark.parametrize("kind", ["generic", "jit_lines_3x3", "double"])
def test_grow_zero_with_a_drop_equals_a_prune(pkg, dev, synth, kind):
    a, b = _layer(pkg, dev, synth, kind, 50), _layer(pkg, dev, synth, kind, 50)
    keep = a.plan.nnz() // 2
    got_map, got_grown = a.plan.rewire(0, None, drop_keep=keep)
    want_map = b.plan.prune(keep=keep)
    assert torch.equal(got_map, want_map) and got_grown.numel() == 0
    assert all(same_bits(x, y) for x, y in zip(a.plan.get_csr(), b.plan.get_csr()))
    assert a.plan.kernel_name == b.plan.kernel_name and a.plan.tiling_info == b.plan.tiling_info
    if a.dt == np.float32:
        assert a.plan.export_aligned().tobytes() == b.plan.export_aligned().tobytes()
    assert np.array_equal(a.forward(), b.forward())
    assert a.plan.stat("rewire_last_dropped") == b.plan.stat("prune_last_dropped") and a.plan.stat("prune_count") == 0
    assert b.plan.stat("rewire_count") == 0
    a.plan.close(), b.plan.close()


@pytest.mark.parametrize("kind", ["generic", "jit_lines_3x3"])
def test_the_kept_values_are_the_devices(pkg, dev, synth, kind):
    """A device-source solver step on one stream (behind work that keeps it busy), no host read, and at once a rewire on
    another stream: the drop ranks the values the step leaves, and the kept entries carry them."""
    layer = _layer(pkg, dev, synth, kind, 53)
    plan = layer.plan
    before = plan.get_csr()
    w0 = before[2].copy()
    n, D = w0.size, rc.dense_size(plan.desc)
    g = sc.seeded_values(n, 54, np.float32, zeros=False)
    hyper = dict(type=sc.SGD, rate=0.75, momentum=0.9)
    w1, _, _ = sc.step(w0, g, np.zeros(n, np.float32), None, **hyper)
    keep, grow = n // 2, n // 4
    score = _rand_dense(D, np.float32, 55)
    want = rc.ref_rewire(plan.desc, (before[0], before[1], w1, before[3]), grow, score, drop_keep=keep)
    assert not np.array_equal(want["entry_map"], rc.ref_rewire(plan.desc, before, grow, score, drop_keep=keep)["entry_map"])
    gd, h = torch.from_numpy(g).to(dev), torch.zeros(n, dtype=torch.float32, device=dev)
    score_d = _dev(score, dev)
    busy = torch.empty((4096, 4096), dtype=torch.float32, device=dev).normal_()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        for _ in range(4):
            busy = busy @ busy
            busy = busy / busy.abs().max()
        plan.solver_step(gd, h, None, **hyper)
    with torch.cuda.stream(s2):
        got_map, got_grown = plan.rewire(grow, score_d, drop_keep=keep)
    torch.cuda.synchronize()
    check_rewired(plan, want, got_map, got_grown)
    plan.close()


@pytest.mark.parametrize("rule,dt", [("sgd", np.float32), ("adam", np.float32), ("adam", np.float64)], ids=["sgd-f32", "adam-f32", "adam-f64"])
def test_training_continues_on_the_device(pkg, dev, synth, rule, dt):
    """The CPU test's sequence with device arrays: forward, backward_values and solver steps before a rewire; histories
    carried by compact_entries into zeros; then the same three calls equal, bit for bit, a fresh plan with numpy-re-indexed
    histories -- and the CPU twin's values."""
    cpu = continuity_cpu(pkg, synth, dt, rule)
    desc, pos, grads, hyper = cpu["desc"], cpu["pos"], cpu["grads"], cpu["hyper"]
    n, adam = pos.size, rule == "adam"
    tdt = torch.float64 if dt == np.float64 else torch.float32
    plan = gpu_plan(pkg, desc, pos, cpu["w0"])
    rs = np.random.RandomState(61)
    x = torch.from_numpy(rs.uniform(-1, 1, (desc.N, desc.C, desc.H, desc.W)).astype(dt)).to(dev)
    td = torch.from_numpy(rs.uniform(-1, 1, (desc.N, desc.M) + tuple(plan.out_hw)).astype(dt)).to(dev)
    bias = torch.from_numpy(rs.uniform(-1, 1, desc.M).astype(dt)).to(dev)
    h = torch.zeros(n, dtype=tdt, device=dev)
    h2 = torch.zeros(n, dtype=tdt, device=dev) if adam else None
    plan.forward(x, bias)
    plan.backward(td, bottom=x, values_diff=True)
    for k in range(2):
        plan.solver_step(torch.from_numpy(grads[k]).to(dev), h, h2, **hyper)
    entry_map, grown = plan.rewire(cpu["grow"], _dev(cpu["score"], dev), drop_keep=cpu["keep"])
    assert np.array_equal(entry_map.cpu().numpy(), cpu["map"]) and np.array_equal(grown.cpu().numpy(), cpu["grown"])
    new_nnz = plan.nnz()
    assert new_nnz == cpu["new_nnz"]
    h_new = pkg.compact_entries(entry_map, h, out=torch.zeros(new_nnz, dtype=tdt, device=dev))
    h2_new = pkg.compact_entries(entry_map, h2, out=torch.zeros(new_nnz, dtype=tdt, device=dev)) if adam else None
    torch.cuda.synchronize()
    h_np, h2_np = h.cpu().numpy(), (h2.cpu().numpy() if adam else None)
    assert same_bits(h_new.cpu().numpy(), rc.reindex(cpu["map"], new_nnz, h_np)) and float(h_new[grown.long()].abs().max()) == 0
    fresh = pkg.Plan(desc)
    fresh.set_csr(*plan.get_csr())
    fh = torch.from_numpy(rc.reindex(cpu["map"], new_nnz, h_np)).to(dev)
    fh2 = torch.from_numpy(rc.reindex(cpu["map"], new_nnz, h2_np)).to(dev) if adam else None
    assert np.array_equal(plan.forward(x, bias).cpu().numpy(), fresh.forward(x, bias).cpu().numpy())
    ga = plan.backward(td, bottom=x, values_diff=True)
    gb = fresh.backward(td, bottom=x, values_diff=True)
    assert same_bits(ga[0].cpu().numpy(), gb[0].cpu().numpy()) and same_bits(ga[1].cpu().numpy(), gb[1].cpu().numpy())
    assert ga[1].numel() == new_nnz
    plan.solver_step(ga[1], h_new, h2_new, **hyper)
    fresh.solver_step(gb[1], fh, fh2, **hyper)
    torch.cuda.synchronize()
    assert all(same_bits(a, b) for a, b in zip(plan.get_csr(), fresh.get_csr()))
    assert same_bits(h_new.cpu().numpy(), fh.cpu().numpy()) and (not adam or same_bits(h2_new.cpu().numpy(), fh2.cpu().numpy()))
    plan.close(), fresh.close()
    # the CPU twin's step on its own gradient: the same bits on a second pair of plans
    plan2 = gpu_plan(pkg, desc, pos, cpu["w0"])
    h = torch.zeros(n, dtype=tdt, device=dev)
    h2 = torch.zeros(n, dtype=tdt, device=dev) if adam else None
    for k in range(2):
        plan2.solver_step(torch.from_numpy(grads[k]).to(dev), h, h2, **hyper)
    entry_map, grown = plan2.rewire(cpu["grow"], _dev(cpu["score"], dev), drop_keep=cpu["keep"])
    h_new = pkg.compact_entries(entry_map, h, out=torch.zeros(new_nnz, dtype=tdt, device=dev))
    h2_new = pkg.compact_entries(entry_map, h2, out=torch.zeros(new_nnz, dtype=tdt, device=dev)) if adam else None
    plan2.solver_step(torch.from_numpy(cpu["g_new"].copy()).to(dev), h_new, h2_new, **hyper)
    torch.cuda.synchronize()
    assert same_bits(plan2.get_csr()[2], cpu["values"]) and same_bits(h_new.cpu().numpy(), cpu["h"])
    assert not adam or same_bits(h2_new.cpu().numpy(), cpu["h2"])
    plan2.close()


def test_accounting_and_three_rewires_in_a_row(pkg, dev, synth):
    """workspace_bytes after rewire, forward, backward and update equals the fresh plan's after the same calls (nothing of
    the old alignment or of the rewire's workspace stays); the stats; the prune_* stats stay untouched; a call that changes
    nothing leaves the backward and update states in place."""
    layer = _layer(pkg, dev, synth, "jit_lines_3x3", 70)
    plan, s = layer.plan, layer.s
    D = rc.dense_size(plan.desc)
    td = torch.from_numpy(np.random.RandomState(71).uniform(-1, 1, (s.N, s.M) + tuple(plan.out_hw)).astype(np.float32)).to(dev)

    def use(p):
        top = p.forward(layer.xd, layer.bd)
        bd, vd, _ = p.backward(td, bottom=layer.xd, values_diff=True)
        p.set_values(torch.from_numpy(p.get_csr()[2]).to(dev))
        torch.cuda.synchronize()
        return top.cpu().numpy(), bd.cpu().numpy(), vd.cpu().numpy()

    use(plan)
    for k, (drop, grow) in enumerate(((0.3, 0.1), (0.1, 0.3), (0.2, 0.2))):
        before = plan.get_csr()
        n = before[2].size
        keep, g = n - int(n * drop), int(n * grow)
        score = _rand_dense(D, np.float32, 72 + k)
        want = rc.ref_rewire(plan.desc, before, g, score, drop_keep=keep)
        got_map, got_grown = plan.rewire(g, _dev(score, dev), drop_keep=keep)
        check_rewired(plan, want, got_map, got_grown)
        assert plan.stat("rewire_count") == k + 1 and plan.stat("rewire_last_dropped") == n - keep and plan.stat("rewire_last_grown") == g
        assert plan.stat("bwd_device_bytes") == 0 and plan.stat("upd_device_bytes") == 0
        assert plan.stat("rewire_realign_us") > 0 and plan.stat("rewire_map_us") > 0
        ref = _fresh(layer, want["csr"])
        assert plan.workspace_bytes == ref.workspace_bytes
        a, b = use(plan), use(ref)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        assert plan.workspace_bytes == ref.workspace_bytes and ref.kernel_name == plan.kernel_name
        ref.close()
    # nothing dropped, nothing grown: the states stay, the map is the identity
    ws, align_us, n = plan.workspace_bytes, plan.stat("align_us"), plan.nnz()
    for grow, sc_d, kw in ((0, None, dict()), (0, None, dict(drop_keep=n + 5)), (0, _dev(_rand_dense(D, np.float32, 79), dev), dict(drop_threshold=0.0))):
        got_map, got_grown = plan.rewire(grow, sc_d, **kw)
        assert np.array_equal(got_map.cpu().numpy(), np.arange(n, dtype=np.int32)) and got_grown.numel() == 0
        assert plan.stat("rewire_last_dropped") == 0 and plan.stat("rewire_last_grown") == 0 and plan.stat("rewire_realign_us") == 0
        assert plan.workspace_bytes == ws and plan.stat("align_us") == align_us
        assert plan.stat("upd_device_bytes") > 0 and plan.stat("bwd_device_bytes") > 0
    assert plan.stat("rewire_count") == 6 and plan.stat("prune_count") == 0 and plan.stat("prune_kernels_us") == 0
    plan.close()


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_an_empty_plan_grows_and_a_full_plan_does_not(pkg, dev, synth, dt):
    s, desc, D, n, pos = _setup(pkg, synth, "D1152")
    np_dt = DTYPES[dt]
    score = _cases(D, dt, 100 + D % 97)["specials"]
    want = _one(pkg, dev, desc, np.zeros(0, np.int64), np.zeros(0, np_dt), 300, score)
    assert want["grown"].size == 300 and np.flatnonzero(np.isnan(score))[0] in want["grown_pos"]
    full = gpu_plan(pkg, desc, np.arange(D), sc.seeded_values(D, 81, np_dt), kernel=pkg.KERNEL_GENERIC)
    align_us = full.stat("align_us")
    got_map, got_grown = full.rewire(5, _dev(score, dev))
    assert np.array_equal(got_map.cpu().numpy(), np.arange(D, dtype=np.int32)) and got_grown.numel() == 0 and full.stat("align_us") == align_us
    want = rc.ref_rewire(desc, full.get_csr(), 5, score, drop_keep=D - 9)          # the dropped positions are no candidates
    got_map, got_grown = full.rewire(5, _dev(score, dev), drop_keep=D - 9)
    check_rewired(full, want, got_map, got_grown)
    assert got_grown.numel() == 0
    full.close()


def test_device_errors(pkg, dev, synth):
    L = pkg.lib()
    s, desc, D, n, pos = _setup(pkg, synth, "D1025")
    plan = gpu_plan(pkg, desc, pos, sc.seeded_values(n, 92, np.float32), kernel=pkg.KERNEL_GENERIC)
    EINVAL, ESTATE = -1, -4
    score = torch.ones(D, dtype=torch.float32, device=dev)
    sp = score.data_ptr()

    def rewire(d, p=plan):
        return L.escoin_plan_rewire(p._h, None if d is None else C.byref(d), None, None, None, None, None)

    def drop(*a):
        return C.pointer(pkg.PruneDesc(*a))

    assert rewire(None) == EINVAL
    assert rewire(pkg.RewireDesc(None, -1, sp, None)) == EINVAL
    assert rewire(pkg.RewireDesc(None, 1, None, None)) == EINVAL
    assert rewire(pkg.RewireDesc(drop(2, 1, 0.0, None), 1, sp, None)) == EINVAL
    assert rewire(pkg.RewireDesc(drop(pkg.PRUNE_KEEP, -1, 0.0, None), 1, sp, None)) == EINVAL
    assert rewire(pkg.RewireDesc(drop(pkg.PRUNE_THRESHOLD, 0, -1.0, None), 1, sp, None)) == EINVAL
    assert rewire(pkg.RewireDesc(drop(pkg.PRUNE_THRESHOLD, 0, float("nan"), None), 1, sp, None)) == EINVAL
    assert plan.nnz() == n and plan.stat("rewire_count") == 0
    ok = pkg.RewireDesc(None, 5, sp, None)
    unaligned = pkg.Plan(desc)
    assert rewire(ok, unaligned) == ESTATE
    host_only = pkg.Plan(desc)
    host_only.weight_align_cpu(np.ones((desc.M, desc.C, desc.KH, desc.KW), np.float32))
    assert rewire(ok, host_only) == ESTATE
    assert L.escoin_plan_rewire_cpu(plan._h, C.byref(ok), None, None, None, None) == ESTATE       # _cpu on a device-aligned plan
    # every output pointer may be NULL on the device entry point; new_nnz and n_grown report the counts
    new_nnz, n_grown = C.c_long(-1), C.c_long(-1)
    assert L.escoin_plan_rewire(plan._h, C.byref(ok), None, None, C.byref(new_nnz), C.byref(n_grown), None) == 0
    assert new_nnz.value == n + 5 and n_grown.value == 5 and plan.nnz() == n + 5
    plan.close(), unaligned.close(), host_only.close()
