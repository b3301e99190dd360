"""escoin_dense_wgrad on the MI355X (escoin_dense_wgrad_mfma_kernel + escoin_dense_wgrad_sum_kernel): every position of the
dense weight gradient on every shape of wgrad_mfma_common.ALL, plain and fuse_relu, against torch float64 autograd with an
all-ones mask and the per-element bound of errbound.backward_bound (its term count N*OH*OW + 4 covers any summation
order, so the split of the pixel axis needs no new tolerance); the splits; accumulation, overwrite, partial batches,
determinism; non-finite containment; the state across re-aligns; graph capture; a RigL step end to end; refusals."""
import numpy as np
import pytest

import errbound as eb
import rewire_common as rc
from dense_wgrad_common import LDS, rule
from wgrad_mfma_common import ALL, make

torch = pytest.importorskip("torch")

from wgrad_common import seeded  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(pkg):
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        pytest.fail("no HIP device visible (these tests run on the MI355X)")
    return torch.device("cuda:0")


_INPUTS = {}
_REFS = {}


def _inputs(synth, name):
    """(shape, weights, activations, bias, top_diff) of a named shape: made once, never written."""
    if name not in _INPUTS:
        s = make(synth, name)
        oh, ow = synth.out_hw(s)
        _INPUTS[name] = (s, synth.pruned_weights(s, 11), synth.activations(s, 12), synth.bias_vector(s, 13),
                         seeded((s.N, s.M, oh, ow), 21))
    return _INPUTS[name]


def _ref(synth, name, n=None):
    """(float64 dense gradient, per-element bound) of the first n images without ReLU: computed once."""
    if (name, n) not in _REFS:
        s, w, x, b, td = _inputs(synth, name)
        want, Bs = eb.backward_bound(s, w, x[:n], b, td[:n], mask=np.ones_like(w, bool))
        _REFS[(name, n)] = (want[1], Bs[1])
    return _REFS[(name, n)]


def _plan(pkg, s, w, relu=False, **opts):
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu), **opts)
    plan.weight_align(w)
    return plan


def _up(dev, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- 1. correctness ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("name", list(ALL))
def test_every_position_within_the_float64_bound(pkg, dev, synth, name, relu):
    s, w, x, b, td = _inputs(synth, name)
    xt, bt, tdt = _up(dev, x, b, td)
    plan = _plan(pkg, s, w, relu)
    assert plan.stat("dwg_count") == 0 and plan.stat("dwg_device_bytes") == 0
    ws0 = plan.workspace_bytes
    top = plan.forward(xt, bt) if relu else None
    got = plan.dense_wgrad(tdt, xt, top=top)
    torch.cuda.synchronize()
    assert plan.stat("dwg_count") == 1 and plan.stat("dwg_lds_bytes") == LDS == 2 * 2 * 32 * 65 * 4
    mtiles, ktiles, chunks, span, splits, D, slab = rule(s, synth.out_hw(s), _cus())
    assert plan.stat("dwg_splits") == splits
    assert plan.stat("dwg_device_bytes") == slab + 16 * ktiles * 64
    assert plan.workspace_bytes == ws0 + plan.stat("dwg_device_bytes")
    assert tuple(got.shape) == w.shape
    if relu:
        want, Bs = eb.backward_bound(s, w, x, b, td, top.cpu().numpy(), mask=np.ones_like(w, bool))
        want, B = want[1], Bs[1]
    else:
        want, B = _ref(synth, name)
    r = eb.within(got.cpu().numpy(), want, B, "dense_wgrad", what=(name, relu))
    print("dense_wgrad %-12s relu=%d splits %d: %.3g of the bound" % (name, relu, splits, r))
    plan.close()


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("name", ["straddle3x3", "small7x7g2", "d_pw", "d_conv1", "d_g3"])
def test_skewed_inputs_within_the_bound(pkg, dev, synth, name, relu):
    """Inputs whose rows, channels and images differ in scale by up to 2^48 (errbound.skew)."""
    s = make(synth, name)
    w, x, b = synth.pruned_weights(s, 91), synth.activations(s, 92), synth.bias_vector(s, 93)
    td = seeded((s.N, s.M) + synth.out_hw(s), 94)
    sk = eb.skew(s, w, x, b, 95, top_diff=td)
    xd, bd, tdd = _up(dev, sk.x.astype(np.float32), None if sk.b is None else sk.b.astype(np.float32), sk.top_diff.astype(np.float32))
    plan = _plan(pkg, s, sk.w, relu)
    top = top_np = None
    if relu:
        top = plan.forward(xd, bd)
        torch.cuda.synchronize()
        top_np = top.cpu().numpy()
    want, Bs = eb.backward_bound(s, sk.w, sk.x, sk.b, sk.top_diff, top_np, mask=np.ones_like(sk.w, bool))
    got = plan.dense_wgrad(tdd, xd, top=top)
    torch.cuda.synchronize()
    assert plan.stat("dwg_count") == 1
    r = eb.within(got.cpu().numpy(), want[1], Bs[1], "dense_wgrad", sk.td_row_exp, axis=0, what=(name, "relu", relu))
    print("errbound dense_wgrad %-12s relu=%d: %.3g" % (name, relu, r))
    plan.close()


# ---- 2. splits -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", [1, 2, 0])
@pytest.mark.parametrize("name", ["small7x7g2", "d_pw"])
def test_splits_stay_within_the_bound_and_follow_the_rule(pkg, dev, synth, name, splits):
    s, w, x, b, td = _inputs(synth, name)
    xt, tdt = _up(dev, x, td)
    plan = _plan(pkg, s, w, dense_wgrad_splits=splits)
    got = plan.dense_wgrad(tdt, xt)
    torch.cuda.synchronize()
    _, _, chunks, span, want_splits, D, slab = rule(s, synth.out_hw(s), _cus(), splits)
    assert chunks == {"small7x7g2": 3, "d_pw": 2}[name]
    assert plan.stat("dwg_splits") == want_splits
    if splits == 1:
        assert want_splits == 1
    if splits == 2 and name == "small7x7g2":
        assert (span, want_splits) == (2, 2)            # three chunks in spans of 2 + 1
    want, B = _ref(synth, name)
    eb.within(got.cpu().numpy(), want, B, "dense_wgrad", what=(name, splits))
    plan.close()


def test_a_partial_batch_whose_last_span_is_empty(pkg, dev, synth):
    """small7x7g2 in two spans of two chunks: 22 images are 1078 pixels, two chunks, all in the first span -- the second
    is not launched, and its stale partials of the full batch before are not summed."""
    s, w, x, b, td = _inputs(synth, "small7x7g2")
    xt, tdt = _up(dev, x, td)
    plan = _plan(pkg, s, w, dense_wgrad_splits=2)
    full = plan.dense_wgrad(tdt, xt)
    got = plan.dense_wgrad(tdt, xt, n_images=22)
    torch.cuda.synchronize()
    assert plan.stat("dwg_splits") == 2
    want, B = _ref(synth, "small7x7g2", 22)
    eb.within(got.cpu().numpy(), want, B, "dense_wgrad", what="22 of 43 images")
    assert _bytes(full) != _bytes(got)
    # one span of the same pixels gives the same bits: the second span contributed nothing
    one = _plan(pkg, s, w, dense_wgrad_splits=1)
    assert _bytes(one.dense_wgrad(tdt, xt, n_images=22)) == _bytes(got)
    one.close()
    plan.close()


# ---- 3. contract -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d_3x3", "d_g3", "small7x7g2"])
def test_accumulate_adds_and_overwrite_clears(pkg, dev, synth, name):
    s, w, x, b, td = _inputs(synth, name)
    xt, tdt = _up(dev, x, td)
    plan = _plan(pkg, s, w)
    pre = seeded(w.shape, 31)
    alone = plan.dense_wgrad(tdt, xt)
    out = torch.from_numpy(pre).to(dev)
    assert plan.dense_wgrad(tdt, xt, out=out, accumulate=True) is out
    junk = torch.full(w.shape, float("nan"), device=dev)
    plan.dense_wgrad(tdt, xt, out=junk)
    torch.cuda.synchronize()
    alone_np = alone.cpu().numpy()
    # one rounded addition of the gradient onto the prefill
    assert _bytes(out) == (pre + alone_np).tobytes()
    want, B = _ref(synth, name)
    oh, ow = synth.out_hw(s)
    eb.within(out.cpu().numpy(), want + pre, eb.accumulated_bound(B, pre, s.N * oh * ow), "dense_wgrad accumulate", what=name)
    assert _bytes(junk) == alone_np.tobytes() and np.all(np.isfinite(alone_np))
    plan.close()


@pytest.mark.parametrize("name", ["d_pw", "d_conv1", "small7x7g2"])
def test_partial_batches_never_read_the_images_past_n_images(pkg, dev, synth, name):
    s, w, x, b, td = _inputs(synth, name)
    plan = _plan(pkg, s, w)
    for n in (0, 1, s.N):
        xn, tdn = x.copy(), td.copy()
        xn[n:] = np.nan
        tdn[n:] = np.nan
        xt, tdt = _up(dev, xn, tdn)
        got = plan.dense_wgrad(tdt, xt, n_images=n)
        torch.cuda.synchronize()
        if n == 0:
            assert np.all(got.cpu().numpy() == 0)
            pre = seeded(w.shape, 32)
            out = torch.from_numpy(pre).to(dev)
            plan.dense_wgrad(tdt, xt, out=out, accumulate=True, n_images=0)
            torch.cuda.synchronize()
            assert _bytes(out) == pre.tobytes()
            continue
        want, B = _ref(synth, name, n)
        eb.within(got.cpu().numpy(), want, B, "dense_wgrad partial", what=(name, n))
    plan.close()


@pytest.mark.parametrize("name", ["straddle3x3", "d_pw"])
def test_identical_bits_on_two_streams_and_on_a_fresh_plan(pkg, dev, synth, name):
    s, w, x, b, td = _inputs(synth, name)
    xt, tdt = _up(dev, x, td)
    plan = _plan(pkg, s, w)
    r1 = plan.dense_wgrad(tdt, xt)
    ws1 = plan.workspace_bytes
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        r2 = plan.dense_wgrad(tdt, xt)
    torch.cuda.synchronize()
    assert plan.workspace_bytes == ws1
    other = _plan(pkg, s, np.where(seeded(w.shape, 41) > 0.3, np.float32(2), np.float32(0)), tiling_batch=256)
    r3 = other.dense_wgrad(tdt, xt)          # another pattern, other values: the same function
    torch.cuda.synchronize()
    assert _bytes(r1) == _bytes(r2) == _bytes(r3)
    plan.close()
    other.close()


# ---- 4. non-finite containment ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d_3x3", "d_conv1"])
def test_a_nan_in_bottom_reaches_exactly_the_pairs_that_read_it(pkg, dev, synth, name):
    s, w, x, b, td = _inputs(synth, name)
    n, c, h, wq = 1, s.C - 1, s.H // 2, s.W // 2 + 1
    x_nan = x.copy()
    x_nan[n, c, h, wq] = np.nan
    xt, tdt = _up(dev, x_nan, td)
    plan = _plan(pkg, s, w)
    got = plan.dense_wgrad(tdt, xt).cpu().numpy()
    oh, ow = synth.out_hw(s)
    cg, mg = s.C // s.group, s.M // s.group
    hit = np.zeros(w.shape, bool)
    for kr in range(s.KH):
        for kc in range(s.KW):
            # output pixels whose tap (kr, kc) reads (h, wq)
            a, r = divmod(h + s.pad_h - kr * s.dil_h, s.stride_h)
            e, q = divmod(wq + s.pad_w - kc * s.dil_w, s.stride_w)
            if r == 0 and q == 0 and 0 <= a < oh and 0 <= e < ow:
                grp = c // cg
                hit[grp * mg:(grp + 1) * mg, c % cg, kr, kc] = True
    assert hit.sum() > 0 and (~hit).sum() > 0
    if name == "d_conv1":
        assert hit.sum() < s.M * s.KH * s.KW                # stride 2: only the taps of the pixel's parity
    assert np.all(np.isnan(got[hit]))
    assert np.all(np.isfinite(got[~hit]))
    plan.close()


# ---- 5. the state survives re-aligns; graph capture ---------------------------------------------------------------------------
def test_the_state_survives_a_rewire_and_a_captured_call_stays_valid(pkg, dev, synth):
    """call, capture a call, rewire (a re-align: the backward and update states go), replay, call again: the state's
    bytes are unchanged, the replay is valid and every result has the bits of a fresh plan's."""
    s, w, x, b, td = _inputs(synth, "d_g3")
    xt, tdt = _up(dev, x, td)
    plan = _plan(pkg, s, w)
    first = plan.dense_wgrad(tdt, xt)
    torch.cuda.synchronize()
    bytes0 = plan.stat("dwg_device_bytes")
    assert bytes0 > 0
    out = torch.zeros_like(first)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.dense_wgrad(tdt, xt, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert _bytes(out) == _bytes(first)
    nnz = plan.nnz()
    plan.rewire(5, first, drop_keep=nnz - 5)
    assert plan.stat("rewire_count") == 1 and plan.stat("dwg_device_bytes") == bytes0
    out.fill_(float("nan"))
    g.replay()
    again = plan.dense_wgrad(tdt, xt)
    torch.cuda.synchronize()
    assert plan.stat("dwg_device_bytes") == bytes0
    fresh = _plan(pkg, s, w)
    want = fresh.dense_wgrad(tdt, xt)
    torch.cuda.synchronize()
    assert _bytes(out) == _bytes(again) == _bytes(first) == _bytes(want)
    # a weight_align keeps it too
    plan.weight_align(w)
    assert plan.stat("dwg_device_bytes") == bytes0 and _bytes(plan.dense_wgrad(tdt, xt)) == _bytes(want)
    plan.close()
    fresh.close()


def test_captured_after_forward_and_backward_on_one_stream(pkg, dev, synth):
    """forward -> backward(values_diff) -> dense_wgrad captured on ONE stream (a chain: no parallel branches) after an
    eager round built the states; the replay's bits equal the eager ones and nothing is allocated."""
    s, w, x, b, td = _inputs(synth, "d_pw")
    xt, bt, tdt = _up(dev, x, b, td)
    plan = _plan(pkg, s, w, relu=True)
    oh, ow = plan.out_hw
    y = torch.zeros((s.N, s.M, oh, ow), device=dev)
    vd = torch.zeros(plan.nnz(), device=dev)
    score = torch.zeros(w.shape, device=dev)

    def step():
        plan.forward(xt, bt, y)
        plan.backward(tdt, bottom=xt, top=y, bottom_diff=None, values_diff=vd)
        plan.dense_wgrad(tdt, xt, top=y, out=score)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = (_bytes(y), _bytes(vd), _bytes(score))
    ws1 = plan.workspace_bytes
    count = plan.stat("dwg_count")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    assert plan.workspace_bytes == ws1 and plan.stat("dwg_count") == count + 1
    vd.zero_()
    score.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert (_bytes(y), _bytes(vd), _bytes(score)) == eager
    assert plan.workspace_bytes == ws1
    plan.close()


# ---- 6. a RigL step end to end --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d_g3", "straddle3x3"])
def test_rigl_step_from_the_plan_alone(pkg, dev, synth, name):
    """score = dense_wgrad; rewire(grow = k, score, drop_keep = nnz - k): the maps equal the rule run on the DOWNLOADED
    device score and values (an integer comparison against the float64 reference would make near-ties flaky), and the next
    forward equals, bit for bit, a fresh plan set_csr'd on the new CSR."""
    s, w, x, b, td = _inputs(synth, name)
    xt, bt, tdt = _up(dev, x, b, td)
    plan = _plan(pkg, s, w)
    nnz = plan.nnz()
    k = max(nnz // 10, 3)
    csr = plan.get_csr()
    score = plan.dense_wgrad(tdt, xt)
    entry_map, grown = plan.rewire(k, score, drop_keep=nnz - k)
    torch.cuda.synchronize()
    want = rc.ref_rewire(plan.desc, csr, k, score.cpu().numpy(), drop_keep=nnz - k)
    assert np.array_equal(entry_map.cpu().numpy(), want["entry_map"])
    assert np.array_equal(grown.cpu().numpy(), want["grown"]) and grown.numel() == k
    assert plan.nnz() == nnz
    fresh = pkg.Plan(pkg.ConvDesc.from_shape(s))
    fresh.set_csr(*want["csr"])
    assert _bytes(plan.forward(xt, bt)) == _bytes(fresh.forward(xt, bt))
    # the compact arrays follow through the map, as after any rewire
    h = torch.from_numpy(seeded((nnz,), 61)).to(dev)
    moved = pkg.compact_entries(entry_map, h, out=torch.zeros(plan.nnz(), device=dev))
    torch.cuda.synchronize()
    assert np.array_equal(moved.cpu().numpy(), rc.reindex(want["entry_map"], plan.nnz(), h.cpu().numpy()))
    plan.close()
    fresh.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, dev, synth):
    s, w, x, b, td = _inputs(synth, "d_g3")
    xt, tdt = _up(dev, x, td)
    # a double plan: ESCOIN_EINVAL with the documented message, from either entry point, and it stays usable
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
    plan.weight_align(w.astype(np.float64))
    for args in ((tdt.double(), xt.double()), (tdt, xt)):
        with pytest.raises(pkg.EscoinError) as e:
            plan.dense_wgrad(*args)
        assert "failed (-1)" in str(e.value) and "no double kernel: use escoin_dense_wgrad_cpu_f64" in str(e.value)
    assert plan.stat("dwg_count") == 0 and plan.stat("dwg_device_bytes") == 0
    got = plan.dense_wgrad_cpu(td.astype(np.float64), x.astype(np.float64))
    want, Bs = eb.backward_bound(s, w.astype(np.float64), x.astype(np.float64), None if b is None else b.astype(np.float64),
                                 td.astype(np.float64), f64=True, mask=np.ones_like(w, bool))
    eb.within(got, want[1], Bs[1], "dense_wgrad_cpu_f64", what="double plan on the device")
    plan.close()
    # before an align
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
    with pytest.raises(pkg.EscoinError) as e:
        plan.dense_wgrad(tdt, xt)
    assert "failed (-4)" in str(e.value)                                  # ESCOIN_ESTATE
    plan.weight_align(w)
    out = torch.zeros(w.shape, device=dev)
    L = pkg.lib()
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    for xb, tdb, ob, n in ((None, tdt, out, s.N), (xt, None, out, s.N), (xt, tdt, None, s.N), (xt, tdt, out, -1), (xt, tdt, out, s.N + 1)):
        assert L.escoin_dense_wgrad(plan._h, P(xb), None, P(tdb), P(ob), n, 0, None) == -1      # ESCOIN_EINVAL
    plan.close()
    relu = _plan(pkg, s, w, relu=True)
    with pytest.raises(pkg.EscoinError) as e:
        relu.dense_wgrad(tdt, xt)                                         # fuse_relu without top
    assert "failed (-1)" in str(e.value) and "top" in str(e.value)
    relu.close()
