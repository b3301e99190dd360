"""The weight gradient on the MI355X under option "wgrad_kernel" = MFMA (escoin_sconv_wgrad_mfma_kernel): the eight sparse
shapes of wgrad_common.SHAPES and six dense ones at the kernel's tile edges (wgrad_mfma_common.DENSE) against torch float64
autograd and the per-element bound of errbound.py; the pattern is all that is written; compact == dense gathered bit for
bit; accumulation, partial batches, determinism, refusals, a captured training loop and set_values.  Every case asserts
that the MFMA kernel ran."""
import numpy as np
import pytest

import errbound as eb
from conftest import rel_err
from wgrad_mfma_common import ALL, make

torch = pytest.importorskip("torch")

from wgrad_common import csr_positions, seeded, torch_backward  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4


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
    """torch float64 (bottom_diff, weight_diff, bias_diff) of the first n images without ReLU: computed once."""
    if (name, n) not in _REFS:
        s, w, x, b, td = _inputs(synth, name)
        _REFS[(name, n)] = torch_backward(x[:n], w, b, s, td[:n])
    return _REFS[(name, n)]


def _plan(pkg, s, w, relu=False, **opts):
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu), wgrad_kernel=pkg.WGRAD_MFMA, **opts)
    plan.weight_align(w)
    return plan


def _chunks(s, synth, n=None):
    oh, ow = synth.out_hw(s)
    return ((s.N if n is None else n) * oh * ow + 1023) // 1024


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _ran_mfma(pkg, plan):
    assert plan.stat("wgrad_kernel") == pkg.WGRAD_MFMA
    assert plan.stat("wgrad_lds_bytes") == 2 * 2 * 32 * 65 * 4 <= 64 * 1024


# ---- 1. correctness --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("name", list(ALL))
def test_matches_torch_writes_the_pattern_only_and_compact_equals_dense(pkg, dev, synth, name, relu):
    s, w, x, b, td = _inputs(synth, name)
    xt, tdt = torch.from_numpy(x).to(dev), torch.from_numpy(td).to(dev)
    bt = torch.from_numpy(b).to(dev) if b is not None else None
    plan = _plan(pkg, s, w, relu)
    with pytest.raises(pkg.EscoinError):
        plan.stat("wgrad_kernel")               # nothing has run yet
    top = plan.forward(xt, bt) if relu else None
    torch.cuda.synchronize()
    want = torch_backward(x, w, b, s, td, top.cpu().numpy()) if relu else _ref(synth, name)
    pos = csr_positions(plan)
    for with_bias in (True, False):
        what = (name, relu, with_bias)
        # NaN outside the pattern: it must come back NaN -- nothing there is read or written
        fill = torch.from_numpy(np.where(w == 0, np.float32(np.nan), np.float32(0))).to(dev)
        _, wd, bsd = plan.backward(tdt, bottom=xt, top=top, bottom_diff=None, weight_diff=fill,
                                   bias_diff=True if with_bias else None)
        _, vd, bsd2 = plan.backward(tdt, bottom=xt, top=top, bottom_diff=None, values_diff=True,
                                    bias_diff=True if with_bias else None)
        torch.cuda.synchronize()
        _ran_mfma(pkg, plan)
        wd, vd = wd.cpu().numpy(), vd.cpu().numpy()
        assert np.all(np.isnan(wd[w == 0])), what
        assert np.all(np.isfinite(wd[w != 0])), what
        wd0 = np.where(w == 0, np.float32(0), wd)
        print(what, "weight_diff rel_err", rel_err(wd0, want[1]),
              "bias_diff rel_err", None if not with_bias else rel_err(bsd.cpu().numpy(), want[2]))
        assert rel_err(wd0, want[1]) <= TOL, what
        if with_bias:
            assert rel_err(bsd.cpu().numpy(), want[2]) <= TOL, what
            assert _bytes(bsd) == _bytes(bsd2), what
        else:
            assert bsd is None and bsd2 is None
        assert vd.shape == (plan.nnz(),) and len(pos) == plan.nnz()
        assert vd.tobytes() == wd.reshape(-1)[pos].tobytes(), what
        assert plan.stat("bwd_chunks") == _chunks(s, synth), what
    plan.close()


def test_bias_gradient_is_the_entry_kernel_s_bit_for_bit(pkg, dev, synth):
    s, w, x, b, td = _inputs(synth, "d_pw")
    xt, tdt = torch.from_numpy(x).to(dev), torch.from_numpy(td).to(dev)
    got = {}
    for kernel in (pkg.WGRAD_MFMA, pkg.WGRAD_ENTRY):
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s), wgrad_kernel=kernel)
        plan.weight_align(w)
        _, _, alone = plan.backward(tdt, bottom_diff=None, bias_diff=True)
        _, vd, fused = plan.backward(tdt, bottom=xt, bottom_diff=None, values_diff=True, bias_diff=True)
        torch.cuda.synchronize()
        assert plan.stat("wgrad_kernel") == kernel
        assert _bytes(alone) == _bytes(fused)
        got[kernel] = (_bytes(fused), _bytes(vd))
        plan.close()
    assert got[pkg.WGRAD_MFMA][0] == got[pkg.WGRAD_ENTRY][0]
    # 1083 products per entry in two different orders: identical weight bits would mean the forced kernel did not run
    assert got[pkg.WGRAD_MFMA][1] != got[pkg.WGRAD_ENTRY][1]


# ---- 2. error bound ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("name", ["straddle3x3", "small7x7g2", "pointwise", "stride2", "d_pw", "d_conv1"])
def test_every_element_within_the_float64_error_bound(pkg, synth, dev, name, relu):
    """Inputs whose rows, channels and images differ in scale by up to 2^48 (errbound.skew): every element of the weight
    and bias gradient within errbound.backward_bound, in dense and in compact form."""
    s = make(synth, name)
    w, x, b = synth.pruned_weights(s, 91), synth.activations(s, 92), synth.bias_vector(s, 93)
    td = seeded((s.N, s.M) + synth.out_hw(s), 94)
    sk = eb.skew(s, w, x, b, 95, top_diff=td)

    def up(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    xd, bd_, tdd = up(sk.x), up(sk.b), up(sk.top_diff)
    plan = _plan(pkg, s, sk.w, relu, backward_kernel=pkg.KERNEL_GENERIC)
    top_np = topd = None
    if relu:
        topd = plan.forward(xd, bd_)
        torch.cuda.synchronize()
        top_np = topd.cpu().numpy()
    want, Bs = eb.backward_bound(s, sk.w, sk.x, sk.b, sk.top_diff, top_np)
    _, wd, bsd = plan.backward(tdd, bottom=xd, top=topd, bottom_diff=None, weight_diff=True, bias_diff=True)
    _, vd, bsd2 = plan.backward(tdd, bottom=xd, top=topd, bottom_diff=None, values_diff=True, bias_diff=True)
    torch.cuda.synchronize()
    _ran_mfma(pkg, plan)
    what = (name, "relu", relu)
    wdn = wd.cpu().numpy()
    r = eb.within(wdn, want[1], Bs[1], "wgrad_kernel 3", sk.td_row_exp, axis=0, what=what)
    rb = eb.within(bsd.cpu().numpy(), want[2], Bs[2], "wgrad_kernel 3 bias", sk.td_row_exp, axis=0, what=what)
    assert np.all(wdn[sk.w == 0] == 0), what
    pos = csr_positions(plan)
    rv = eb.within(vd.cpu().numpy(), want[1].reshape(-1)[pos], Bs[1].reshape(-1)[pos], "wgrad_kernel 3 compact", what=what)
    eb.within(bsd2.cpu().numpy(), want[2], Bs[2], "wgrad_kernel 3 compact bias", sk.td_row_exp, axis=0, what=what)
    print("errbound backward weight kernel 3 (MFMA) %-12s relu=%d: %.3g, bias %.3g, values %.3g" % (name, relu, r, rb, rv))
    assert r <= 1.0 and rb <= 1.0 and rv <= 1.0
    plan.close()


# ---- 3. accumulation and partial batches -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d_3x3", "d_g3", "dil2_asym"])
def test_accumulates_into_prefilled_blobs(pkg, dev, synth, name):
    s, w, x, b, td = _inputs(synth, name)
    xt, tdt = torch.from_numpy(x).to(dev), torch.from_numpy(td).to(dev)
    want = _ref(synth, name)
    plan = _plan(pkg, s, w)
    pre_w, pre_b = seeded(w.shape, 31), seeded((s.M,), 32)
    pre_v = seeded((plan.nnz(),), 33)
    _, wd, bsd = plan.backward(tdt, bottom=xt, bottom_diff=None, weight_diff=torch.from_numpy(pre_w).to(dev),
                               bias_diff=torch.from_numpy(pre_b).to(dev))
    _, vd, _ = plan.backward(tdt, bottom=xt, bottom_diff=None, values_diff=torch.from_numpy(pre_v).to(dev))
    _, vd0, _ = plan.backward(tdt, bottom=xt, bottom_diff=None, values_diff=True)
    torch.cuda.synchronize()
    _ran_mfma(pkg, plan)
    wd, vd, vd0 = wd.cpu().numpy(), vd.cpu().numpy(), vd0.cpu().numpy()
    pos = csr_positions(plan)
    assert wd[w == 0].tobytes() == pre_w[w == 0].tobytes()          # outside the pattern: the prefill, untouched
    assert rel_err(wd, want[1] + pre_w) <= TOL
    assert rel_err(bsd.cpu().numpy(), want[2] + pre_b) <= TOL
    # one rounded addition of the gradient to the prefill
    assert vd.tobytes() == (pre_v + vd0).tobytes()
    assert wd.reshape(-1)[pos].tobytes() == (pre_w.reshape(-1)[pos] + vd0).tobytes()
    plan.close()


PARTIAL = [("small7x7g2", 1), ("small7x7g2", 42), ("small7x7g2", 22),      # 22 x 49 = 1078 px: pixel 1024 is mid-row in image 20
           ("d_pw", 1), ("d_pw", 2), ("d_s2pw", 4), ("d_conv1", 1)]


@pytest.mark.parametrize("name,n", PARTIAL, ids=["%s-%d" % p for p in PARTIAL])
def test_partial_batch_is_the_gradient_of_the_first_images(pkg, dev, synth, name, n):
    s, w, x, b, td = _inputs(synth, name)
    assert 0 < n < s.N
    xt, tdt = torch.from_numpy(x).to(dev), torch.from_numpy(td).to(dev)
    want = _ref(synth, name, n)
    plan = _plan(pkg, s, w)
    _, wd, bsd = plan.backward(tdt[:n], bottom=xt[:n], bottom_diff=None, weight_diff=True, bias_diff=True)
    _, vd, _ = plan.backward(tdt[:n], bottom=xt[:n], bottom_diff=None, values_diff=True)
    torch.cuda.synchronize()
    _ran_mfma(pkg, plan)
    wd, vd = wd.cpu().numpy(), vd.cpu().numpy()
    print(name, n, "weight_diff rel_err", rel_err(wd, want[1]), "bias_diff rel_err", rel_err(bsd.cpu().numpy(), want[2]))
    assert rel_err(wd, want[1]) <= TOL and rel_err(bsd.cpu().numpy(), want[2]) <= TOL
    assert np.all(wd[w == 0] == 0)
    assert vd.tobytes() == wd.reshape(-1)[csr_positions(plan)].tobytes()
    assert plan.stat("bwd_chunks") == _chunks(s, synth, n)
    plan.close()


def test_empty_rows_an_empty_group_and_an_empty_pattern(pkg, dev, synth):
    """Rows and a conv group without entries: their tiles do nothing and their positions stay untouched; nnz == 0: no
    launch, no error, the bias gradient still comes."""
    s, w, x, b, td = _inputs(synth, "d_g3")
    xt, tdt = torch.from_numpy(x).to(dev), torch.from_numpy(td).to(dev)
    mg = s.M // s.group
    for case in ("rows_and_group", "nothing"):
        w2 = w.copy()
        w2[:mg] = 0                       # group 0
        w2[mg + 1] = 0                    # a row of group 1
        if case == "nothing":
            w2[:] = 0
        want = torch_backward(x, w2, b, s, td)
        plan = _plan(pkg, s, w2)
        assert plan.nnz() == int((w2 != 0).sum())
        fill = torch.from_numpy(np.where(w2 == 0, np.float32(np.nan), np.float32(0))).to(dev)
        _, wd, bsd = plan.backward(tdt, bottom=xt, bottom_diff=None, weight_diff=fill, bias_diff=True)
        _, vd, _ = plan.backward(tdt, bottom=xt, bottom_diff=None, values_diff=True)
        torch.cuda.synchronize()
        _ran_mfma(pkg, plan)
        wd = wd.cpu().numpy()
        assert np.all(np.isnan(wd[w2 == 0])), case
        assert rel_err(np.where(w2 == 0, np.float32(0), wd), want[1]) <= TOL, case
        assert rel_err(bsd.cpu().numpy(), want[2]) <= TOL, case
        assert vd.cpu().numpy().tobytes() == wd.reshape(-1)[csr_positions(plan)].tobytes(), case
        plan.close()


def test_non_finite_bottom_reaches_only_the_entries_whose_tap_reads_it(pkg, dev, synth):
    s, w, x, b, td = _inputs(synth, "d_3x3")
    c = 7
    x_inf = x.copy()
    x_inf[1, c, 0, 0] = np.inf
    tdt = torch.from_numpy(td).to(dev)
    plan = _plan(pkg, s, w)
    _, clean, _ = plan.backward(tdt, bottom=torch.from_numpy(x).to(dev), bottom_diff=None, values_diff=True)
    _, dirty, _ = plan.backward(tdt, bottom=torch.from_numpy(x_inf).to(dev), bottom_diff=None, values_diff=True)
    torch.cuda.synchronize()
    _ran_mfma(pkg, plan)
    clean, dirty = clean.cpu().numpy(), dirty.cpu().numpy()
    # pixel (0, 0) is read by output pixel (pad - kr, pad - kc): inside the image for kr, kc <= pad = 1
    col = plan.get_csr()[1]
    ic, kr, kc = col // 9, (col // 3) % 3, col % 3
    hit = (ic == c) & (kr <= 1) & (kc <= 1)
    assert hit.sum() > 0 and (~hit).sum() > 0
    assert not np.any(np.isfinite(dirty[hit]))
    assert dirty[~hit].tobytes() == clean[~hit].tobytes()
    plan.close()


# ---- 4. determinism ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["straddle3x3", "d_pw"])
def test_determinism_streams_tiling_batch_and_memory(pkg, dev, synth, name):
    s, w, x, b, td = _inputs(synth, name)
    xt, tdt = torch.from_numpy(x).to(dev), torch.from_numpy(td).to(dev)
    plan = _plan(pkg, s, w)
    ws0 = plan.workspace_bytes

    def call(p):
        return p.backward(tdt, bottom=xt, bottom_diff=None, values_diff=True, bias_diff=True)
    r1 = call(plan)
    ws1 = plan.workspace_bytes
    assert ws1 > ws0
    assert ws1 == plan.stat("device_bytes") + plan.stat("bwd_device_bytes") + plan.stat("upd_device_bytes")
    # the (row, column) -> entry table alone is M x Kd ints
    assert plan.stat("bwd_device_bytes") >= 4 * w.size
    r2 = call(plan)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        r3 = call(plan)
    torch.cuda.synchronize()
    assert plan.workspace_bytes == ws1
    other = _plan(pkg, s, w, tiling_batch=256)
    r4 = call(other)
    torch.cuda.synchronize()
    _ran_mfma(pkg, plan)
    _ran_mfma(pkg, other)
    for a, c, e, f in zip(r1[1:], r2[1:], r3[1:], r4[1:]):
        assert _bytes(a) == _bytes(c) == _bytes(e) == _bytes(f)
    plan.close()
    other.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------
def test_a_double_plan_refuses_and_stays_usable(pkg, dev, synth):
    s, w, x, b, td = _inputs(synth, "d_g3")
    w64 = w.astype(np.float64)
    xt, tdt = torch.from_numpy(x.astype(np.float64)).to(dev), torch.from_numpy(td.astype(np.float64)).to(dev)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s), wgrad_kernel=pkg.WGRAD_MFMA)
    plan.weight_align(w64)
    for _ in range(2):          # a refused build leaves no half-built state behind
        with pytest.raises(pkg.EscoinError) as e:
            plan.backward(tdt, bottom=xt, bottom_diff=None, weight_diff=True)
        assert "failed (-1)" in str(e.value)            # ESCOIN_EINVAL
    with pytest.raises(pkg.EscoinError):
        plan.stat("wgrad_kernel")
    plan.set_option("wgrad_kernel", pkg.WGRAD_AUTO)
    plan.weight_align(w64)
    _, wd, bsd = plan.backward(tdt, bottom=xt, bottom_diff=None, weight_diff=True, bias_diff=True)
    torch.cuda.synchronize()
    want = _ref(synth, "d_g3")
    assert plan.stat("wgrad_kernel") == pkg.WGRAD_ENTRY
    assert rel_err(wd.cpu().numpy(), want[1]) <= 1e-12 and rel_err(bsd.cpu().numpy(), want[2]) <= 1e-12
    plan.close()


# ---- 6. captured training loop -----------------------------------------------------------------------------------------
def test_captured_training_loop_equals_eager_steps(pkg, dev, synth):
    """forward -> backward(values_diff) -> solver_step(SGD with momentum, clear_diff) on d_pw: after one eager step the
    loop is captured on one stream, replayed three times and compared with three eager steps of a second plan: values
    and histories bit for bit."""
    s, w0, x, b, td = _inputs(synth, "d_pw")
    xt, tdt = torch.from_numpy(x).to(dev), torch.from_numpy(td).to(dev)
    bt = torch.from_numpy(b).to(dev)
    hyper = dict(type="sgd", rate=1e-3, momentum=0.9, clear_diff=1)

    def make_plan():
        plan = _plan(pkg, s, w0)
        oh, ow = plan.out_hw
        n = plan.nnz()
        return plan, dict(y=torch.zeros((s.N, s.M, oh, ow), device=dev), vd=torch.zeros(n, device=dev), h=torch.zeros(n, device=dev))

    def step(plan, u):
        plan.forward(xt, bt, u["y"])
        plan.backward(tdt, bottom=xt, bottom_diff=None, values_diff=u["vd"])
        plan.solver_step(u["vd"], u["h"], **hyper)

    def warm(plan, u):
        v0 = plan.get_csr()[2].copy()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step(plan, u)           # builds the backward and update states outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        _ran_mfma(pkg, plan)
        assert plan.stat("update_fast") == 1
        plan.set_values(torch.from_numpy(v0).to(dev))
        u["h"].zero_()
        torch.cuda.synchronize()
        return v0

    ref, ru = make_plan()
    v0 = warm(ref, ru)
    for _ in range(3):
        step(ref, ru)
    torch.cuda.synchronize()

    plan, u = make_plan()
    warm(plan, u)
    ws1 = plan.workspace_bytes
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(plan, u)
    assert plan.workspace_bytes == ws1
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert plan.workspace_bytes == ws1
    _ran_mfma(pkg, plan)
    va, vr = plan.get_csr()[2], ref.get_csr()[2]
    assert va.tobytes() == vr.tobytes() and not np.array_equal(va, v0)
    assert _bytes(u["h"]) == _bytes(ru["h"]) and float(u["h"].abs().max()) > 0
    assert _bytes(u["y"]) == _bytes(ru["y"])
    assert np.all(u["vd"].cpu().numpy() == 0)
    plan.close()
    ref.close()


# ---- 7. set_values -----------------------------------------------------------------------------------------------------------
def test_set_values_does_not_change_the_weight_gradient(pkg, dev, synth):
    s, w, x, b, td = _inputs(synth, "d_3x3")
    xt, tdt = torch.from_numpy(x).to(dev), torch.from_numpy(td).to(dev)
    plan = _plan(pkg, s, w)
    _, vd1, bs1 = plan.backward(tdt, bottom=xt, bottom_diff=None, values_diff=True, bias_diff=True)
    plan.set_values(torch.from_numpy(seeded((plan.nnz(),), 55)).to(dev))
    assert plan.stat("update_fast") == 1
    _, vd2, bs2 = plan.backward(tdt, bottom=xt, bottom_diff=None, values_diff=True, bias_diff=True)
    torch.cuda.synchronize()
    _ran_mfma(pkg, plan)
    assert _bytes(vd1) == _bytes(vd2) and _bytes(bs1) == _bytes(bs2)
    assert rel_err(vd2.cpu().numpy(), _ref(synth, "d_3x3")[1].reshape(-1)[csr_positions(plan)]) <= TOL
    plan.close()
