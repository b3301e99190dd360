"""The data gradient on the MI355X under option "backward_kernel" = BWD_MFMA (escoin_sconv_dgrad_mfma_kernel): the shapes
of dgrad_mfma_common.SHAPES and a seeded slice of random geometries against torch float64 autograd and the per-element
bound of errbound.py, on inputs whose rows, channels and images differ in scale by up to 2^48 (errbound.skew) -- the bound
is the sparse sum's: the kernel's dense product adds exact zeros for pruned weights.  Partial batches into a NaN-filled
blob, an empty weight block, determinism, in-place weight updates, no allocation after the first call, a captured
forward + backward, refusals.  Every case asserts that the MFMA kernel ran."""
import ctypes

import numpy as np
import pytest

import errbound as eb
from conftest import rel_err
from dgrad_mfma_common import SHAPES, make, random_shapes, weights
from upd_common import new_weights, values_at

torch = pytest.importorskip("torch")

from wgrad_common import seeded, torch_backward  # noqa: E402

pytestmark = pytest.mark.gpu
LDS = 2 * 2 * 32 * 65 * 4


@pytest.fixture(scope="module")
def dev(pkg):
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        pytest.fail("no HIP device visible (these tests run on the MI355X)")
    return torch.device("cuda:0")


_CASES = {}


def _case(synth, s, w_seed=None):
    """(shape, skewed inputs) of a shape: made once, never written."""
    if s.name not in _CASES:
        w = weights(synth, s) if w_seed is None else synth.pruned_weights(s, w_seed)
        x, b = synth.activations(s, 12), synth.bias_vector(s, 13)
        td = seeded((s.N, s.M) + synth.out_hw(s), 21)
        _CASES[s.name] = (s, eb.skew(s, w, x, b, 95, top_diff=td))
    return _CASES[s.name]


def _up(a, dev, dt=np.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)


def _plan(pkg, s, w, relu=False, kernel=None, **opts):
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu), backward_kernel=pkg.BWD_MFMA if kernel is None else kernel, **opts)
    plan.weight_align(w)
    return plan


def _ran_mfma(pkg, plan):
    assert plan.stat("bwd_data_kernel") == pkg.BWD_MFMA == 5
    assert plan.stat("dgrad_lds_bytes") == LDS <= 64 * 1024


def _nan_like(s, dev):
    return torch.full((s.N, s.C, s.H, s.W), float("nan"), device=dev)


def _check_shape(pkg, dev, s, sk, relu):
    """MFMA and gather data gradient of one skewed layer, every element within the bound of the float64 reference."""
    xd, bd_, tdd = _up(sk.x, dev), _up(sk.b, dev), _up(sk.top_diff, dev)
    plan = _plan(pkg, s, sk.w, relu)
    with pytest.raises(pkg.EscoinError):
        plan.stat("bwd_data_kernel")            # nothing has run yet
    top_np = topd = None
    if relu:
        topd = plan.forward(xd, bd_)
        torch.cuda.synchronize()
        top_np = topd.cpu().numpy()
    want, Bs = eb.backward_bound(s, sk.w, sk.x, sk.b, sk.top_diff, top_np)
    what = (s.name, "relu", relu)
    got, _, _ = plan.backward(tdd, top=topd, bottom_diff=_nan_like(s, dev))
    torch.cuda.synchronize()
    _ran_mfma(pkg, plan)
    r = eb.within(got.cpu().numpy(), want[0], Bs[0], "bwd_data_kernel 5", sk.chan_exp, what=what)
    plan.close()
    gather = _plan(pkg, s, sk.w, relu, kernel=pkg.KERNEL_GENERIC)
    ref, _, _ = gather.backward(tdd, top=topd, bottom_diff=_nan_like(s, dev))
    torch.cuda.synchronize()
    assert gather.stat("bwd_data_kernel") == pkg.KERNEL_GENERIC and gather.stat("dgrad_lds_bytes") == 0
    rg = eb.within(ref.cpu().numpy(), want[0], Bs[0], "bwd_data_kernel 1", sk.chan_exp, what=what)
    gather.close()
    print("errbound backward data kernel 5 (MFMA) %-16s relu=%d: %.3g (gather %.3g)" % (s.name, relu, r, rg))
    assert r <= 1.0 and rg <= 1.0


# ---- 1. every shape against the float64 reference ------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_element_within_the_float64_error_bound(pkg, synth, dev, name, relu):
    s, sk = _case(synth, make(synth, name))
    _check_shape(pkg, dev, s, sk, relu)


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
def test_random_geometries_within_the_bound(pkg, synth, dev, relu):
    for i, s in enumerate(random_shapes(synth)):
        s, sk = _case(synth, s, w_seed=100 + i)
        _check_shape(pkg, dev, s, sk, relu)


@pytest.mark.parametrize("name", ["pw_s2", "3x3_s2x3_g2"])
def test_partial_batches_leave_the_other_images_untouched(pkg, synth, dev, name):
    """bottom_diff pre-filled with NaN: images at or past n_images stay NaN, none survives below; n_images = 0 writes nothing."""
    s, sk = _case(synth, make(synth, name))
    tdd = _up(sk.top_diff, dev)
    want, Bs = eb.backward_bound(s, sk.w, sk.x, sk.b, sk.top_diff)
    plan = _plan(pkg, s, sk.w)
    for n in (0, s.N - 1, 1):
        assert 0 <= n < s.N
        full = _nan_like(s, dev)
        # (the C entry point: whole blobs and n_images, as a layer with a partial last batch calls it)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        pkg.check(pkg.lib().escoin_backward(plan._h, None, None, ctypes.c_void_p(tdd.data_ptr()), ctypes.c_void_p(full.data_ptr()),
                                            None, None, n, stream), "escoin_backward")
        torch.cuda.synchronize()
        _ran_mfma(pkg, plan)
        got = full.cpu().numpy()
        assert np.all(np.isnan(got[n:])), (name, n)
        assert not np.any(np.isnan(got[:n])), (name, n)
        eb.within(got[:n], want[0][:n], Bs[0][:n], "bwd_data_kernel 5", sk.chan_exp, what=(name, "n_images", n))
    plan.close()


def test_an_empty_weight_block_is_skipped_and_equals_explicit_zeros(pkg, synth, dev):
    """Rows 32..63 of the weights are zero: K-step 1 of 3 holds no entry and is not run.  The same plan with those zeros
    handed over as explicit CSR zeros runs it: both within the bound of one reference."""
    s, sk = _case(synth, make(synth, "emptyblock"))
    assert not sk.w[32:64].any() and sk.w[:32].all() and sk.w[64:].all()
    tdd = _up(sk.top_diff, dev)
    want, Bs = eb.backward_bound(s, sk.w, sk.x, sk.b, sk.top_diff)
    plan = _plan(pkg, s, sk.w)
    full = pkg.Plan(pkg.ConvDesc.from_shape(s), backward_kernel=pkg.BWD_MFMA)
    full.weight_align_cpu(np.where(sk.w == 0, np.float32(1), sk.w))
    rp, ci, vals, ng = values_at(full, sk.w)
    assert (vals == 0).sum() == 32 * s.C
    full.set_csr(rp, ci, vals, ng)
    got = []
    for p in (plan, full):
        bd, _, _ = p.backward(tdd, bottom_diff=_nan_like(s, dev))
        torch.cuda.synchronize()
        _ran_mfma(pkg, p)
        got.append(bd.cpu().numpy())
        eb.within(got[-1], want[0], Bs[0], "bwd_data_kernel 5", sk.chan_exp, what=("emptyblock", p is full))
    # one more live step (one int) in one (group, phase, channel tile) list; the weight gradient's share grows with nnz
    assert full.stat("bwd_device_bytes") == plan.stat("bwd_device_bytes") + 4 + _slab_delta(s, synth, 32 * s.C)
    plan.close()
    full.close()


def _slab_delta(s, synth, more_nnz):
    """Bytes the backward state grows by with more_nnz more entries, its live lists aside: the weight-gradient slab (one
    float per chunk and entry) and the entries' positions in weight_diff (one int each)."""
    oh, ow = synth.out_hw(s)
    chunks = (s.N * oh * ow + 1023) // 1024
    return 4 * chunks * more_nnz + 4 * more_nnz


# ---- 2. determinism ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pw_s2", "3x3_s2x3_g2"])
def test_determinism_streams_and_images_alone(pkg, synth, dev, name):
    """Two calls on two streams give equal bits; image i computed alone equals image i of the batch bit for bit (the sum
    order does not depend on n_images or on the image's place in a pixel tile)."""
    s, sk = _case(synth, make(synth, name))
    tdd = _up(sk.top_diff, dev)
    plan = _plan(pkg, s, sk.w)
    ws0 = plan.workspace_bytes
    a, _, _ = plan.backward(tdd)
    torch.cuda.synchronize()
    ws1 = plan.workspace_bytes
    assert ws1 > ws0
    assert ws1 == plan.stat("device_bytes") + plan.stat("bwd_device_bytes") + plan.stat("upd_device_bytes")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b, _, _ = plan.backward(tdd)
    torch.cuda.synchronize()
    assert plan.workspace_bytes == ws1                  # no allocation after the first call
    _ran_mfma(pkg, plan)
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert np.array_equal(a, b) and np.all(np.isfinite(a)) and np.abs(a).max() > 0
    for i in range(s.N):
        one, _, _ = plan.backward(tdd[i:i + 1].contiguous())
        torch.cuda.synchronize()
        assert np.array_equal(one.cpu().numpy()[0], a[i]), (name, i)
    plan.close()


# ---- 3. in-place weight updates reach the phase matrices ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pw_s2", "3x3_s2x3_g2"])
def test_updates_reach_the_phase_matrices_in_place(pkg, synth, dev, name):
    """After set_values, update_values (device source) and one solver step the MFMA data gradient equals, bit for bit,
    that of a fresh plan aligned by set_csr on the new values; the update list grew by nnz with the backward state."""
    s, sk = _case(synth, make(synth, name))
    tdd = _up(sk.top_diff, dev)
    plan = _plan(pkg, s, sk.w)
    nnz = plan.nnz()
    assert nnz > 0

    def fresh_equals(step):
        rp, ci, vals, ng = plan.get_csr()               # (brings the host values up to date)
        fresh = pkg.Plan(pkg.ConvDesc.from_shape(s), backward_kernel=pkg.BWD_MFMA)
        fresh.set_csr(rp, ci, vals, ng)
        got, _, _ = plan.backward(tdd, bottom_diff=_nan_like(s, dev))
        ref, _, _ = fresh.backward(tdd, bottom_diff=_nan_like(s, dev))
        torch.cuda.synchronize()
        _ran_mfma(pkg, plan)
        _ran_mfma(pkg, fresh)
        fresh.close()
        got, ref = got.cpu().numpy(), ref.cpu().numpy()
        assert np.array_equal(got, ref) and np.all(np.isfinite(got)), (name, step)
        return got

    w1, _ = new_weights(sk.w, 41)
    plan.set_values(_up(values_at(plan, w1)[2], dev))   # before the backward state exists
    assert plan.stat("update_fast") == 1
    before = plan.stat("update_destinations")
    g0 = fresh_equals("set_values before the first backward")
    w2, w2_nan = new_weights(sk.w, 42)
    plan.set_values(_up(values_at(plan, w2)[2], dev))
    assert plan.stat("update_fast") == 1
    assert plan.stat("update_destinations") == before + nnz
    g1 = fresh_equals("set_values")
    assert not np.array_equal(g0, g1)
    w3, w3_nan = new_weights(sk.w, 43)
    plan.update_values(_up(w3_nan, dev))                # device source, NaN outside the pattern
    assert plan.stat("update_fast") == 1
    g2 = fresh_equals("update_values")
    assert not np.array_equal(g1, g2)
    vd, h = _up(seeded((nnz,), 44), dev), torch.zeros(nnz, device=dev)
    plan.solver_step(vd, h, type="sgd", rate=0.05, momentum=0.9)
    assert plan.stat("update_fast") == 1
    assert plan.stat("update_destinations") == before + nnz
    g3 = fresh_equals("solver_step")
    assert not np.array_equal(g2, g3)
    plan.close()


# ---- 4. captured forward + backward ------------------------------------------------------------------------------------------
def test_forward_and_mfma_backward_captured_into_one_graph(pkg, synth, dev):
    """After a warm-up, forward + backward (MFMA data gradient, fuse_relu) captured into one graph and replayed twice on
    new data: each replay equals the eager result bit for bit, and nothing is allocated."""
    s = make(synth, "3x3_s2x3_g2")
    w, b = weights(synth, s), synth.bias_vector(s, 13)
    plan = _plan(pkg, s, w, relu=True)
    oh, ow = plan.out_hw
    u = dict(x=torch.zeros((s.N, s.C, s.H, s.W), device=dev), td=torch.zeros((s.N, s.M, oh, ow), device=dev),
             y=torch.zeros((s.N, s.M, oh, ow), device=dev), bd=torch.zeros((s.N, s.C, s.H, s.W), device=dev), b=_up(b, dev))

    def step():
        plan.forward(u["x"], u["b"], u["y"])
        plan.backward(u["td"], top=u["y"], bottom_diff=u["bd"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                      # warm-up: builds the backward state outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _ran_mfma(pkg, plan)
    ws1 = plan.workspace_bytes
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    assert plan.workspace_bytes == ws1
    for rnd in range(2):
        u["x"].copy_(torch.from_numpy(synth.activations(s, 900 + rnd)))
        u["td"].copy_(torch.from_numpy(seeded(tuple(u["td"].shape), 950 + rnd)))
        u["bd"].fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        replayed = u["bd"].cpu().numpy().copy()
        u["bd"].fill_(float("nan"))
        step()
        torch.cuda.synchronize()
        eager = u["bd"].cpu().numpy()
        assert np.array_equal(replayed, eager) and np.all(np.isfinite(eager)) and np.abs(eager).max() > 0, rnd
    assert plan.workspace_bytes == ws1
    plan.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_a_double_plan_refuses_and_stays_usable(pkg, synth, dev):
    s = make(synth, "3x3_s2")
    w64 = weights(synth, s).astype(np.float64)
    td = seeded((s.N, s.M) + synth.out_hw(s), 21, np.float64)
    tdt = torch.from_numpy(td).to(dev)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s), backward_kernel=pkg.BWD_MFMA)
    plan.weight_align(w64)
    for _ in range(2):          # a refused build leaves no half-built state behind
        with pytest.raises(pkg.EscoinError) as e:
            plan.backward(tdt)
        assert "failed (-1)" in str(e.value)            # ESCOIN_EINVAL
    with pytest.raises(pkg.EscoinError):
        plan.stat("bwd_data_kernel")
    # the refused plan still runs its forward; the same weights on a new plan with the default option get the gather kernel
    x64 = synth.activations(s, 12).astype(np.float64)
    y = plan.forward(torch.from_numpy(x64).to(dev))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
    plan.close()
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
    plan.weight_align(w64)
    got, _, _ = plan.backward(tdt)
    torch.cuda.synchronize()
    assert plan.stat("bwd_data_kernel") == pkg.KERNEL_GENERIC
    want = torch_backward(np.zeros((s.N, s.C, s.H, s.W)), w64, None, s, td)[0]
    assert rel_err(got.cpu().numpy(), want) <= 1e-12
    plan.close()
