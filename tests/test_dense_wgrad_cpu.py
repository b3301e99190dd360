"""escoin_dense_wgrad_cpu[_f64] without a GPU: the dense weight gradient -- every position of blobs_[0], inside and outside
the pattern -- on every shape of wgrad_mfma_common.ALL, float and double, plain and fuse_relu, against torch float64
autograd with an all-ones mask and the per-element bound of errbound.backward_bound (its term count N*OH*OW + 4 covers
any summation order); accumulation, thread-count independence, partial batches, the errors, and agreement with
backward_cpu's masked gradient inside the pattern."""
import numpy as np
import pytest

import errbound as eb
from wgrad_mfma_common import ALL, make

torch = pytest.importorskip("torch")

from wgrad_common import csr_positions, seeded  # noqa: E402

_INPUTS = {}


def _inputs(synth, name, dt):
    """(shape, weights, activations, bias, top_diff) of a named shape in dtype dt: made once, never written."""
    if (name, dt) not in _INPUTS:
        s = make(synth, name)
        oh, ow = synth.out_hw(s)
        b = synth.bias_vector(s, 13)
        _INPUTS[(name, dt)] = (s, synth.pruned_weights(s, 11).astype(dt), synth.activations(s, 12).astype(dt),
                               None if b is None else b.astype(dt), seeded((s.N, s.M, oh, ow), 21).astype(dt))
    return _INPUTS[(name, dt)]


def _plan(pkg, s, w, relu=False):
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu))
    plan.weight_align_cpu(w)
    return plan


def _bound(s, w, x, b, td, top, f64, n=None):
    """(float64 dense gradient, its per-element bound) of the first n images."""
    want, Bs = eb.backward_bound(s, w, x[:n], b, td[:n], None if top is None else top[:n], f64=f64,
                                 mask=np.ones_like(w, bool))
    return want[1], Bs[1]


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(ALL))
def test_every_position_within_the_float64_bound(pkg, synth, name, dt, relu):
    s, w, x, b, td = _inputs(synth, name, dt)
    plan = _plan(pkg, s, w, relu)
    top = plan.forward_cpu(x, b, n_threads=4) if relu else None
    got = plan.dense_wgrad_cpu(td, x, top=top, n_threads=4)
    assert got.shape == w.shape and got.dtype == dt
    want, B = _bound(s, w, x, b, td, top, dt == np.float64)
    r = eb.within(got, want, B, "dense_wgrad_cpu", what=(name, dt.__name__, relu))
    # outside the pattern the gradient is there too -- what the masked paths never write
    assert np.any(got[w == 0] != 0) or not np.any(w == 0)
    # inside the pattern: backward_cpu's masked gradient, within the same bound
    _, wd, _ = plan.backward_cpu(td, bottom=x, top=top, bottom_diff=None, weight_diff=True, n_threads=4)
    pos = csr_positions(plan)
    assert np.all(np.abs(got.reshape(-1)[pos].astype(np.float64) - wd.reshape(-1)[pos]) <= B.reshape(-1)[pos])
    print("dense_wgrad_cpu %-12s %s relu=%d: %.3g of the bound" % (name, dt.__name__, relu, r))
    plan.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["d_3x3", "d_g3", "dil2_asym"])
def test_accumulate_adds_onto_a_prefilled_blob_with_one_rounding(pkg, synth, name, dt):
    s, w, x, b, td = _inputs(synth, name, dt)
    plan = _plan(pkg, s, w)
    pre = seeded(w.shape, 31).astype(dt)
    alone = plan.dense_wgrad_cpu(td, x)
    out = pre.copy()
    assert plan.dense_wgrad_cpu(td, x, out=out, accumulate=True) is out
    assert out.tobytes() == (pre + alone).tobytes()
    want, B = _bound(s, w, x, b, td, None, dt == np.float64)
    oh, ow = synth.out_hw(s)
    eb.within(out, want + pre, eb.accumulated_bound(B, pre, s.N * oh * ow, f64=dt == np.float64), "dense_wgrad_cpu accumulate", what=name)
    # overwrite clears whatever was there
    junk = np.full(w.shape, np.nan, dt)
    plan.dense_wgrad_cpu(td, x, out=junk)
    assert junk.tobytes() == alone.tobytes()
    plan.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["straddle3x3", "d_pw", "small7x7g2"])
def test_bits_do_not_depend_on_the_thread_count(pkg, synth, name, dt):
    s, w, x, b, td = _inputs(synth, name, dt)
    plan = _plan(pkg, s, w, relu=True)
    top = plan.forward_cpu(x, b, n_threads=2)
    a = plan.dense_wgrad_cpu(td, x, top=top, n_threads=1)
    c = plan.dense_wgrad_cpu(td, x, top=top, n_threads=4)
    assert a.tobytes() == c.tobytes() and np.any(a != 0)
    plan.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["d_pw", "d_conv1", "small7x7g2"])
def test_partial_batches_never_read_the_images_past_n_images(pkg, synth, name, dt):
    s, w, x, b, td = _inputs(synth, name, dt)
    plan = _plan(pkg, s, w)
    for n in (0, 1, s.N):
        xn, tdn = x.copy(), td.copy()
        xn[n:] = np.nan
        tdn[n:] = np.nan
        got = plan.dense_wgrad_cpu(tdn, xn, n_images=n)
        if n == 0:
            assert np.all(got == 0)
            pre = seeded(w.shape, 32).astype(dt)
            out = pre.copy()
            plan.dense_wgrad_cpu(tdn, xn, out=out, accumulate=True, n_images=0)
            assert out.tobytes() == pre.tobytes()
            continue
        want, B = _bound(s, w, x, b, td, None, dt == np.float64, n)
        eb.within(got, want, B, "dense_wgrad_cpu partial", what=(name, n))
    plan.close()


def test_the_result_does_not_depend_on_the_pattern_or_the_values(pkg, synth):
    s, w, x, b, td = _inputs(synth, "d_g3", np.float32)
    a = _plan(pkg, s, w)
    c = _plan(pkg, s, np.where(seeded(w.shape, 41) > 0.5, np.float32(3), np.float32(0)))
    assert a.nnz() != c.nnz()
    assert a.dense_wgrad_cpu(td, x).tobytes() == c.dense_wgrad_cpu(td, x).tobytes()
    a.close()
    c.close()


def test_the_result_feeds_rewire_cpu_as_its_score(pkg, synth):
    import rewire_common as rc
    s, w, x, b, td = _inputs(synth, "d_g3", np.float32)
    plan = _plan(pkg, s, w)
    score = plan.dense_wgrad_cpu(td, x)
    csr = plan.get_csr()
    k = 7
    want = rc.ref_rewire(plan.desc, csr, k, score, drop_keep=plan.nnz() - k)
    entry_map, grown = plan.rewire_cpu(k, score, drop_keep=plan.nnz() - k)
    assert np.array_equal(entry_map, want["entry_map"]) and np.array_equal(grown, want["grown"])
    plan.close()


def test_errors(pkg, synth):
    s, w, x, b, td = _inputs(synth, "d_g3", np.float32)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
    with pytest.raises(pkg.EscoinError) as e:
        plan.dense_wgrad_cpu(td, x)
    assert "failed (-4)" in str(e.value)                                  # ESCOIN_ESTATE: before an align
    plan.weight_align_cpu(w)
    out = np.zeros(w.shape, np.float32)
    L, p = pkg.lib(), pkg._np_ptr
    bad = [(None, p(td), p(out), s.N), (p(x), None, p(out), s.N), (p(x), p(td), None, s.N), (p(x), p(td), p(out), -1)]
    for xb, tdb, ob, n in bad:
        assert L.escoin_dense_wgrad_cpu(plan._h, xb, None, tdb, ob, n, 0, 1) == -1      # ESCOIN_EINVAL
        assert L.escoin_last_error() != b""
    # the other Dtype's entry point
    with pytest.raises(pkg.EscoinError) as e:
        plan.dense_wgrad_cpu(td.astype(np.float64), x.astype(np.float64))
    assert "failed (-4)" in str(e.value)
    plan.close()
    relu = _plan(pkg, s, w, relu=True)
    with pytest.raises(pkg.EscoinError) as e:
        relu.dense_wgrad_cpu(td, x)                                       # fuse_relu without top
    assert "failed (-1)" in str(e.value) and "top" in str(e.value)
    relu.close()
