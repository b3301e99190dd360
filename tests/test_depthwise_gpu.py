"""Plan option "depthwise" on the MI355X: every shape of depthwise_common.py under "depthwise_band_rows" in (0, 1, 2) bit for bit
against the generic kernels and within errbound's bound of the float64 reference; stats; unserved plans; an in-place update."""
import numpy as np
import pytest

import depthwise_common as dc
import errbound as eb
from upd_common import new_weights, values_at

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(pkg):
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        pytest.fail("no HIP device visible (these tests run on the MI355X)")
    return torch.device("cuda:0")


def _up(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _plan(pkg, s, w, relu=False, **opts):
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu), **opts)
    plan.weight_align(w)
    return plan


def _on(pkg, s, w, band_rows, relu=False):
    plan = _plan(pkg, s, w, relu, depthwise=1, depthwise_band_rows=band_rows)
    assert plan.stat("depthwise") == 1 and "escoin_depthwise_kernel" in plan.kernel_name
    assert 0 < plan.stat("depthwise_lds_bytes") <= 4 * dc.WAVE_LDS <= 160 * 1024
    assert 1 <= plan.stat("depthwise_band_rows") <= (band_rows or 1 << 30)
    return plan


def _forward(plan, x, b, dev):
    return plan.forward(_up(x, dev), _up(b, dev)).cpu().numpy()


def _backward(plan, s, x, td, dev, top=None):
    """[bottom_diff, weight_diff, bias_diff] as numpy; bottom_diff into a NaN-filled blob.  top: the forward's, on a fuse_relu plan."""
    full = torch.full((s.N, s.C, s.H, s.W), float("nan"), device=dev)
    out = plan.backward(_up(td, dev), bottom=_up(x, dev), top=_up(top, dev), bottom_diff=full, weight_diff=True,
                        bias_diff=True if s.bias else None)
    return [None if t is None else t.cpu().numpy() for t in out]


@pytest.mark.parametrize("band_rows", dc.BAND_ROWS)
@pytest.mark.parametrize("name,bias,relu", [(n, True, False) for n in dc.SHAPES] + [("mult2", True, True)] + [
    (n, bias, relu) for n in ("3x3_s1", "3x3_s2") for bias, relu in ((False, False), (True, True), (False, True))])
def test_forward_and_data_gradient_are_the_generic_kernels_bits(pkg, synth, dev, name, bias, relu, band_rows):
    s, w, x, b, td = dc.case(synth, name)
    s, b = s._replace(bias=bias), b if bias else None
    plan = _on(pkg, s, w, band_rows, relu)
    generic = _plan(pkg, s, w, relu, kernel=pkg.KERNEL_GENERIC, backward_kernel=pkg.KERNEL_GENERIC)
    off = _plan(pkg, s, w, relu)
    # forward
    want, B = eb.forward_bound(s, w, x, b, relu=relu)
    got = _forward(plan, x, b, dev)
    assert np.array_equal(got, _forward(generic, x, b, dev))
    eb.within(got, want, B, "escoin_depthwise_kernel", what=(name, band_rows))
    if name == "pruned":
        assert plan.get_csr()[0][0] == plan.get_csr()[0][1] and np.array_equal(got[:, 0], np.broadcast_to(b[0], got[:, 0].shape))      # the empty row: the bias
    # a partial batch: the top of images at or past n_images stays as it was
    top, xd, bd = torch.full(got.shape, float("nan"), device=dev), _up(x, dev), _up(b, dev)
    plan.forward_ptr(xd.data_ptr(), bd.data_ptr() if bias else 0, top.data_ptr(), s.N - 1)       # (torch's current stream is the default one)
    assert np.array_equal(top.cpu().numpy()[:s.N - 1], got[:s.N - 1]) and np.isnan(top.cpu().numpy()[s.N - 1:]).all()
    # data gradient; the weight and bias gradients are those of the plan without the option
    mask = got if relu else None
    grads = _backward(plan, s, x, td, dev, mask)
    assert plan.stat("bwd_data_kernel") == pkg.BWD_DEPTHWISE == 6 and 0 < plan.stat("dgrad_lds_bytes") <= 4 * dc.WAVE_LDS
    want, Bs = eb.backward_bound(s, w, x, b, td, mask)
    eb.within(grads[0], want[0], Bs[0], "escoin_depthwise_dgrad_kernel", what=(name, band_rows))
    assert np.array_equal(grads[0], _backward(generic, s, x, td, dev, mask)[0]) and generic.stat("bwd_data_kernel") == pkg.KERNEL_GENERIC
    assert all(np.array_equal(g, v) for g, v in zip(grads[1:], _backward(off, s, x, td, dev, mask)[1:]))
    [p.close() for p in (plan, generic, off)]


@pytest.mark.parametrize("what", ["cg2", "double", "dense", "lowered"])
def test_unserved_plans_run_as_without_the_option(pkg, synth, dev, what):
    s, w, x, b, td = dc.case(synth, "cg2" if what == "cg2" else "3x3_s1")
    opts = dict(dense=dict(kernel=pkg.KERNEL_DENSE), lowered=dict(conv_mode=pkg.CONV_MODE_LOWERED_SPARSE)).get(what, {})
    if what == "double":
        w, x, b, td = (a.astype(np.float64) for a in (w, x, b, td))
    on, off = _plan(pkg, s, w, depthwise=1, **opts), _plan(pkg, s, w, **opts)
    assert on.stat("depthwise") == 0 and on.kernel_name == off.kernel_name and "depthwise" not in on.kernel_name
    assert np.array_equal(_forward(on, x, b, dev), _forward(off, x, b, dev))
    if what in ("cg2", "double"):       # (a forced "kernel" and a lowered mode name the forward alone)
        got, want = on.backward(_up(td, dev))[0], off.backward(_up(td, dev))[0]
        assert on.stat("bwd_data_kernel") == off.stat("bwd_data_kernel") != dc.BWD_DEPTHWISE and torch.equal(got, want)


def test_update_in_place_equals_a_fresh_plan(pkg, synth, dev):
    s, w, x, b, td = dc.case(synth, "mult2")
    plan = _on(pkg, s, w, 2)
    _backward(plan, s, x, td, dev)                      # (the backward state exists before the update)
    w_new, w_nan = new_weights(w, 31)
    plan.update_values(w_nan)
    fresh = pkg.Plan(pkg.ConvDesc.from_shape(s), depthwise=1)
    fresh.set_csr(*values_at(plan, w_new))
    assert np.array_equal(_forward(plan, x, b, dev), _forward(fresh, x, b, dev))
    assert all(np.array_equal(g, v) for g, v in zip(_backward(plan, s, x, td, dev), _backward(fresh, s, x, td, dev)))
    assert plan.stat("bwd_data_kernel") == dc.BWD_DEPTHWISE
