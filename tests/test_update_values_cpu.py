"""escoin_update_values_cpu[_f64]: new weights at the old pattern on plans that live on the host (no GPU needed).  The
reference point is always a fresh CPU-aligned plan on the new weights; equality is np.array_equal, no tolerance.  The
oracle is consulted once per case on top, so that "both wrong in the same way" cannot pass."""
import ctypes as C

import numpy as np
import pytest

from conftest import Golden, GOLDEN_DIR, rel_err
from upd_common import new_weights, same_bits, values_at

import os

CASES = ["lenet_conv2_n2", "alex_like_g2_k5p2", "ref_group3", "ref_simple_k3s2", "ref_dilated_k3d2", "googlenet_like_1x1",
         "nonsquare_k3x5_s1x2_p1x2", "res5_like_nobias"]


def _seeded(shape, seed, dt):
    return np.random.RandomState(seed).uniform(-1, 1, shape).astype(dt)


def _run(plan, x, bias, td):
    top = plan.forward_cpu(x, bias, n_threads=3)
    bd, wd, bsd = plan.backward_cpu(td, bottom=x, weight_diff=True, bias_diff=True if bias is not None else None, n_threads=2)
    return top, bd, wd, bsd


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["float", "double"])
def test_update_values_cpu_equals_a_fresh_plan(pkg, oracle, name, dt):
    gd = Golden(os.path.join(GOLDEN_DIR, name + ".npz"))
    x, w = gd.x.astype(dt), gd.w.astype(dt)
    bias = None if gd.bias is None else gd.bias.astype(dt)
    plan = pkg.Plan(gd.desc(pkg))
    plan.weight_align_cpu(w)
    rp0, ci0, _, ng0 = plan.get_csr()
    td = _seeded((gd.N, gd.M) + plan.out_hw, 3, dt)
    _, _, wd_before, _ = _run(plan, x, bias, td)

    # (a) every kept weight replaced by a nonzero value; everything outside the pattern is NaN and must not be read
    w_new, w_nan = new_weights(w, 17, zeros=False)
    plan.update_values_cpu(w_nan)
    fresh = pkg.Plan(gd.desc(pkg))
    fresh.weight_align_cpu(w_new)
    got, want = _run(plan, x, bias, td), _run(fresh, x, bias, td)
    for a, b in zip(got, want):
        assert (a is None and b is None) or np.array_equal(a, b)
    g = gd.geom(oracle)
    ref = oracle.conv_forward_f64(g, x, w_new, bias) if dt == np.float64 else oracle.conv_forward(g, x, w_new, bias, gate=False)
    print("%s %s: forward vs oracle rel_err=%.3g" % (name, dt.__name__, rel_err(got[0], ref)))
    assert rel_err(got[0], ref) <= 1e-4
    rp, ci, va, ng = plan.get_csr()
    assert np.array_equal(rp, rp0) and np.array_equal(ci, ci0) and np.array_equal(ng, ng0)
    assert same_bits(va, values_at(plan, w_new)[2]) and same_bits(va, fresh.get_csr()[2])
    assert plan.stat("update_count") == 1

    # (b) a few kept weights become exactly 0 and one -0.0: they stay in the CSR as explicit zeros.  (weight_align_cpu
    # on the new blob would drop them; a zero term changes no sum, so forward and data gradient still equal the fresh
    # plan's, and the weight gradient -- a function of bottom and top_diff alone -- still reaches every old position.)
    w_zero, w_zero_nan = new_weights(w, 23, zeros=True)
    assert np.count_nonzero(w_zero) < np.count_nonzero(w)
    plan.update_values_cpu(w_zero_nan)
    fresh.weight_align_cpu(w_zero)
    got, want = _run(plan, x, bias, td), _run(fresh, x, bias, td)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], wd_before)
    rp, ci, va, ng = plan.get_csr()
    assert np.array_equal(rp, rp0) and np.array_equal(ci, ci0) and np.array_equal(ng, ng0)
    want_va = values_at(plan, w_zero)[2]
    assert same_bits(va, want_va) and np.count_nonzero(va == 0) >= 4 and np.any(np.signbit(va) & (va == 0))
    plan.close()
    fresh.close()


def test_update_values_cpu_errors(pkg):
    L = pkg.lib()
    d = pkg.ConvDesc(1, 2, 5, 5, 2, 3, 3, 1, 1, 1, 1, 1, 1, 1, 0, 0)
    w = np.zeros((2, 2, 3, 3), np.float32)
    w[0, 0, 1, 1] = 1.0
    w[1, 1, 0, 2] = -2.0
    plan = pkg.Plan(d)
    p32, p64 = w.ctypes.data_as(C.c_void_p), w.astype(np.float64).ctypes.data_as(C.c_void_p)
    assert L.escoin_update_values_cpu(plan._h, p32) == -4            # ESCOIN_ESTATE: before an align
    assert "before" in L.escoin_last_error().decode()
    plan.weight_align_cpu(w)
    assert L.escoin_update_values_cpu(plan._h, None) == -1           # ESCOIN_EINVAL
    assert L.escoin_update_values_cpu(None, p32) == -1
    assert L.escoin_update_values_cpu_f64(plan._h, p64) == -4        # the other Dtype's entry point
    assert L.escoin_update_values_cpu(plan._h, p32) == 0
    plan.weight_align_cpu(w.astype(np.float64))
    assert L.escoin_update_values_cpu(plan._h, p32) == -4
    assert L.escoin_update_values_cpu_f64(plan._h, p64) == 0
    # the GPU entry points: NULL is refused first; without a device they say so and compute nothing
    for fn in (L.escoin_update_values, L.escoin_plan_set_values):
        assert fn(plan._h, None, 0, None) == -1
        assert fn(None, p32, 0, None) == -1
    if pkg.device_count() == 0:
        for fn, ptr in ((L.escoin_update_values, p32), (L.escoin_plan_set_values, p32), (L.escoin_update_values_f64, p64),
                        (L.escoin_plan_set_values_f64, p64)):
            assert fn(plan._h, ptr, 0, None) == -5                   # ESCOIN_ENODEVICE
            assert "no HIP device" in L.escoin_last_error().decode()
    else:
        assert L.escoin_update_values(plan._h, p32, 0, None) == -4   # a CPU-aligned plan has no device side
    for key in ("update_fast", "update_count", "update_destinations", "upd_device_bytes"):
        assert plan.stat(key) >= 0
    assert plan.stat("upd_device_bytes") == 0 and plan.workspace_bytes == 0
    plan.close()
