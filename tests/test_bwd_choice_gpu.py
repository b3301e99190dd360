"""The device path follows the host-only rule (csrc/align_rules.h bwd_choice) on the card at hand -- needs an MI355X.
Eight cases of tests/bwd_choice_common.py, four accepted and four refused, each as a plan of that shape with half of its
weights zeroed: one escoin_backward returns the code and leaves the escoin_last_error text and the stats "wgrad_kernel",
"wgrad_lds_bytes" and "dgrad_lds_bytes" that tests/cpp/bwd_choice_check.cpp prints for the case with this device's CU
count and the plan's nonzero count."""
import numpy as np
import pytest

from bwd_choice_common import BY_NAME, EINVAL, SHAPE_FIELDS, build_checker, run_checker

pytestmark = pytest.mark.gpu

ACCEPTED = ("s1_auto", "s1_generic", "s1_bwd_mfma", "s2_wgrad_mfma")
REFUSED = ("s2_tiled", "s2_staged", "f64_bwd_mfma", "f64_wgrad_mfma")


def _weights(shape, dtype):
    rng = np.random.RandomState(31)
    w = rng.uniform(-1, 1, (shape["M"], shape["C"] // shape["group"], shape["KH"], shape["KW"])).astype(dtype)
    w[rng.uniform(size=w.shape) < 0.5] = 0
    return w


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """name -> (case, weights, what the rule decides on this device for the weights' nonzero count)"""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    tmp = tmp_path_factory.mktemp("bwd_choice_gpu")
    picked = [BY_NAME[n] for n in ACCEPTED + REFUSED]
    weights = {c["name"]: _weights(c["shape"], np.float64 if c["f64"] else np.float32) for c in picked}
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    want = run_checker(build_checker(tmp), tmp, picked, n_cu, {n: int(np.count_nonzero(w)) for n, w in weights.items()})
    return {c["name"]: (c, weights[c["name"]], w) for c, w in zip(picked, want)}


@pytest.mark.parametrize("name", ACCEPTED + REFUSED)
def test_backward_follows_the_host_rule(pkg, cases, name):
    import torch
    case, w, want = cases[name]
    assert (want["rc"] == 0) == (name in ACCEPTED), want
    s = case["shape"]
    desc = pkg.ConvDesc(*([s[k] for k in SHAPE_FIELDS] + [1, 0]))      # (has_bias, no fuse_relu)
    plan = pkg.Plan(desc, backward_kernel=case["bwd"], wgrad_kernel=case["wgrad"])
    plan.weight_align(w)
    dt = torch.float64 if case["f64"] else torch.float32
    gen = torch.Generator().manual_seed(32)
    x = torch.rand((s["N"], s["C"], s["H"], s["W"]), generator=gen, dtype=dt).cuda()
    top_diff = torch.rand((s["N"], s["M"]) + tuple(plan.out_hw), generator=gen, dtype=dt).cuda()
    if want["rc"] == 0:
        plan.backward(top_diff, bottom=x, weight_diff=True, bias_diff=True)
        torch.cuda.synchronize()
        got = {k: plan.stat(k) for k in ("wgrad_kernel", "wgrad_lds_bytes", "dgrad_lds_bytes")}
        print(name, want, got, plan.stat("bwd_data_kernel"))
        assert got == {k: want[k] for k in got}
        if want["data"] == "mfma":
            assert plan.stat("bwd_data_kernel") == 5
    else:
        with pytest.raises(pkg.EscoinError) as e:
            plan.backward(top_diff, bottom=x, weight_diff=True, bias_diff=True)
        print(name, want, e.value)
        assert want["rc"] == EINVAL and str(e.value) == "escoin_backward failed (%d): %s" % (want["rc"], want["error"])
        # no state was built: nothing to report
        assert plan.stat("wgrad_lds_bytes") == want["wgrad_lds_bytes"] == 0
        assert plan.stat("dgrad_lds_bytes") == want["dgrad_lds_bytes"] == 0
        with pytest.raises(pkg.EscoinError):
            plan.stat("wgrad_kernel")
    plan.close()
