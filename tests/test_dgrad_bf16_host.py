"""Plan option "dgrad_math" without a GPU: its values and refusals by name, the new stat before any launch, and
align_rules.h dgb_plan (through tests/cpp/dgrad_bf16_rule_check.cpp, plain g++: the rule is host-only) on the shapes that
test_dgrad_bf16_gpu.py shares: dgrad_mfma_common.SHAPES without the full-size layer, and one with three live steps."""
import os
import subprocess

import numpy as np
import pytest

import dgrad_mfma_common as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS = 2 * 2 * 64 * 64 * 2      # 2 buffers x (weights, G) x 64 rows x 64 bf16
# name: (N, C, H, W, M, KH, kwargs of synth.shape)
SHAPES = {k: v for k, v in dc.SHAPES.items() if k != "res3a_branch2a"}
SHAPES["steps3"] = (1, 64, 8, 8, 70, 1, dict(stride=2, sparsity=0.3))     # Kp = 70: live steps {0, 1, 2}, one pair and an odd tail


def make(synth, name):
    N, C, H, W, M, K, kw = SHAPES[name]
    return synth.shape(name, N, C, H, W, M, K, **kw)


def test_option_values_refusals_and_the_stat_before_any_launch(pkg, synth):
    s = make(synth, "3x3_s2")
    w = synth.pruned_weights(s, 1)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s), backward_kernel=pkg.BWD_MFMA, dgrad_math=pkg.MATH_BF16)
    plan.set_option("dgrad_math", 0)
    for v in (2, -1):
        with pytest.raises(pkg.EscoinError) as e:
            plan.set_option("dgrad_math", v)
        assert "failed (-1)" in str(e.value) and "dgrad_math must be" in str(e.value)        # ESCOIN_EINVAL, by name
    plan.set_option("dgrad_math", 1)
    plan.weight_align_cpu(w)                                    # CPU mode ignores it
    plan.set_option("dgrad_math", 0)                            # ... and an aligned plan takes it
    plan.set_option("dgrad_math", 1)
    assert [plan.stat(k) for k in ("dgrad_math", "dgrad_lds_bytes")] == [0, 0]      # nothing has run
    with pytest.raises(pkg.EscoinError, match="dgrad_math = 1 .*double"):          # a double align of a plan that asks for bf16
        plan.weight_align_cpu(w.astype(np.float64))
    plan.close()
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
    plan.weight_align_cpu(w.astype(np.float64))
    with pytest.raises(pkg.EscoinError, match="dgrad_math = 1 .*double"):          # ... and bf16 asked of a double plan
        plan.set_option("dgrad_math", 1)
    plan.close()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    out = str(tmp_path_factory.mktemp("dgb") / "dgrad_bf16_rule_check")
    srcs = [os.path.join(ROOT, "tests", "cpp", "dgrad_bf16_rule_check.cpp")] + [
        os.path.join(csrc, f) for f in ("align_rules.cpp", "csr_tables.cpp", "stream_builder.cpp", "jit_codegen.cpp")]
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-o", out] + srcs + ["-lpthread"])
    return out


@pytest.mark.parametrize("name", list(SHAPES))
def test_rule_gives_the_fp32_kernels_tile_plan_and_the_bf16_lds_bytes(exe, synth, name):
    s = make(synth, name)

    def rule(f64):
        words = list(s[1:15]) + [int(f64)]
        return [int(v) for v in subprocess.check_output([exe] + [str(v) for v in words], timeout=60).decode().split()[1:]]
    ph = dc.phases(s)
    mg = s.M // s.group
    cols_total = sum(-(-mg * len(p["taps"]) // 32) * 32 for p in ph)
    tiles_max = max(-(-s.N * p["rows"] * p["cols"] // 64) for p in ph)
    assert rule(False) == [1, LDS, s.stride_h * s.stride_w, -(-(s.C // s.group) // 64), cols_total, tiles_max] and LDS == 32768
    assert rule(True)[0] == 0                                   # float plans only
