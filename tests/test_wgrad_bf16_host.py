"""Plan option "wgrad_math" without a GPU: its values and refusals by name, the new stats before any launch, and
align_rules.h wgb_plan (through tests/cpp/wgrad_bf16_rule_check.cpp, plain g++: the rule is host-only) on the shapes that
test_wgrad_bf16_gpu.py shares: eight of wgrad_mfma_common.ALL and three that reach the 16-byte staging paths."""
import os
import subprocess

import numpy as np
import pytest

from wgrad_mfma_common import ALL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS = 2 * 2 * 64 * 64 * 2      # 2 buffers x (G, X) x 64 rows x 64 bf16
# name: (N, C, H, W, M, KH, kwargs of synth.shape)
SHAPES = {k: ALL[k] for k in ("d_pw", "d_3x3", "d_conv1", "d_s2pw", "d_g3", "d_onepx", "small7x7g2", "dil2_asym")}
SHAPES.update({
    "b_pw4": (5, 72, 12, 12, 70, 1, dict(sparsity=0.0)),         # 720 px: 11 steps + a 16-pixel tail; column tiles of 64 + 8; G and X by 16 bytes
    "b_pw4x": (9, 8, 12, 12, 8, 1, dict(sparsity=0.5)),          # 1296 px: the chunk boundary at pixel 16 of image 7
    "b_3x3v": (2, 8, 12, 12, 8, 3, dict(pad=1, sparsity=0.5)),   # G by 16 bytes, X gathered
})
# (vec_g, vec_x) the rule allows: OH*OW % 4 == 0; and 1x1, stride 1, pad 0 on top of it
RULE = {"d_pw": (0, 0), "d_3x3": (1, 0), "d_conv1": (0, 0), "d_s2pw": (1, 0), "d_g3": (0, 0), "d_onepx": (0, 0),
        "small7x7g2": (0, 0), "dil2_asym": (0, 0), "b_pw4": (1, 1), "b_pw4x": (1, 1), "b_3x3v": (1, 0)}


def make(synth, name):
    N, C, H, W, M, K, kw = SHAPES[name]
    return synth.shape(name, N, C, H, W, M, K, **kw)


def test_option_values_refusals_and_stats_before_any_launch(pkg, synth):
    s = make(synth, "b_3x3v")
    w = synth.pruned_weights(s, 1)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s), wgrad_kernel=pkg.WGRAD_MFMA, wgrad_math=pkg.MATH_BF16)
    plan.set_option("wgrad_math", 0)
    for v in (2, -1):
        with pytest.raises(pkg.EscoinError) as e:
            plan.set_option("wgrad_math", v)
        assert "failed (-1)" in str(e.value) and "wgrad_math must be" in str(e.value)        # ESCOIN_EINVAL, by name
    plan.set_option("wgrad_math", 1)
    plan.weight_align_cpu(w)                                    # CPU mode ignores it
    plan.set_option("wgrad_math", 0)                            # ... and an aligned plan takes it
    plan.set_option("wgrad_math", 1)
    assert [plan.stat(k) for k in ("wgrad_math", "dwg_math", "wgrad_lds_bytes", "dwg_lds_bytes")] == [0, 0, 0, 0]   # nothing has run
    with pytest.raises(pkg.EscoinError, match="wgrad_math = 1 .*double"):          # a double align of a plan that asks for bf16
        plan.weight_align_cpu(w.astype(np.float64))
    plan.close()
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
    plan.weight_align_cpu(w.astype(np.float64))
    with pytest.raises(pkg.EscoinError, match="wgrad_math = 1 .*double"):          # ... and bf16 asked of a double plan
        plan.set_option("wgrad_math", 1)
    plan.close()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    out = str(tmp_path_factory.mktemp("wgb") / "wgrad_bf16_rule_check")
    srcs = [os.path.join(ROOT, "tests", "cpp", "wgrad_bf16_rule_check.cpp")] + [
        os.path.join(csrc, f) for f in ("align_rules.cpp", "csr_tables.cpp", "stream_builder.cpp", "jit_codegen.cpp")]
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-o", out] + srcs + ["-lpthread"])
    return out


@pytest.mark.parametrize("name", list(SHAPES))
def test_rule_gives_the_lds_bytes_and_the_operands_that_may_load_16_bytes(exe, synth, name):
    s = make(synth, name)

    def rule(f64):
        words = list(s[1:15]) + [int(f64)]
        return [int(v) for v in subprocess.check_output([exe] + [str(v) for v in words], timeout=60).decode().split()[1:]]
    oh, ow = synth.out_hw(s)
    mg, kdim = s.M // s.group, s.C // s.group * s.KH * s.KW
    assert rule(False) == [1, LDS, RULE[name][0], RULE[name][1], -(-mg // 64), -(-kdim // 64), -(-s.N * oh * ow // 1024)]
    assert RULE[name][0] == int(oh * ow % 4 == 0) and LDS == 32768
    assert rule(True)[0] == 0                                   # float plans only
