"""Plan option "dense_math" without a GPU: its values and refusals, align_rules.h db16_plan (through
tests/cpp/dense_bf16_rule_check.cpp, plain g++) on the cases of dense_bf16_common.py, and that module's bf16 rounding
against torch.bfloat16."""
import os
import subprocess

import numpy as np
import pytest

import dense_bf16_common as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_values_and_refusals(pkg, synth):
    assert (pkg.MATH_FP32, pkg.MATH_BF16) == (0, 1)
    s = synth.shape("b16_opt", 2, 8, 6, 6, 8, 3, pad=1, sparsity=0.0)
    w = synth.pruned_weights(s, 1)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s), dense_math=1)
    plan.set_option("dense_math", 0)
    for v in (2, -1):
        with pytest.raises(pkg.EscoinError) as e:
            plan.set_option("dense_math", v)
        assert "failed (-1)" in str(e.value) and "dense_math must be" in str(e.value)        # ESCOIN_EINVAL, by name
    plan.set_option("dense_math", 1)
    plan.weight_align_cpu(w)                                    # CPU mode ignores it
    plan.set_option("dense_math", 0)                            # ... and an aligned plan takes it
    plan.set_option("dense_math", 1)
    assert plan.stat("dense_math") == 0 and plan.stat("dense_variant") == 0             # nothing has run
    with pytest.raises(pkg.EscoinError, match="dense_math = 1 .*double"):          # a double align of a plan that asks for bf16
        plan.weight_align_cpu(w.astype(np.float64))
    plan.close()
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
    plan.weight_align_cpu(w.astype(np.float64))
    plan.set_option("dense_math", 0)
    with pytest.raises(pkg.EscoinError, match="dense_math = 1 .*double"):          # ... and bf16 asked of a double plan
        plan.set_option("dense_math", 1)
    plan.close()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    out = str(tmp_path_factory.mktemp("db16") / "dense_bf16_rule_check")
    srcs = [os.path.join(ROOT, "tests", "cpp", "dense_bf16_rule_check.cpp")] + [
        os.path.join(csrc, f) for f in ("align_rules.cpp", "csr_tables.cpp", "stream_builder.cpp", "jit_codegen.cpp")]
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-o", out] + srcs + ["-lpthread"])
    return out


def _rule(exe, s, f64=False, n_images=None, n_cu=256):
    words = list(s[1:15]) + [int(f64), s.N if n_images is None else n_images, s.group, n_cu]
    return [int(v) for v in subprocess.check_output([exe] + [str(v) for v in words], timeout=60).decode().split()[1:]]


@pytest.mark.parametrize("c", bc.CASES, ids=bc.IDS)
def test_rule_gives_every_case_its_tiles(exe, synth, c):
    s = synth.shape(c.name, *c.dims, **c.kw)
    kdim, ksteps, bm, n_pt, n_mt, tiles = bc.PLANS[c.name]
    assert kdim == s.C // s.group * s.KH * s.KW
    assert _rule(exe, s, n_images=c.n_images) == [0, bm, n_pt, n_mt, ksteps, tiles, tiles]
    assert _rule(exe, s, n_images=c.n_images, n_cu=1)[-2:] == [tiles, min(tiles, 2)]    # two persistent workgroups per CU
    assert _rule(exe, s, f64=True)[0] == -4                                             # ESCOIN_ESTATE: float plans only


def test_numpy_rounding_is_torch_bfloat16s():
    torch = pytest.importorskip("torch")
    bits = np.array([0x3F800000, 0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001,       # exact; ties to even, to odd + 1; either side
                     0x3FFF8000, 0x3FFFFFFF, 0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF,   # carries; the largest finite; past it
                     0x00000000, 0x80000000, 0x00008000, 0x00018000, 0x807FFFFF, 0xBF808000, 0xFF7F8000], np.uint32)
    rs = np.random.RandomState(5)
    a = np.concatenate([bits.view(np.float32), rs.standard_normal(4096).astype(np.float32) * np.ldexp(1.0, rs.randint(-40, 40, 4096)).astype(np.float32)])
    want = torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy()
    got = bc.bf16_rne(a)
    assert (got.view(np.uint32) == want.view(np.uint32)).all(), a[got.view(np.uint32) != want.view(np.uint32)][:4]
    assert np.isinf(got[9]) and np.isinf(got[10]) and got[8] == np.float32(3.3895314e38) and got[17] == -np.inf
