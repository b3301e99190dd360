"""Plan option "dense_split" without a GPU: its values and refusals, and align_rules.h db3_plan (through
tests/cpp/dense_split_rule_check.cpp, plain g++) on the cases of dense_bf16_common.py."""
import os
import subprocess

import numpy as np
import pytest

import dense_bf16_common as bc
from test_dense_bf16_host import ROOT, _rule


def test_option_values_and_refusals(pkg, synth):
    s = synth.shape("db3_opt", 2, 8, 6, 6, 8, 3, pad=1, sparsity=0.0)
    w = synth.pruned_weights(s, 1)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s), dense_split=1)
    plan.set_option("dense_split", 0)
    for v in (2, -1):
        with pytest.raises(pkg.EscoinError) as e:
            plan.set_option("dense_split", v)
        assert "failed (-1)" in str(e.value) and "dense_split must be 0 or 1" in str(e.value)   # ESCOIN_EINVAL, by name
    plan.set_option("dense_split", 1)
    plan.weight_align_cpu(w)                                    # CPU mode ignores it
    plan.set_option("dense_split", 0)                           # ... and an aligned plan takes it
    plan.set_option("dense_split", 1)
    assert plan.stat("dense_split") == 0 and plan.stat("dense_variant") == 0            # nothing has run
    with pytest.raises(pkg.EscoinError, match="dense_split = 1 .*double"):         # a double align of a plan that asks for it
        plan.weight_align_cpu(w.astype(np.float64))
    plan.close()
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
    plan.weight_align_cpu(w.astype(np.float64))
    plan.set_option("dense_split", 0)
    with pytest.raises(pkg.EscoinError, match="dense_split = 1 .*double"):         # ... and asked of a double plan
        plan.set_option("dense_split", 1)
    plan.close()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    out = str(tmp_path_factory.mktemp("db3") / "dense_split_rule_check")
    srcs = [os.path.join(ROOT, "tests", "cpp", "dense_split_rule_check.cpp")] + [
        os.path.join(csrc, f) for f in ("align_rules.cpp", "csr_tables.cpp", "stream_builder.cpp", "jit_codegen.cpp")]
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-o", out] + srcs + ["-lpthread"])
    return out


@pytest.mark.parametrize("c", bc.CASES, ids=bc.IDS)
def test_rule_gives_every_case_the_bf16_tiles_in_steps_of_32(exe, synth, c):
    s = synth.shape(c.name, *c.dims, **c.kw)
    kdim, _, bm, n_pt, n_mt, tiles = bc.PLANS[c.name]
    assert _rule(exe, s, n_images=c.n_images) == [0, bm, n_pt, n_mt, -(-kdim // 32), tiles, tiles]
    assert _rule(exe, s, f64=True)[0] == -4                                             # ESCOIN_ESTATE: float plans only
