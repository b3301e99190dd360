"""The code-touch election on the device (csrc/align_rules.h touch_election, plan option "code_touchers") -- needs an
MI355X.

The election changes which workgroups ask for 64 lines per code touch and which for one; it changes no instruction of
the generated code and nothing a result depends on.  So the outputs at stride 1 (every workgroup touches: the behaviour
before the election), stride 2 and the rule must be EQUAL bit for bit, under both compiled bodies and both code
loaders, the stats must name the stride of the last launch, and the persisted aligned form must not depend on the
option (tests/golden/touch_election_exports.json: SHA-256 of escoin_plan_export_aligned, recorded on an MI355X by
tests/golden/make_touch_election_golden.py)."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "touch_election_exports.json")
TOL = 1e-4      # test_gpu_parity.py's tolerance for generated code against the CPU oracle

# name -> (N, C, H, W, M, K, pad, sparsity)
LAYERS = {
    "k3_8x8": (3, 16, 8, 8, 16, 3, 1, 0.9),            # 3x3 / pad 1, C = M = 16
    "k3_columns": (9, 32, 7, 7, 136, 3, 1, 0.9),       # 3x3, M = 136: several workgroup columns (six on 256 CUs), generic body
    "pw_14x14": (5, 64, 14, 14, 64, 1, 0, 0.95),       # pointwise
    # 48 tiles in each of two grid rows on 256 CUs: six workgroups per XCD and row, so strides above 1 leave workgroups
    # that touch one line (the three layers above run so few workgroups that every one is rank 0 of its set)
    "k3_many_tiles": (96, 24, 14, 14, 64, 3, 1, 0.9),
}
STRIDES = (1, 2, 0)       # 0: the rule
RULE_STRIDE = 8           # csrc/align_rules.h kTouchRuleStride: the rule's answer on a device of eight XCDs
WEIGHTS_SEED = 5100


@pytest.fixture(scope="module")
def torch_cuda(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert pkg.device_count() >= 1
    return torch


def shape_of(synth, name):
    N, C, H, W, M, K, pad, sp = LAYERS[name]
    return synth.shape(name, N, C, H, W, M, K, pad=pad, sparsity=sp, bias=True)


def aligned_plan(pkg, synth, name, **options):
    s = shape_of(synth, name)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=True), kernel=pkg.KERNEL_JIT, tiling_batch=256, **options)
    plan.weight_align(synth.pruned_weights(s, WEIGHTS_SEED))
    return plan


_REFS = {}


def _reference(oracle, synth, name):
    """(x, bias, the oracle's output) of a layer, computed once."""
    if name not in _REFS:
        s = shape_of(synth, name)
        w, b, x = synth.pruned_weights(s, WEIGHTS_SEED), synth.bias_vector(s, WEIGHTS_SEED + 1), synth.activations(s, WEIGHTS_SEED + 2)
        g = oracle.geom(s.C, s.H, s.W, s.M, s.KH, s.KW, s.pad_h, s.pad_w, 1, 1, 1, 1, 1)
        _REFS[name] = (x, b, oracle.conv_forward(g, x, w, b, relu=True, gate=False, threads=4))
    return _REFS[name]


@pytest.mark.parametrize("options", [dict(), dict(body_variant=0), dict(code_loader=1)], ids=["auto_body", "generic_body", "code_loader"])
@pytest.mark.parametrize("name", list(LAYERS))
def test_outputs_are_bit_equal_at_every_stride(pkg, oracle, synth, torch_cuda, name, options):
    torch = torch_cuda
    dev = torch.device("cuda:0")
    x, b, want = _reference(oracle, synth, name)
    xd, bd = torch.from_numpy(x).to(dev), torch.from_numpy(b).to(dev)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    outs, lines, infos, bodies = [], [], set(), set()
    for stride in STRIDES:
        plan = aligned_plan(pkg, synth, name, code_touchers=stride, **options)
        assert "jit" in plan.kernel_name and plan.stat("code_bytes") > 0
        assert plan.stat("code_direct") == (0 if options.get("code_loader") else 1)
        infos.add(plan.tiling_info)
        got = plan.forward(xd, bd)
        torch.cuda.synchronize()
        # the stats describe the launch that just ran
        t = plan.stat("code_touchers")
        if name == "pw_14x14":
            # its code carries no touches (and the chained pointwise body does not elect): stride 1 whatever is asked
            assert t == 1, (name, stride, t)
        elif stride >= 1:
            assert t == stride, (name, stride, t)
        else:
            assert t == (RULE_STRIDE if n_cu >= 64 and n_cu % 8 == 0 else 1), (name, t, n_cu)      # what the rule ships
        bodies.add(plan.stat("body_variant"))
        if "body_variant" in options:
            assert plan.stat("body_variant") == 0
        if name == "k3_columns":
            assert plan.stat("workgroup_columns") > 1
        lines.append(plan.stat("touch_lines_per_launch"))
        outs.append(got)
        plan.close()
    assert len(infos) == 1 and len(bodies) == 1, (infos, bodies)       # the option reaches no layout or body decision
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), name
    err = rel_err(outs[0].cpu().numpy(), want)
    print("%s %s body %s: rel_err %.3g, touch lines per launch at strides 1 / 2 / rule: %s (%s)" % (name, options, bodies, err, lines, infos.pop()))
    assert err <= TOL, (name, err)
    # fewer touchers never ask for more lines; where a set has several workgroups, stride 2 asks for fewer
    # (the pointwise layer's code is generated without touches: 0 lines at every stride)
    assert lines[1] <= lines[0] and lines[2] <= lines[0] and (lines[0] > 0 or name == "pw_14x14"), lines
    if name == "k3_many_tiles" and n_cu == 256:
        assert lines[2] < lines[1] < lines[0], lines
        # the chained 3x3 body -- the benched layers' -- runs here with workgroups that do not touch, unless the generic one is forced
        assert bodies == {0 if "body_variant" in options else 1}, bodies


def test_the_stats_follow_the_forced_stride(pkg, synth, torch_cuda):
    """Strides beyond the issue's three on the layer whose sets have several workgroups: equal outputs, the stat names the
    stride (capped at 65535: rank 0 alone), the line count never grows with it, and a negative stride is refused."""
    torch = torch_cuda
    dev = torch.device("cuda:0")
    s = shape_of(synth, "k3_many_tiles")
    xd = torch.from_numpy(synth.activations(s, WEIGHTS_SEED + 2)).to(dev)
    bd = torch.from_numpy(synth.bias_vector(s, WEIGHTS_SEED + 1)).to(dev)
    first, seen = None, []
    for stride in (1, 3, 16, 70000):
        plan = aligned_plan(pkg, synth, "k3_many_tiles", code_touchers=stride)
        got = plan.forward(xd, bd)
        torch.cuda.synchronize()
        assert plan.stat("code_touchers") == min(stride, 65535)
        first = got if first is None else first
        assert torch.equal(got, first), stride
        seen.append(plan.stat("touch_lines_per_launch"))
        plan.close()
    assert seen[0] == max(seen) and seen[-1] == min(seen), seen
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
    with pytest.raises(pkg.EscoinError):
        plan.set_option("code_touchers", -1)
    plan.close()


def test_a_reused_code_address_runs_the_new_code_with_few_touchers(pkg, oracle, synth, torch_cuda):
    """test_gpu_parity.py's test_code_address_reuse_runs_the_new_code with the election on: a destroyed plan's address
    range comes back for the next plan's code, and most workgroups of the new plan no longer pull whole lines of it --
    what they run must still be the new code.  The rule, then one toucher per set, other weights every round."""
    torch = torch_cuda
    dev = torch.device("cuda:0")
    s = synth.shape("reuse_k3", 96, 24, 14, 14, 64, 3, pad=1, sparsity=0.9, bias=False)
    g = oracle.geom(s.C, s.H, s.W, s.M, s.KH, s.KW, s.pad_h, s.pad_w, 1, 1, 1, 1, 1)
    x = synth.activations(s, 41)
    xd = torch.from_numpy(x).to(dev)
    for it, stride in enumerate((0, 65535, 0, 65535)):
        w = synth.pruned_weights(s, 5200 + it)
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s), kernel=pkg.KERNEL_JIT, tiling_batch=256, code_touchers=stride)
        plan.weight_align(w)
        got = plan.forward(xd, None).cpu().numpy()
        assert rel_err(got, oracle.conv_forward(g, x, w, None, gate=False, threads=4)) <= TOL, (it, stride)
        plan.close()        # the next round's code takes this one's place


def test_exports_match_the_recorded_digests_at_every_stride(pkg, synth, torch_cuda):
    """The option reaches nothing the aligned form persists -- generated code, tables, tags: at the rule's and at a forced
    stride every layer exports the bytes whose digest tests/golden/touch_election_exports.json records (first recorded
    with the library of the commit before the election existed, which is how the election is known to have changed no
    generated byte).  A change that legitimately alters the code or the format regenerates the file:
    tests/golden/make_touch_election_golden.py."""
    torch = torch_cuda
    with open(GOLDEN) as f:
        golden = json.load(f)
    if torch.cuda.get_device_properties(0).multi_processor_count != golden["n_cu"]:
        pytest.skip("the golden digests are a %d-CU device's" % golden["n_cu"])
    assert sorted(golden["sha256"]) == sorted(LAYERS)
    for name in LAYERS:
        for stride in (0, 2):
            plan = aligned_plan(pkg, synth, name, code_touchers=stride)
            digest = hashlib.sha256(np.ascontiguousarray(plan.export_aligned()).tobytes()).hexdigest()
            plan.close()
            assert digest == golden["sha256"][name], (name, stride)
