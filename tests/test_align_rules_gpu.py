"""The device path and the host-only rules agree on the card at hand: every branch case of tests/golden/align_cases.json
is aligned on the GPU, and its tiling_info, kernel_choice and small_launch_rule are what tests/cpp/align_rules_check.cpp
(the rules alone, compiled without ROCm) prints for this device's CU count -- whatever that count is."""
import pytest

from test_align_rules import build_host_rules, fingerprint_tool, host_rules

pytestmark = pytest.mark.gpu


def test_device_alignment_follows_the_host_rules(tmp_path, pkg, synth):
    import torch
    tool = fingerprint_tool()
    cases = tool.load_cases("branch")
    assert len(cases) >= 17
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    want = host_rules(build_host_rules(tmp_path), tmp_path, synth, cases, n_cu)
    for c, w in zip(cases, want):
        plan = pkg.Plan(pkg.ConvDesc.from_shape(tool.case_shape(synth, c)), **tool.case_options(c))
        plan.weight_align(tool.case_weights(synth, c))
        got = {"tiling_info": plan.tiling_info, "kernel_choice": plan.stat("kernel_choice"),
               "small_launch_rule": plan.stat("small_launch_rule")}
        plan.close()
        assert got == {k: w[k] for k in got}, c["name"]
