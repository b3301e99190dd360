"""Layer<Dtype>::SolverUpdate through the C++ shim (tests/cpp/shim_solver_selftest.cpp): three training steps per solver
rule with the rule written on the host over the dense blobs followed by WeightUpdate() -- the path that exists without the
fused step -- against the same steps with SolverUpdate(): identical tops, blobs_[0] and blobs_[1] after every step, pruned
weights still exactly 0."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "caffe-escoin_amd", "caffe_shim", "shim_solver_selftest")
CASES = ("Simple3x3", "Strided", "Dilated", "Pointwise", "Group3")
RULES = ("sgd", "nesterov", "adam")


def _run(args, env=None):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "caffe-escoin_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "caffe-escoin_amd", "caffe_shim")], stdout=subprocess.DEVNULL)
    out = subprocess.run([EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900, env=env)
    text = out.stdout.decode()
    print(text)
    assert out.returncode == 0, text
    assert "all OK" in text
    return text


def _assert_cases(text, brew):
    for case in CASES:
        for rule in RULES:
            for dtype in ("float", "double"):
                lines = [l for l in text.splitlines() if l.split()[:4] == [dtype, brew, case, rule]]
                assert len(lines) == 1 and lines[0].rstrip().endswith("OK"), (dtype, brew, case, rule)
                assert "differing 0" in lines[0] and "pruned-revived 0" in lines[0] and "kept 0 " not in lines[0]


def test_shim_solver_update_cpu_mode():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")     # CPU mode must not need a device
    _assert_cases(_run(["--cpu-only"], env), "CPU")


@pytest.mark.gpu
def test_shim_solver_update_gpu_mode():
    text = _run([])
    for brew in ("CPU", "GPU"):
        _assert_cases(text, brew)
