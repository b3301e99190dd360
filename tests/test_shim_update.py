"""Layer<Dtype>::WeightUpdate through the C++ shim (tests/cpp/shim_update_selftest.cpp): three solver steps (plain SGD on
the masked diff) with WeightUpdate() against the same steps with WeightAlign() -- identical tops after every step,
identical weights at the end, pruned weights still exactly 0."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "caffe-escoin_amd", "caffe_shim", "shim_update_selftest")
CASES = ("Simple3x3", "Strided", "Dilated", "Pointwise", "Group3")


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
        for dtype in ("float", "double"):
            lines = [l for l in text.splitlines() if l.startswith(dtype + " " + brew + " " + case + " ")]
            assert len(lines) == 1 and lines[0].rstrip().endswith("OK"), (dtype, brew, case)
            assert "differing 0" in lines[0] and "pruned-revived 0" in lines[0] and "kept 0 " not in lines[0]


def test_shim_weight_update_cpu_mode():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")     # CPU mode must not need a device
    _assert_cases(_run(["--cpu-only"], env), "CPU")


@pytest.mark.gpu
def test_shim_weight_update_gpu_mode():
    text = _run([])
    for brew in ("CPU", "GPU", "MIXED"):
        _assert_cases(text, brew)
