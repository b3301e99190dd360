"""ConvolutionLayer<Dtype>::DenseWeightDiff through the C++ shim (tests/cpp/shim_dense_wgrad_selftest.cpp): the dense
weight gradient of a Convolution / ConvolutionReLU layer at every position of blobs_[0] against a double-precision loop
nest and its per-element bound, its agreement with Backward's masked gradient inside the pattern, the untouched blobs_[0],
the blob as Rewire's score (the grown positions are the rule's) and identical bits after the Rewire."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "caffe-escoin_amd", "caffe_shim", "shim_dense_wgrad_selftest")
CASES = ("Simple3x3", "Pointwise", "Group3", "Wide70", "ReLU3x3")


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
            lines = [l for l in text.splitlines() if l.split()[:3] == [dtype, brew, case]]
            assert len(lines) == 1 and lines[0].rstrip().endswith("OK"), (dtype, brew, case)
            assert "differing 0" in lines[0] and "grown-wrong 0" in lines[0]
            assert "outside-nonzero 0 " not in lines[0]
            # the matrix-core kernel ran exactly where it exists: the float GPU brew (the double GPU brew falls back)
            device = brew == "GPU" and dtype == "float"
            assert ("device-calls 2" if device else "device-calls 0") in lines[0]


def test_shim_dense_wgrad_cpu_mode():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")     # CPU mode must not need a device
    _assert_cases(_run(["--cpu-only"], env), "CPU")


@pytest.mark.gpu
def test_shim_dense_wgrad_gpu_mode():
    text = _run([])
    for brew in ("CPU", "GPU"):
        _assert_cases(text, brew)
