"""ConvolutionLayer::Backward through the C++ shim: tests/cpp/shim_backward_selftest.cpp, a compact port of the
reference's GradientChecker over its 2-D gradient cases (test_convolution_layer.cpp:709-812), float and double, all
weights kept and about half pruned."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "caffe-escoin_amd", "caffe_shim", "shim_backward_selftest")
CASES = ("TestGradient", "TestDilatedGradient", "Test1x1Gradient", "TestGradientGroup")


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
            for kind in ("dense", "pruned"):
                assert any(l.startswith(dtype + " " + brew + " " + case + " ") and " %s " % kind in l and
                           l.rstrip().endswith("OK") for l in text.splitlines()), (dtype, brew, case, kind)


def test_shim_backward_gradient_check_cpu_mode():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")     # CPU mode must not need a device
    _assert_cases(_run(["--cpu-only"], env), "CPU")


@pytest.mark.gpu
def test_shim_backward_gradient_check_gpu_mode():
    text = _run([])
    _assert_cases(text, "CPU")
    _assert_cases(text, "GPU")
