"""Caffe::set_wgrad_pointwise through the C++ shim on the GPU: tests/cpp/shim_wgrad_pointwise_selftest.cpp runs one pointwise
ConvolutionLayer and one InnerProductLayer (Caffe::set_b2s) through Backward_gpu with the option on and off, each against
the same layer's CPU-mode Backward within the shim selftests' 1e-4, and reads which weight-gradient kernel ran."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "caffe-escoin_amd", "caffe_shim", "shim_wgrad_pointwise_selftest")


@pytest.mark.gpu
def test_shim_layers_with_and_without_wgrad_pointwise():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "caffe-escoin_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "caffe-escoin_amd", "caffe_shim")], stdout=subprocess.DEVNULL)
    out = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode()
    print(text)
    assert out.returncode == 0 and "all OK" in text, text
    lines = text.splitlines()
    for layer in ("Convolution", "InnerProduct"):
        assert any(l.startswith("float GPU %s wgrad_pointwise 1 ran 4:" % layer) and l.rstrip().endswith("OK") for l in lines)
        assert any(l.startswith("float GPU %s wgrad_pointwise 0 ran " % layer) and l.rstrip().endswith("OK") for l in lines)
