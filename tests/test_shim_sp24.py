"""Caffe::set_sp24 through the C++ shim on the GPU: tests/cpp/shim_sp24_selftest.cpp runs one ConvolutionLayer with 2:4 weights
through Forward_gpu with the option on and off and reads whether the dense launch ran the 2:4 kernel."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "caffe-escoin_amd", "caffe_shim", "shim_sp24_selftest")


@pytest.mark.gpu
def test_shim_layer_with_and_without_sp24():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "caffe-escoin_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "caffe-escoin_amd", "caffe_shim")], stdout=subprocess.DEVNULL)
    out = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert out.returncode == 0 and "sp24 ran 1 / 0" in out.stdout.decode() and "all OK" in out.stdout.decode(), out.stdout.decode()
