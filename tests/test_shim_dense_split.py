"""Caffe::set_dense_split through the C++ shim on the GPU: tests/cpp/shim_dense_split_selftest.cpp runs one dense
ConvolutionLayer through Forward_gpu with the option on and off and reads whether the dense launch ran the split kernel."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "caffe-escoin_amd", "caffe_shim", "shim_dense_split_selftest")


@pytest.mark.gpu
def test_shim_layer_with_and_without_dense_split():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "caffe-escoin_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "caffe-escoin_amd", "caffe_shim")], stdout=subprocess.DEVNULL)
    out = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300).stdout.decode()
    assert "dense_split ran 1 / 0" in out and "all OK" in out, out
