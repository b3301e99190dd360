"""Caffe::set_w2b through the C++ shim: tests/cpp/shim_w2b_selftest.cpp runs one 300-wide ConvolutionLayer<float> Forward_gpu
and Backward_gpu with the option on and off on integer data: the same bits, and stat "w2b" says which ran."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_shim_w2b_layer_against_the_same_layer_without_it():
    shim = os.path.join(ROOT, "caffe-escoin_amd", "caffe_shim")
    if not os.path.exists(os.path.join(shim, "shim_w2b_selftest")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "caffe-escoin_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
        subprocess.check_call(["make", "-C", shim], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(shim, "shim_w2b_selftest")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode()
    assert out.returncode == 0 and "all OK" in text and "float GPU w2b on ran 1 (2 strips), off ran 0" in text, text
