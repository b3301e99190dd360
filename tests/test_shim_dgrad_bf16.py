"""Caffe::set_dgrad_math through the C++ shim on the GPU: tests/cpp/shim_dgrad_bf16_selftest.cpp runs one strided
ConvolutionLayer through Backward_gpu under the MFMA data-gradient kernel with the option on and off, reads which math the
launch ran and holds the bottom diff to the bound of the operands it multiplied."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "caffe-escoin_amd", "caffe_shim", "shim_dgrad_bf16_selftest")


@pytest.mark.gpu
def test_shim_layer_with_and_without_dgrad_math_bf16():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "caffe-escoin_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "caffe-escoin_amd", "caffe_shim")], stdout=subprocess.DEVNULL)
    out = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert out.returncode == 0 and "dgrad_math ran 1 / 0" in out.stdout.decode() and "all OK" in out.stdout.decode(), out.stdout.decode()
