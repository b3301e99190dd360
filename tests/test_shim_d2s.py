"""DeconvolutionLayer<float> through the C++ shim on the GPU: tests/cpp/shim_d2s_selftest.cpp runs Forward_gpu and Backward_gpu
of the layers k4s2p1 and k3s2p1 through plan option "deconv", each against a plain float64 loop over the layer's definition
within the derived bound.  The CPU-mode runs and the Dtype = double abort are in test_d2s_cpu.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "caffe-escoin_amd", "caffe_shim", "shim_d2s_selftest")


@pytest.mark.gpu
def test_shim_deconvolution_layer_on_the_device():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "caffe-escoin_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "caffe-escoin_amd", "caffe_shim")], stdout=subprocess.DEVNULL)
    out = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode()
    print(text)
    assert out.returncode == 0 and "all OK" in text, text
    for name in ("k4s2p1", "k3s2p1"):
        assert any(l.startswith("GPU %s deconv ran 1" % name) and l.rstrip().endswith("OK") for l in text.splitlines()), text
