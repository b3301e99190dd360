"""InnerProductLayer and Caffe::set_b2s through the C++ shim on the GPU: tests/cpp/shim_b2s_selftest.cpp runs one InnerProduct
layer's Forward, Backward, SolverUpdate, Prune and Forward again with the option on (float: the inner plan runs), off, and
in double (the option does not serve it), each against a plain float64 loop within the derived bound.  The CPU-mode runs
and the transpose = true abort are in test_b2s_host.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "caffe-escoin_amd", "caffe_shim", "shim_b2s_selftest")


@pytest.mark.gpu
def test_shim_inner_product_layer_with_and_without_b2s():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "caffe-escoin_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "caffe-escoin_amd", "caffe_shim")], stdout=subprocess.DEVNULL)
    out = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode()
    print(text)
    assert out.returncode == 0 and "all OK" in text, text
    lines = text.splitlines()
    assert any(l.startswith("float GPU b2s 1 ran 1 (update_fast 1)") and l.rstrip().endswith("OK") for l in lines)
    assert any(l.startswith("float GPU b2s 0 ran 0 (update_fast 1)") and l.rstrip().endswith("OK") for l in lines)
    assert any(l.startswith("double GPU b2s 1 ran 0") and l.rstrip().endswith("OK") for l in lines)
