"""Caffe::set_backward_kernel through the C++ shim: tests/cpp/shim_dgrad_selftest.cpp runs one strided
ConvolutionLayer<float> Backward under the MFMA data-gradient kernel and one under the default, checks both bottom diffs
against a float64 restatement within the derived bound and reads each plan's stat "bwd_data_kernel"; in CPU mode the
setter is accepted and ignored."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "caffe-escoin_amd", "caffe_shim", "shim_dgrad_selftest")


def _run(args, env=None):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "caffe-escoin_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "caffe-escoin_amd", "caffe_shim")], stdout=subprocess.DEVNULL)
    out = subprocess.run([EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, env=env)
    text = out.stdout.decode()
    print(text)
    assert out.returncode == 0, text
    assert "all OK" in text
    return text


def test_shim_backward_kernel_setter_is_ignored_in_cpu_mode():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")     # CPU mode must not need a device
    text = _run(["--cpu-only"], env)
    assert any(l.startswith("float CPU setter ignored") and l.rstrip().endswith("OK") for l in text.splitlines())


@pytest.mark.gpu
def test_shim_dgrad_mfma_against_the_default_kernel():
    text = _run([])
    assert any(l.startswith("float GPU backward_kernel mfma ran 5, default ran 1") and l.rstrip().endswith("OK")
               for l in text.splitlines())
