"""Caffe::set_s2b through the C++ shim: tests/cpp/shim_s2b_selftest.cpp runs one dilated ConvolutionLayer<float> Forward,
Backward, SolverUpdate and Forward again with the option on and with it off, checks both tops and both bottom diffs
against a float64 restatement within the derived bound, the untouched weight / bias gradients and the solver's new blobs
bit for bit between the two, and reads each plan's stat "s2b"; in CPU mode the setter is accepted and ignored."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "caffe-escoin_amd", "caffe_shim", "shim_s2b_selftest")


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


def test_shim_s2b_setter_is_ignored_in_cpu_mode():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")     # CPU mode must not need a device
    text = _run(["--cpu-only"], env)
    assert any(l.startswith("float CPU setter ignored") and l.rstrip().endswith("OK") for l in text.splitlines())


@pytest.mark.gpu
def test_shim_s2b_layer_against_the_same_layer_without_it():
    text = _run([])
    assert any(l.startswith("float GPU s2b on ran 1 (update_fast 1), off ran 0") and l.rstrip().endswith("OK")
               for l in text.splitlines())
