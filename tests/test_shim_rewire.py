"""Layer<Dtype>::Rewire through the C++ shim (tests/cpp/shim_rewire_selftest.cpp): after two training steps a third of
the entries are dropped by magnitude and as many grown where a dense score is largest; the dropped positions of blobs_[0]
are +0 in data and diff, the grown positions hold the initial values, the weights' histories travel through the entry map
into zeros (not cleared), a SolverUpdate afterwards equals the same on a layer rebuilt from the blob with hand-re-indexed
histories, and a WeightAlign from the blob reproduces the rewired pattern -- all bit for bit."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "caffe-escoin_amd", "caffe_shim", "shim_rewire_selftest")
CASES = ("Simple3x3", "Pointwise", "Group3")
RULES = ("sgd", "adam")


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
        for rule in RULES:
            for dtype in ("float", "double"):
                lines = [l for l in text.splitlines() if l.split()[:4] == [dtype, brew, case, rule]]
                assert len(lines) == 1 and lines[0].rstrip().endswith("OK"), (dtype, brew, case, rule)
                assert "differing 0" in lines[0] and "realign-differing 0" in lines[0]
                assert "live-history 0 " not in lines[0] and "grown 0 " not in lines[0]


def test_shim_rewire_cpu_mode():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")     # CPU mode must not need a device
    _assert_cases(_run(["--cpu-only"], env), "CPU")


@pytest.mark.gpu
def test_shim_rewire_gpu_mode():
    text = _run([])
    for brew in ("CPU", "GPU"):
        _assert_cases(text, brew)
