"""tools/fuzz_backward.py without a GPU: seeded random geometries through backward_cpu (float and double, dense and compact,
accumulation, partial batches) against torch float64 autograd, and the condition that makes the device slice's tolerance
honest: an independent float32 evaluation of the same cases stays within a quarter of it."""
import os
import sys

import numpy as np
import pytest

from conftest import rel_err

torch = pytest.importorskip("torch")

from wgrad_common import torch_backward  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_backward  # noqa: E402

SEEDS = [20261019, 11, 777]       # shared with test_backward_fuzz_gpu.py
CASES = 60


@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_slice_of_the_backward_fuzzer_in_cpu_mode(pkg, seed):
    with open(os.devnull, "w") as sink:
        worst = {}
        ran, lines, by_name = fuzz_backward.fuzz(CASES, seed, out=sink, device=False, worst=worst)
    assert not lines, "\n".join(lines[:10])
    assert ran == 6 * CASES and by_name["partial calls"] >= 5 and by_name["accumulation cases"] >= 10
    # some cases ran on skewed inputs, every element of every gradient within its derived bound (tests/errbound.py)
    print("worst err / bound:", sorted(worst.items()))
    assert by_name[fuzz_backward.SKEWED] >= CASES // 12 and max(worst.values()) <= 1.0, (by_name, worst)


def _float32_autograd(x, w, b, s, td):
    F = torch.nn.functional
    X = torch.tensor(x, requires_grad=True)
    Wt = torch.tensor(w, requires_grad=True)
    B = torch.tensor(b, requires_grad=True) if b is not None else None
    F.conv2d(X, Wt, B, stride=(s.stride_h, s.stride_w), padding=(s.pad_h, s.pad_w), dilation=(s.dil_h, s.dil_w),
             groups=s.group).backward(torch.tensor(td))
    return X.grad.numpy(), Wt.grad.numpy() * (w != 0), B.grad.numpy() if B is not None else None


def test_an_independent_float32_evaluation_stays_within_a_quarter_of_the_tolerance(synth):
    """torch float32 autograd (another summation order than any kernel of this library) against the float64 reference on
    every case of every seed the suite uses: at most TOL / 4, so a kernel that misses TOL is wrong and not merely
    rounding otherwise.  Largest value observed: 3.3e-6 (profiles/backward_fuzz.md)."""
    worst = 0.0
    for seed in SEEDS:
        for c in fuzz_backward.generate(CASES, seed, synth):
            w, x, b, td = fuzz_backward.inputs(synth, c._replace(f64=False))
            want = torch_backward(x, w, b, c.s, td)
            got = _float32_autograd(x, w, b, c.s, td)
            for g, r in zip(got, want):
                if g is not None:
                    worst = max(worst, rel_err(g, r))
    print("float32 autograd against float64: worst rel err %.3g" % worst)
    assert worst <= fuzz_backward.TOL / 4


def test_the_generator_is_seeded_and_reaches_every_class_of_case(synth):
    a, b = fuzz_backward.generate(CASES, SEEDS[0], synth), fuzz_backward.generate(CASES, SEEDS[0], synth)
    assert a == b and a != fuzz_backward.generate(CASES, SEEDS[1], synth)
    for seed in SEEDS:
        cs = fuzz_backward.generate(CASES, seed, synth)
        e = fuzz_backward.expected_runs(synth, cs)
        assert e["transposed"] >= CASES and e["gather"] >= CASES and e["jit"] >= CASES // 4, e
        assert sum(c.relu and c.n_part > 0 and fuzz_backward.transposable(c) for c in cs) >= 1, seed
        assert sum(c.window > 0 for c in cs) >= 5 and sum(c.update for c in cs) >= 5 and sum(c.mlb > 0 for c in cs) >= 2
        assert sum(not fuzz_backward.geometry_transposable(c.s) and c.s.stride_h == 1 == c.s.stride_w for c in cs) >= 1
