"""tools/fuzz_backward.py on the MI355X: a seeded slice per seed -- every backward_kernel and wgrad_kernel against torch
float64 autograd, the gather kernel bit for bit against the CPU mode, accumulation, partial batches, blobs as windows off
a 16-byte boundary, in-place updates, determinism -- with coverage floors computed from the generator and the geometry
predicates (profiles/backward_fuzz.md has the seconds per seed and a longer sweep)."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_backward  # noqa: E402

pytestmark = pytest.mark.gpu
SEEDS = [20261019, 11, 777]       # shared with test_backward_fuzz_cpu.py
CASES = 60


_STOPPED = []       # the line of a run that ended on something other than a refusal: no later seed touches the device


@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_slice_of_the_backward_fuzzer(pkg, synth, seed):
    if _STOPPED:
        pytest.fail("not started: an earlier seed " + _STOPPED[0])
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        pytest.fail("no HIP device visible (these tests run on the MI355X)")
    with open(os.devnull, "w") as sink:
        worst = {}
        ran, lines, by_name = fuzz_backward.fuzz(CASES, seed, out=sink, worst=worst)
    print(ran, sorted(by_name.items()))
    print("worst err / bound per kernel:", sorted(worst.items()))
    _STOPPED.extend(ln for ln in lines if "stopped by" in ln)
    assert not lines, "\n".join(lines[:10])
    # some cases ran on skewed inputs, every element of every gradient within its derived bound (tests/errbound.py)
    assert by_name[fuzz_backward.SKEWED] >= CASES // 12 and max(worst.values()) <= 1.0, (by_name, worst)
    e = fuzz_backward.expected_runs(synth, fuzz_backward.generate(CASES, seed, synth))
    refused = by_name["staged refusals (float, stride 1: the LDS budget)"]
    assert by_name["(data gradients on the transposed plan)"] >= e["transposed"] >= CASES, (by_name, e)
    assert by_name["(data gradients on the gather kernel)"] >= e["gather"] >= CASES, (by_name, e)
    assert by_name.get("bwd_data_kernel jit", 0) >= e["jit"] >= CASES // 4, (by_name, e)
    assert by_name.get("wgrad_kernel staged", 0) >= e["staged_candidates"] - refused, (by_name, e)
    assert 5 * refused <= e["staged_candidates"], (by_name, e)
    # measured, not derived: under AUTO the stat shows a fast kernel on every case where the tiled families cover the
    # transposed descriptor (GENERIC there would be the gather kernel or a plan that fell back) ...
    assert by_name[fuzz_backward.AUTO_FAST] == e["auto_fast"] >= CASES // 6, (by_name, e)
    # ... and the forced stream kernel ran on all of them but the few whose weight stream exceeds the LDS budget
    stream_refused = by_name[fuzz_backward.STREAM_REFUSALS]
    assert by_name.get("bwd_data_kernel tiled", 0) >= e["jit"] - stream_refused and 5 * stream_refused <= e["jit"], (by_name, e)
    for name in ("partial calls", "accumulation cases", "window cases", "update cases"):
        assert by_name[name] >= 5, (name, by_name)
