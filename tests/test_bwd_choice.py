"""The backward's kernel choice without a GPU (csrc/align_rules.h bwd_choice through tests/cpp/bwd_choice_check.cpp,
compiled with plain g++ and no ROCm include path): every branch and every refusal of the ladder that stood inline in
sconv_backward.hip, against expectations written by hand from that ladder (tests/bwd_choice_common.py)."""
import pytest

from bwd_choice_common import CASES, build_checker, run_checker


@pytest.fixture(scope="module")
def decided(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bwd_choice")
    return dict(zip((c["name"] for c in CASES), run_checker(build_checker(tmp), tmp, CASES)))


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_choice_is_the_ladders(decided, name):
    case = next(c for c in CASES if c["name"] == name)
    got = decided[name]
    print(name, got)
    assert {k: got[k] for k in case["expect"]} == case["expect"]


def test_table_covers_the_ladder(decided):
    """Every data path, every weight-gradient kernel and every refusal text occurs."""
    ok = [r for r in decided.values() if r["rc"] == 0]
    assert {r["data"] for r in ok} == {"inner", "transposed", "gather", "mfma"}
    assert {r["wgrad_kernel"] for r in ok} == {1, 2, 3}
    assert len({r["error"] for r in decided.values() if r["rc"] != 0}) == 7
    assert all(r["rc"] == -1 and r["error"] for r in decided.values() if r["rc"] != 0)
