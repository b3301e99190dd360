"""Plan option "sp24" without a GPU: its values and refusals, synth.pattern_2of4, and align_rules.h sp24_plan and csr_tables.h
sp24_index (through tests/cpp/sp24_rule_check.cpp, plain g++) against a few lines of numpy."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_values_and_refusals(pkg, synth):
    s = synth.shape("sp_opt", 2, 8, 6, 6, 8, 3, pad=1, sparsity=0.0)
    w = synth.pattern_2of4(synth.pruned_weights(s, 1))
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s), sp24=1)
    plan.set_option("sp24", 0)
    for v in (2, -1):
        with pytest.raises(pkg.EscoinError) as e:
            plan.set_option("sp24", v)
        assert "failed (-1)" in str(e.value) and "sp24 must be 0 or 1" in str(e.value)       # ESCOIN_EINVAL, by name
    plan.weight_align_cpu(w)                                    # aligned without it ...
    with pytest.raises(pkg.EscoinError) as e:
        plan.set_option("sp24", 1)
    assert "failed (-4)" in str(e.value) and "sp24" in str(e.value) and "before weight_align" in str(e.value)      # ESCOIN_ESTATE
    plan.close()
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s), sp24=1)
    x = synth.activations(s, 2)
    plain = pkg.Plan(pkg.ConvDesc.from_shape(s))
    plain.weight_align_cpu(w)
    plan.weight_align_cpu(w)                                    # CPU mode ignores it
    assert np.array_equal(plan.forward_cpu(x), plain.forward_cpu(x))
    plan.set_option("sp24", 0)                                  # off and on again after an align that had it
    plan.set_option("sp24", 1)
    assert (plan.stat("sp24_pattern"), plan.stat("dense_sp24")) == (0, 0)                   # no device table, nothing has run
    with pytest.raises(pkg.EscoinError, match="sp24 = 1 .*double"):          # a double align of a plan that asks for it
        plan.weight_align_cpu(w.astype(np.float64))
    plan.close()
    plain.weight_align_cpu(w.astype(np.float64))
    with pytest.raises(pkg.EscoinError, match="sp24 = 1 .*double"):          # ... and asked of a double plan
        plain.set_option("sp24", 1)
    plain.close()


@pytest.mark.parametrize("k", [72, 27, 2])
def test_pattern_2of4_keeps_the_two_largest_of_every_group(synth, k):
    rs = np.random.RandomState(k)
    w = rs.randint(-3, 4, (5, k, 1, 1)).astype(np.float32)      # small integers: ties, and zeros among the largest
    got = synth.pattern_2of4(w).reshape(5, k)
    assert got.dtype == w.dtype and ((got == 0) | (got == w.reshape(5, k))).all()
    for r in range(5):
        for j in range(0, k, 4):
            grp, kept = w[r, j:j + 4, 0, 0], got[r, j:j + 4]
            want = np.zeros_like(grp)
            for i in sorted(range(len(grp)), key=lambda i: (-abs(grp[i]), i))[:2]:      # ties go to the lower position
                want[i] = grp[i]
            assert (kept == want).all() and np.count_nonzero(kept) <= 2, (r, j, grp, kept)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    out = str(tmp_path_factory.mktemp("sp24") / "sp24_rule_check")
    srcs = [os.path.join(ROOT, "tests", "cpp", "sp24_rule_check.cpp")] + [
        os.path.join(csrc, f) for f in ("align_rules.cpp", "csr_tables.cpp", "stream_builder.cpp", "jit_codegen.cpp")]
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-o", out] + srcs + ["-lpthread"])
    return out


def _check(exe, s, rows=None, f64=False):
    args = list(s[1:15]) + [int(f64), s.N, s.group, 256]
    for r in rows or []:
        args += [len(r)] + list(r)
    lines = subprocess.check_output([exe] + [str(v) for v in args], timeout=60).decode().splitlines()
    return [[int(v) for v in ln.split()[1:]] for ln in lines]


def _words(rows, n_rows, lda):
    """The table in numpy: per group of 4 the entries' positions, filled up with the lowest free ones, ascending."""
    idx = np.full((n_rows, lda // 16), 0x4444, np.uint16)
    for r, cols in enumerate(rows):
        for j in range(lda // 4):
            pos = [c % 4 for c in cols if c // 4 == j]
            pos = sorted(pos + [q for q in range(4) if q not in pos][:2 - len(pos)])
            idx[r, j // 4] &= np.uint16(~(0xF << 4 * (j % 4)) & 0xFFFF)
            idx[r, j // 4] |= np.uint16((pos[0] | pos[1] << 2) << 4 * (j % 4))
    return idx.reshape(-1).tolist()


def test_rule_and_index_words(exe, synth):
    # K = 27 (K % 4 != 0), lda 32: row 0 holds an empty group (4..7), 1-entry groups at positions 0, 3 and 1 (8, 15, 17), full
    # groups and the short last group 24..26; row 1 is empty; row 2 is full at the other ends
    s = synth.shape("sp_rule", 2, 3, 9, 9, 3, 3, pad=1, stride=2, sparsity=0.0)
    rows = [[0, 3, 8, 15, 17, 20, 22, 25, 26], [], [1, 2, 5, 6, 9, 10, 12, 13, 24]]
    plan, index = _check(exe, s, rows)
    assert plan == [0, 64, 1, 1, 1, 1, 1, 3 + 128, 2, (3 + 128) * 2 * 2]
    assert index[0] == 1 and index[1:] == _words(rows, 3 + 128, 32)
    assert index[1:3] == [0xC44C, 0x4984]                  # row 0 by hand: (0,3) (0,1) (0,1) (0,3) | (0,1) (0,2) (1,2) (0,1), low nibble first
    assert _check(exe, s, [[0, 1, 2], [], []])[1] == [0]                                # 3 entries in a group: no 2:4 pattern
    assert _check(exe, s, [[24, 25, 26], [], []])[1] == [0]                             # ... in the short last group too
    assert _check(exe, s, f64=True)[0][0] == -4                                         # ESCOIN_ESTATE: float plans only
    # the tile plan is the bf16 kernel's: K = 216 in four k-steps, Mg = 130 in two channel tiles of 128
    assert _check(exe, synth.shape("sp_dil", 2, 24, 13, 16, 20, 3, pad=2, dil=2))[0][:5] == [0, 64, 4, 1, 4]
    assert _check(exe, synth.shape("sp_3x3", 3, 8, 9, 11, 130, 3, pad=1))[0][:8] == [0, 128, 3, 2, 2, 6, 6, 258]
