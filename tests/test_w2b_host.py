"""Plan option "w2b" without a GPU: the option's values and refusals; align_rules.h w2b_plan through
tests/cpp/w2b_plan_check.cpp, compiled with plain g++ and no ROCm include path (that compile is the proof that the rule is
host-only), against the numpy restatement of w2b_common.py on the shapes and on the layers the option does not serve; and, with
the strips the compiled rule gives, pack -> convolution of N * S strip images -> unpack / unpack_sum against the convolution
itself, exactly, on integer-valued inputs."""
import os
import subprocess

import numpy as np
import pytest

from w2b_common import SHAPES, make, pack, plan_row, unpack, unpack_sum

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_values_and_refusals(pkg, synth):
    s = make(synth, "k5p2_g2")
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s), s2d=1, s2b=1)               # may be set together
    for key, good, bad in (("w2b", (0, 1), (2, -1)), ("w2b_strip", (0, 4, 8, 252), (-4, 2, 6, 10, 256, 260))):
        for v in good + bad:                                                # (5x5: a multiple of 4 with 4 <= SW and SW + 4 <= 256)
            if v in good:
                plan.set_option(key, v)
                continue
            with pytest.raises(pkg.EscoinError) as e:
                plan.set_option(key, v)
            assert "failed (-1)" in str(e.value) and key in str(e.value)    # ESCOIN_EINVAL
    plan.weight_align_cpu(synth.pruned_weights(s, 11))
    for key in ("w2b", "w2b_strip"):
        with pytest.raises(pkg.EscoinError) as e:
            plan.set_option(key, 0)                                         # after the align
        assert "failed (-4)" in str(e.value) and "before" in str(e.value)   # ESCOIN_ESTATE
    assert [plan.stat(k) for k in ("w2b", "w2b_strips", "w2b_strip", "w2b_scratch_bytes")] == [0] * 4     # no device align: not active
    plan.close()
    names = ["escoin_plan_w2b_pack", "escoin_plan_w2b_unpack", "escoin_plan_w2b_unpack_sum"]
    assert all(n in pkg.API_SYMBOLS and hasattr(pkg.lib(), n) and hasattr(pkg.Plan, n[12:]) for n in names)


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    """w2b_plan's answers for (shape, strip, is_f64) cases: g++, -Icsrc -Iinclude, nothing of ROCm."""
    tmp = tmp_path_factory.mktemp("w2b")
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "cpp", "w2b_plan_check.cpp")] + [
        os.path.join(csrc, f) for f in ("align_rules.cpp", "csr_tables.cpp", "stream_builder.cpp", "jit_codegen.cpp")]
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-Wall", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-o", str(tmp / "check")] +
                          srcs + ["-lpthread"])

    def run(cases):
        fields = "N C H W M KH KW pad_h pad_w stride_h stride_w dil_h dil_w group".split()
        text = "".join(" ".join(str(int(v)) for v in [getattr(s, f) for f in fields] + [bool(s.bias), 1, f64, strip]) + "\n" for s, strip, f64 in cases)
        (tmp / "cases.txt").write_text(text)
        out = subprocess.check_output([str(tmp / "check"), str(tmp / "cases.txt")], timeout=60).decode()
        return [[int(v) for v in line.split()] for line in out.splitlines()]
    return run


def test_the_rule_equals_its_restatement(synth, rule):
    sh = synth.shape
    cases = [(make(synth, n), SHAPES[n][10], 0, 1) for n in SHAPES] + [
        (make(synth, "k3p1"), 0, 0, 0),                                                     # a narrow row without the test option
        (make(synth, "real", stride=2), 0, 0, 0), (make(synth, "real", dil=2, pad=2), 0, 0, 0), (make(synth, "real"), 0, 1, 0),   # ... double
        (sh("fcn", 8, 64, 250, 500, 128, 3, pad=1), 0, 0, 1), (sh("w257_p0", 1, 1, 3, 257, 1, 3), 0, 0, 1),
        (sh("ow508", 1, 1, 3, 508, 1, 3, pad=1), 0, 0, 1),                                  # ceil(508 / 2) = 254 would round to 256
        (sh("k7", 1, 1, 1, 600, 1, 1, KW=7, pad=0, pad_w=3), 0, 0, 1),
        (sh("images_fit", 21845, 1, 1, 600, 1, 1), 0, 0, 1), (sh("images_over", 21846, 1, 1, 600, 1, 1), 0, 0, 0),   # N * 3 at 65535
        (sh("blob_fits", 1, 1, 1 << 20, 2016, 1, 1), 0, 0, 1), (sh("blob_2_31", 1, 1, 1 << 20, 2048, 1, 1), 0, 0, 0),
        (sh("strips_2_31", 1, 1, 1 << 19, 4094, 1, 1, KW=3), 0, 0, 0),                      # X' and T' alone: 17 strips of 244 + 2
    ]
    rows = rule([c[:3] for c in cases])
    assert len(rows) == len(cases)
    for (s, strip, f64, served), row in zip(cases, rows):
        assert row == plan_row(synth, s, strip, bool(f64)) and row[0] == served, (s.name, row)
    assert rows[6][1:4] == [2, 152, 154] and rows[0][1:4] == [3, 8, 10] and rows[13][1:4] == [3, 172, 174]


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_pack_convolution_of_the_strips_unpack_is_the_convolution_exactly(synth, rule, name, relu):
    """Integer-valued inputs, so every order of summation is exact in float64."""
    s = make(synth, name)
    S, SW, Wi = rule([(s, SHAPES[name][10], 0)])[0][1:4]
    oh, ow = synth.out_hw(s)
    rs = np.random.RandomState(31)
    w = synth.pruned_weights(s, 31)
    w = torch.from_numpy(np.where(w != 0, rs.randint(1, 4, w.shape) * rs.choice([-1, 1], w.shape), 0).astype(np.float64))
    x = rs.randint(-3, 4, (s.N, s.C, s.H, s.W)).astype(np.float64)
    b = torch.from_numpy(rs.randint(-5, 6, (s.M,)).astype(np.float64))
    td = rs.randint(-3, 4, (s.N, s.M, oh, ow)).astype(np.float64)
    kw, kwi = dict(padding=(s.pad_h, s.pad_w), groups=s.group), dict(padding=(s.pad_h, 0), groups=s.group)
    lin = torch.nn.functional.conv2d(torch.from_numpy(x), w, b, **kw)
    want = (lin.clamp(min=0) if relu else lin).numpy()
    xi = pack(x, S, SW, Wi, s.pad_w)
    top = unpack(torch.nn.functional.conv2d(torch.from_numpy(xi), w, b, **kwi).numpy(), S, SW, ow, relu=relu)
    assert xi.shape == (s.N * S, s.C, s.H, Wi) and np.array_equal(top, want)
    g = np.where(want > 0, td, 0.0) if relu else td
    gi = pack(td, S, SW, SW, 0, mask=top if relu else None)
    assert np.array_equal(unpack(gi, S, SW, ow), g) and not gi.reshape(s.N, S, -1, SW)[:, -1, :, ow - (S - 1) * SW:].any()
    dxi = torch.nn.grad.conv2d_input(xi.shape, w, torch.from_numpy(gi), **kwi).numpy()
    dx = torch.nn.grad.conv2d_input(x.shape, w, torch.from_numpy(g), **kw).numpy()
    assert np.array_equal(unpack_sum(dxi, S, SW, s.W, s.pad_w), dx) and np.abs(dx).max() > 0
