"""Plan option "depthwise" without a GPU: the options' values and refusals, and -- through tests/cpp/depthwise_rule_check.cpp,
compiled with plain g++ and no ROCm include path (the proof that the rule is host-only) -- align_rules.h dw_plan held to what
csrc/depthwise.hip relies on, by brute force over the shapes of depthwise_common.py, and bwd_choice with the option."""
import os
import subprocess

import pytest

import depthwise_common as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_GATHER, K_MFMA, K_DEPTHWISE = 2, 3, 4          # align_rules.h BwdDataPath


def test_option_values_and_refusals(pkg, synth):
    assert pkg.BWD_DEPTHWISE == dc.BWD_DEPTHWISE
    s, w = dc.case(synth, "3x3_s1")[:2]
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
    for key, v in (("depthwise", 2), ("depthwise", -1), ("depthwise_band_rows", -1)):
        with pytest.raises(pkg.EscoinError) as e:
            plan.set_option(key, v)
        assert "failed (-1)" in str(e.value) and key in str(e.value)        # ESCOIN_EINVAL
    plan.set_option("depthwise", 1)
    plan.set_option("depthwise_band_rows", 2)
    assert plan.stat("depthwise") == 0 and plan.stat("depthwise_lds_bytes") == 0      # nothing is active before a device align
    plan.weight_align_cpu(w)
    for key in ("depthwise", "depthwise_band_rows"):
        with pytest.raises(pkg.EscoinError) as e:
            plan.set_option(key, 0)
        assert "failed (-4)" in str(e.value) and "before" in str(e.value)       # ESCOIN_ESTATE
    plan.close()
    pkg.Plan(pkg.ConvDesc.from_shape(s), depthwise=1, depthwise_band_rows=1).close()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    out = str(tmp_path_factory.mktemp("dw") / "depthwise_rule_check")
    srcs = [os.path.join(ROOT, "tests", "cpp", "depthwise_rule_check.cpp")] + [os.path.join(csrc, f) for f in ("align_rules.cpp", "stream_builder.cpp", "jit_codegen.cpp")]
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-o", out] + srcs + ["-lpthread"])
    return out


def _rule(exe, s, f64=False, band_rows=0, n_cu=256):
    words = list(s[1:15]) + [int(f64), band_rows, n_cu]     # N .. group, in ConvShape's order
    out = {}
    for line in subprocess.check_output([exe] + [str(v) for v in words], timeout=60).decode().splitlines():
        out.setdefault(line.split()[0], []).append([int(v) for v in line.split()[1:]])
    return out


@pytest.mark.parametrize("band_rows", dc.BAND_ROWS)
@pytest.mark.parametrize("name", list(dc.SHAPES))
def test_rule_serves_every_shape(exe, synth, name, band_rows):
    s = dc.make(synth, name)
    r = _rule(exe, s, band_rows=band_rows)
    assert r["served"] == [[1]]
    band, nbands, px, rows, padl, pitch, lds, units, dband, dnbands, dpx, drows, dpitch, dlds, dunits = r["plan"][0]
    (oh, ow), region = synth.out_hw(s), dc.WAVE_LDS // 4
    assert px in (1, 2, 4) and dpx in (1, 2, 4) and pitch % 4 == dpitch % 4 == padl % 4 == 0 and padl >= s.pad_w
    assert 1 <= band <= (band_rows or oh) and 1 <= dband <= (band_rows or s.H)          # a forced band is obeyed
    assert rows * pitch <= region and drows * dpitch <= region and lds == 16 * rows * pitch and dlds == 16 * max(drows, 1) * dpitch
    assert units == s.N * s.group * nbands and dunits == s.N * s.C * dnbands
    # forward: the bands cover every output row once; a window is exactly the rows its taps reach; every column read is inside
    assert [b[0] for b in r["fwd"]] + [oh] == [0] + [b[1] for b in r["fwd"]] and len(r["fwd"]) == nbands
    for o0, o1, first, n in r["fwd"]:
        reach = [o * s.stride_h - s.pad_h + kr * s.dil_h for o in range(o0, o1) for kr in range(s.KH)]
        assert (first, first + n - 1) == (min(reach), max(reach)) and 0 < o1 - o0 <= band and n <= rows
    cols = [o * s.stride_w - s.pad_w + kc * s.dil_w + padl for o in range(-(-ow // 4) * 4) for kc in range(s.KW)]
    assert 0 <= min(cols) and max(cols) < pitch
    # data gradient: the bands cover every bottom row once; a band's top rows hold every row an entry contributes from
    assert [b[0] for b in r["bwd"]] + [s.H] == [0] + [b[1] for b in r["bwd"]] and len(r["bwd"]) == dnbands
    for h0, h1, first, n in r["bwd"]:
        th = [h + s.pad_h - kr * s.dil_h for h in range(h0, h1) for kr in range(s.KH)]
        src = [t // s.stride_h for t in th if t >= 0 and t % s.stride_h == 0 and t // s.stride_h < oh]
        assert all(first <= t < first + n for t in src) and n <= drows and 0 <= first and first + max(n, 0) <= oh
    choice = r["choice"][0]       # the option off, on under AUTO, on under GENERIC, on under BWD_MFMA, on with an inner plan
    assert choice[1:4] == [K_DEPTHWISE, K_GATHER, K_MFMA] and K_DEPTHWISE not in (choice[0], choice[4])


def test_rule_leaves_the_other_plans_alone(exe, synth):
    # Cg = 2; a double plan; three padded rows exceed a wave's region; 2.4e9 units
    for shape, f64 in [(dc.make(synth, "cg2"), False), (dc.make(synth, "3x3_s1"), True),
                       (synth.shape("long_row", 1, 2, 3, 3000, 2, 3, pad=1, group=2), False),
                       (synth.shape("units", 60000, 40000, 1, 1, 40000, 1, group=40000), False)]:
        r = _rule(exe, shape, f64=f64)
        assert r["served"] == [[0]] and "plan" not in r, shape.name
        assert r["choice"][0][0] == r["choice"][0][1] and K_DEPTHWISE not in r["choice"][0], shape.name
