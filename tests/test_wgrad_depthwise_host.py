"""Plan option "wgrad_depthwise" without a GPU: the options' values and refusals, and -- through
tests/cpp/wgrad_depthwise_rule_check.cpp, compiled with plain g++ and no ROCm include path -- align_rules.h dww_plan, bwd_choice's
decision and csr_tables.h dww_segments on the cases of wgrad_depthwise_common.py."""
import os
import subprocess

import pytest

import depthwise_common as dc
import wgrad_depthwise_common as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY, POINTWISE, DEPTHWISE, MEG = 1, 4, 5, 1000000


def test_option_values_and_refusals(pkg, synth):
    assert pkg.WGRAD_DEPTHWISE == DEPTHWISE
    s, w = dc.case(synth, "3x3_s1")[:2]
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s), wgrad_depthwise=1, wgrad_depthwise_slices=3)
    for key, v in (("wgrad_depthwise", 2), ("wgrad_depthwise", -1), ("wgrad_depthwise_slices", -1), ("wgrad_kernel", DEPTHWISE)):
        with pytest.raises(pkg.EscoinError) as e:
            plan.set_option(key, v)
        assert "failed (-1)" in str(e.value) and key in str(e.value)        # ESCOIN_EINVAL
    assert plan.stat("wgrad_depthwise_slices") == 0                         # nothing has run
    plan.weight_align_cpu(w)                                                # CPU mode ignores it
    plan.close()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    out = str(tmp_path_factory.mktemp("dww") / "wgrad_depthwise_rule_check")
    srcs = [os.path.join(ROOT, "tests", "cpp", "wgrad_depthwise_rule_check.cpp")] + [
        os.path.join(csrc, f) for f in ("align_rules.cpp", "csr_tables.cpp", "stream_builder.cpp", "jit_codegen.cpp")]
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-o", out] + srcs + ["-lpthread"])
    return out


def _rule(exe, s, f64=False, band_rows=0, slices=0, n_cu=256, n_images=1, row_len=None):
    words = list(s[1:15]) + [int(f64), band_rows, slices, n_cu, n_images, s.KH * s.KW if row_len is None else row_len]
    out = {}
    for line in subprocess.check_output([exe] + [str(v) for v in words], timeout=60).decode().splitlines():
        out.setdefault(line.split()[0], []).append([int(v) for v in line.split()[1:]])
    return out


@pytest.mark.parametrize("name,opts,px,slices", sorted({(n, o, px, sl) for n, _, o, px, sl in wc.CASES}))
def test_rule_and_segments_on_every_case(exe, synth, name, opts, px, slices):
    s = wc.case(synth, name)[0]
    r = _rule(exe, s, band_rows=opts[0], slices=opts[1], n_images=s.N - 1)
    assert r["served"] == [[1]] and r["refused"] == [[1, 1, 1]]
    band, nbands, got_px, S, per, part, full = r["plan"][0]
    # the pinned instantiation and slices; the band obeys its cap; a partial batch has the slices its pairs fill
    assert (got_px, full) == (px, slices) and 1 <= band <= (opts[0] or s.H) and full <= S and part == -(-(s.N - 1) * nbands // per)
    # off: AUTO's kernel, the chunks; on: the kernel, a slab of max(chunks, S) rows; a forced ENTRY wins; "wgrad_pointwise" does not serve these
    off, on, forced, both = r["choice"][0]
    assert off // MEG != DEPTHWISE and on == DEPTHWISE * MEG + max(off % MEG, S) and forced == ENTRY * MEG + off % MEG and both == on
    # segments: rows in order, every entry in exactly one, at most 16 each, the empty row 0 keeps one
    taps, want, e = s.KH * s.KW, [[0, 0, 0]], 0
    for oc in range(1, s.M):
        want += [[oc, e + j, min(16, taps - j)] for j in range(0, taps, 16)]
        e += taps
    assert r["seg"] == want


def test_slice_lengths_clamps_and_unserved_plans(exe, synth):
    # 3x3_s1 in bands of 2 rows (few CUs leave the rule's band above 2): 10 pairs in slices of 4, 4 and 2; one image: 5 pairs, 2 slices
    assert _rule(exe, dc.make(synth, "3x3_s1"), band_rows=2, slices=3, n_cu=1)["plan"] == [[2, 5, 1, 3, 4, 2, 3]]
    assert _rule(exe, dc.make(synth, "img7"), band_rows=1, slices=1000)["plan"][0][3:5] == [21, 1]       # S is clamped to the pairs
    # a 1x1 depthwise plan with both options on is the pointwise kernel's
    pw = _rule(exe, synth.shape("dw1x1", 2, 4, 5, 5, 4, 1, group=4), row_len=1)
    assert [c // MEG for c in pw["choice"][0][1:]] == [DEPTHWISE, ENTRY, POINTWISE]
    for shape, f64 in [(dc.make(synth, "cg2"), False), (dc.make(synth, "3x3_s1"), True)]:       # Cg = 2; a double plan
        r = _rule(exe, shape, f64=f64)
        assert r["served"] == [[0]] and r["choice"][0][0] == r["choice"][0][1] and r["choice"][0][1] // MEG != DEPTHWISE
