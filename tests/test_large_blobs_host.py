"""The library's size limits without a GPU (include/escoin.h "Size limits"), and that the large-blob GPU cases
(large_common.py, test_large_blobs_gpu.py) exercise what they claim and can show the failures they are there for.

tests/cpp/launch_limits_check.cpp, compiled with plain g++ and no ROCm include path, holds every launch-time limit of
csrc/align_rules.h and every plan rule's 2^31 / 65535 limit to its edge (`edges`), and answers for each GPU case what the
rules make of it: the launches of launch_tiled, each one's epilogue path and compiled body (`cases`)."""
import json
import os
import subprocess

import numpy as np
import pytest

import large_common as lg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"AUTO": 0, "GENERIC": 1, "TILED": 2, "DENSE": 3}

REFUSALS = lg.REFUSALS


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    out = tmp_path_factory.mktemp("launch_limits")
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    exe = str(out / "launch_limits_check")
    srcs = [os.path.join(ROOT, "tests", "cpp", "launch_limits_check.cpp")] + [os.path.join(csrc, f) for f in
                                                                             ("align_rules.cpp", "stream_builder.cpp", "jit_codegen.cpp")]
    flags = ["g++", "-O2", "-std=c++17", "-I" + csrc, "-I" + os.path.join(ROOT, "include")]      # no ROCm include path
    procs = [subprocess.Popen(flags + ["-c", s, "-o", str(out / (os.path.basename(s) + ".o"))]) for s in srcs]
    assert all(p.wait() == 0 for p in procs)
    subprocess.check_call(flags + ["-o", exe] + [str(out / (os.path.basename(s) + ".o")) for s in srcs] + ["-lpthread"])
    return exe, out


def _rules(tool, synth, rows):
    """What the rules make of (layer, plan's batch, kernel, images of the call) rows, one dict each."""
    exe, out = tool
    lines = []
    for layer, plan_n, kernel, n in rows:
        path = str(out / ("w_%s.f32" % layer))
        if not os.path.exists(path):
            lg.pattern(synth, layer)[1].astype(np.float32).tofile(path)
        s = lg.shape(synth, layer, plan_n)
        lines.append(" ".join(str(int(v)) for v in (s.N, s.C, s.H, s.W, s.M, s.KH, s.KW, s.pad_h, s.pad_w, s.stride_h, s.stride_w, s.dil_h,
                                                    s.dil_w, s.group, KERNELS[kernel], n, lg.N_CU)) + " " + path)
    manifest = str(out / "manifest.txt")
    with open(manifest, "w") as f:
        f.write("\n".join(lines) + "\n")
    run = subprocess.run([exe, "cases", manifest], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = run.stdout.decode()
    assert run.returncode == 0, text
    got = [json.loads(l) for l in text.splitlines()]
    assert len(got) == len(rows), text
    return got


def test_every_limit_flips_at_its_documented_value(tool):
    run = subprocess.run([tool[0], "edges"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = run.stdout.decode()
    assert run.returncode == 0 and "FAIL" not in text and text.rstrip().endswith(", 0 failed"), text
    # the edges the cases are built on are among the checks
    for what in ("epi_store: true at 2^31 - 4 bytes, false at 2^31", "dense: 0xFFFFFFF0 - 4 bytes of bottom or of weights pass",
                 "dense: 0xFFFFFFF0 bytes of bottom or of weights are refused",
                 "tiled: with the real limit a launch takes (0xFFFFFFF0 - 16) / in_image = 16383 images of 2^18 bytes"):
        assert "ok    " + what in text, what


def test_the_gpu_cases_exercise_what_they_claim(tool, synth):
    """For every forward case the rules give the launches, the epilogue path and the compiled body the case names, and the
    kernel it forces accepts the size."""
    cases = lg.FORWARD
    assert len(set(map(lg.case_id, cases))) == len(cases)
    got = _rules(tool, synth, [(c.layer, c.plan_n, c.kernel, c.n) for c in cases])
    for c, r in zip(cases, got):
        what = (lg.case_id(c), r)
        if c.kernel == "AUTO":
            assert r["jit"] == 1 and "generated-code" in r["tiling_info"], what
        if c.kernel == "TILED":
            assert r["jit"] == 0 and r["tiling_info"].startswith("stream "), what
        if c.kernel in ("AUTO", "TILED"):
            assert r["tiled_error"] == "" and r["launches"] == c.launches, what
            assert (r["epi_store_first"], r["epi_store_last"]) == c.epi and (r["body_variant_first"], r["body_variant_last"]) == c.body, what
            assert r["first_images"] + (r["launches"] - 2) * r["chunk"] + r["last_images"] == c.n if r["launches"] > 1 else r["first_images"] == c.n, what
        if c.kernel == "GENERIC":
            assert r["generic_error"] == "", what
        if c.kernel == "DENSE":
            assert r["dense_error"] == "", what
    # the edges really are edges: the top of the N below is the last under 2^31 bytes, a second launch starts at 0xFFFFFFF0 - 16
    for c in cases:
        top = 4 * lg.top_image_elems(synth, c.layer)
        if c.epi == (1, 1) and c.plan_n > c.n and c.launches == 1 and top * c.plan_n >= 2 ** 31:
            assert top * c.n < 2 ** 31 <= top * (c.n + 1) and c.plan_n == c.n + 1, lg.case_id(c)
        if c.launches == 2:
            l = lg.LAYERS[c.layer]
            image = 4 * l.C * l.H * l.W
            chunk = (0xFFFFFFF0 - 16) // image
            assert chunk < c.n <= chunk + 2 and 2 ** 32 - image <= chunk * image < 2 ** 32, lg.case_id(c)


def test_the_refusals_are_the_rules(tool, synth):
    got = _rules(tool, synth, [(layer, n, "AUTO", n) for layer, n, _, _ in REFUSALS] + [("c3_bottom", 16383, "DENSE", 16383),
                                                                                         ("sp_strided", 2047, "AUTO", 2047),
                                                                                         ("one", 65535, "GENERIC", 65535)])
    for (layer, n, key, msg), r in zip(REFUSALS, got):
        assert r[key] == msg, (layer, n, r)
    assert got[3]["dense_error"] == "" and got[4]["tiled_error"] == "" and got[5]["generic_error"] == "", got[3:]
    l = lg.LAYERS["c3_bottom"]
    assert 16384 * l.C * l.H * l.W * 4 == 2 ** 32
    assert 2048 * lg.top_image_elems(synth, "sp_strided") * 4 == 2 ** 31


def test_the_backward_inputs_show_a_displaced_image_and_the_weight_reference_is_the_batch_s(synth):
    """A bottom_diff that comes from 2^31 or 2^32 bytes or elements away violates backward_bound on every image; and the
    weight gradient summed from the pattern images' gradients is the float64 gradient of the batch itself."""
    from wgrad_common import torch_backward
    want, B = lg.bwd_reference(synth)[:2]
    per = want[0].size
    for elems in (2 ** 29, 2 ** 30, 2 ** 31, 2 ** 32):
        assert elems % per == 0 and (elems // per) % lg.PERIOD != 0
        assert lg.displaced_violates(want, B, elems) and lg.displaced_violates(want, B, -elems), elems
    assert (np.abs(lg.SENTINEL - want) > B).reshape(lg.PERIOD, -1).any(axis=1).all()
    s28, w, b, _, x28 = lg.pattern(synth, lg.BWD_LAYER)
    td28 = lg.bwd_pattern(synth)[1]
    n = 61
    idx = np.arange(n) % lg.PERIOD
    (ww, wb), (Bw, Bb) = lg.weight_reference(synth, n)
    _, wd, bsd = torch_backward(x28[idx], w, b, s28, td28[idx])
    # two float64 sums of the same terms in different orders: far inside the float bound
    assert (np.abs(wd - ww) <= 1e-6 * Bw).all() and (np.abs(bsd - wb) <= 1e-6 * Bb).all()
    assert np.abs(wd).max() > 0 and (ww[w == 0] == 0).all()


def _worst(got, want, B):
    return float((np.abs(got - want) / B).max())


@pytest.mark.parametrize("n", sorted(set(n for n, _ in lg.BWD_WGRAD)))
def test_the_weight_and_bias_bounds_show_nothing_written_a_lost_tail_and_a_displaced_top_diff(synth, n):
    """With the bound of the reduction's depth (large_common.weight_reference), at every batch of the GPU cases: (a) a
    gradient of zeros, (b) a batch whose images from 2^31 or 2^32 bytes or 2^31 elements of top_diff on are lost and
    (c) one whose top_diff is read that far back violate the weight bound; (a) and (b) the bias bound too.  (b) and (c)
    need more than one image past the edge: the batches one image past it (the edges themselves) are there for the
    kernels' indexing at the edge, the batches 512 and 1024 past it for what lies beyond.  A displaced top_diff moves
    the bias gradient only by the images at the two ends of the window it sums -- a bias does not know which image is
    which -- so (c) is not asked of the bias."""
    (ww, wb), (Bw, Bb) = lg.weight_reference(synth, n)
    assert _worst(0 * ww, ww, Bw) > 100 and _worst(0 * wb, wb, Bb) > 100
    oh, ow = synth.out_hw(lg.shape(synth, lg.BWD_LAYER, 1))
    assert lg.reduction_depth(synth, n) == 1024 + -(-n * oh * ow // 1024)
    shown = 0
    for edge in lg.BWD_EDGES:
        if n - edge < 512:
            continue
        shown += 1
        lost = lg.batch_gradient(synth, n, lost_from=edge)
        assert _worst(lost[0], ww, Bw) > 10 and _worst(lost[1], wb, Bb) > 10, (n, edge)
        moved = lg.batch_gradient(synth, n, displaced=edge)
        assert _worst(moved[0], ww, Bw) > 10, (n, edge)
    assert shown >= 1
    # every edge is more than 512 images inside one of the batches
    assert all(any(m - edge >= 512 for m, _ in lg.BWD_WGRAD) for edge in lg.BWD_EDGES)


def test_the_mfma_case_s_weight_bound_shows_zeros_and_a_lost_tail(synth):
    """The dense weight gradient at 32767 images of 1 x 256 x 256 (large_common.MFMA_LAYER), bounded by the depth of
    dense_wgrad's reduction (the GPU test reads the plan's splits; here three spans around it): zeros and a batch that
    lost everything past 2^31 bytes of the bottom violate it.  And its data gradient shows a displaced image."""
    n, layer = lg.MFMA_MAX_IMAGES, lg.MFMA_LAYER
    l = lg.LAYERS[layer]
    assert n * l.H * l.W == 2 ** 31 - 2 ** 16
    for span in (1, 128, 512):
        (ww, _), (Bw, _) = lg.weight_reference(synth, n, layer, chunk_span=span)
        assert _worst(0 * ww, ww, Bw) > 10, span
        lost = lg.batch_gradient(synth, n, layer, lost_from=2 ** 31 // (4 * l.H * l.W))
        assert _worst(lost[0], ww, Bw) > 10, span
    want, B = lg.bwd_reference(synth, layer)
    for elems in (2 ** 29, 2 ** 30, 2 ** 31):
        assert lg.displaced_violates(want, B, elems) and lg.displaced_violates(want, B, -elems), elems


def test_the_backward_and_inner_cases_claim_what_the_rules_give(tool, synth):
    """The transposed data gradient of BWD_LAYER is a forward of the c3_bottom geometry with top_diff as its bottom: one
    launch past 2^31 bytes at 8193 images, two at 16385, which the forward cases of that layer claim and
    test_the_gpu_cases_exercise_what_they_claim holds to the rules."""
    a, t = lg.LAYERS[lg.BWD_LAYER], lg.LAYERS["c3_bottom"]
    assert (a.M, a.H, a.W, a.C, a.K, a.K - 1 - a.pad, a.stride, a.dil, a.group) == (t.C, t.H, t.W, t.M, t.K, t.pad, t.stride, t.dil, t.group)
    claimed = dict(((c.n, c.kernel), c.launches) for c in lg.FORWARD if c.layer == "c3_bottom" and c.plan_n == c.n)
    for n, kn in lg.BWD_DATA:
        if kn in ("AUTO", "TILED"):
            assert claimed[(n, kn)] == (1 if n == 8193 else 2), (n, kn)
    assert 8193 * a.M * a.H * a.W * 4 > 2 ** 31 and 16385 * a.M * a.H * a.W * 4 > 2 ** 32


@pytest.mark.parametrize("layer", sorted(set(c.layer for c in lg.FORWARD) | set(l for l, _, _ in lg.INNER)))
def test_the_inputs_show_a_displaced_image_and_a_stale_sentinel(synth, layer):
    """An output that comes from 2^31 or 2^32 bytes, or 2^31 or 2^32 elements, away in the blob violates the bound on at
    least one element of every image, and so does the sentinel left in place."""
    want, B = lg.reference(synth, layer)
    per = lg.top_image_elems(synth, layer)
    assert want.shape[0] == lg.PERIOD and want[0].size == per
    for elems in (2 ** 29, 2 ** 30, 2 ** 31, 2 ** 32):
        assert elems % (lg.PERIOD * per) != 0
        if elems % per == 0:      # whole images: a count that is no multiple of the period
            assert (elems // per) % lg.PERIOD != 0
        assert lg.displaced_violates(want, B, elems), (layer, elems)
        assert lg.displaced_violates(want, B, -elems), (layer, -elems)
    stale = np.abs(lg.SENTINEL - want) > B
    assert stale.reshape(lg.PERIOD, -1).any(axis=1).all(), layer
    # ... and the bottom side: a forward whose every INPUT element is read from that far away in the periodic bottom blob
    # (another image where the distance is whole images, a splice of two otherwise) violates the bound on every image
    import errbound as eb
    s28, w, b, _, x28 = lg.pattern(synth, layer)
    for elems in (2 ** 29, 2 ** 30, 2 ** 31, 2 ** 32):
        assert elems % x28.size != 0
        for sign in (1, -1):
            moved = np.roll(x28.reshape(-1), -sign * (elems % x28.size)).reshape(x28.shape)
            got = np.maximum(eb.conv64(moved, w, b, s28), 0.0)
            assert (np.abs(got - want) > B).reshape(lg.PERIOD, -1).any(axis=1).all(), (layer, sign * elems)


# ---- option "deconv": large_common.DC_LAYER ----------------------------------------------------------------------------------------
def test_the_deconv_cases_are_at_the_edges_they_claim(pkg):
    """The top of 8191 images is the last under 2^31 bytes and that of 16385 the first past 2^32; T' passes 2^31 bytes in all
    of them and 2^32 in the last; every ELEMENT offset stays under 2^31.  32768 images, a top of exactly 2^31 elements, are
    refused at the align by d2s_plan's message for the top -- on the host as on the device, before anything is allocated --
    and this layer's T' gets there first: 29026 images are the last it serves (test_d2s_host.py holds each limit of
    d2s_plan to its own edge on layers made for it)."""
    import d2s_common as dc
    s = lg.DC_LAYER
    P, kh, kw, hi, wi = dc.inner_dims(s)
    assert s.M * dc.out_hw(s)[0] * dc.out_hw(s)[1] == lg.DC_TOP_IMAGE == 2 ** 16 and s.M * P * hi * wi == lg.DC_T_IMAGE == 73984
    assert (P, kh, kw, hi, wi) == (4, 2, 2, 17, 17)
    assert 8191 * lg.DC_TOP_IMAGE * 4 < 2 ** 31 == 8192 * lg.DC_TOP_IMAGE * 4 < 8191 * lg.DC_T_IMAGE * 4
    assert 16384 * lg.DC_TOP_IMAGE * 4 == 2 ** 32 < 16385 * lg.DC_T_IMAGE * 4 and 16385 * lg.DC_T_IMAGE < 2 ** 31
    assert lg.DC_BACKWARD_N * lg.DC_TOP_IMAGE * 4 > 2 ** 31 and lg.DC_REFUSED_N * lg.DC_TOP_IMAGE == 2 ** 31
    # what a case holds: bottom, top and the plan's T' / G' scratch (for the backward top_diff and bottom_diff as well)
    per_in = s.C * s.H * s.W
    assert all(lg.need_bytes(c.n * per_in, c.plan_n * lg.DC_TOP_IMAGE) + 4 * c.plan_n * lg.DC_T_IMAGE <= lg.MAX_CASE_BYTES for c in lg.DC_FORWARD)
    n = lg.DC_BACKWARD_N
    assert lg.need_bytes(n * per_in, n * per_in, n * lg.DC_TOP_IMAGE) + 4 * n * lg.DC_T_IMAGE <= lg.MAX_CASE_BYTES
    w = lg.dc_pattern()[1]
    for images, why in ((29026, None), (29027, "the inner top T' reaches 2^31 elements"), (lg.DC_REFUSED_N, lg.DC_TOP_REFUSAL)):
        plan = pkg.Plan(dc.desc(pkg, lg.dc_shape(images), True, True), deconv=1)
        if why is None:
            plan.weight_align_cpu(w)
            assert plan.stat("host_aligned") == 1
        else:
            with pytest.raises(pkg.EscoinError) as e:
                plan.weight_align_cpu(w)
            assert "failed (-1)" in str(e.value) and why in str(e.value), str(e.value)
            assert plan.stat("host_aligned") == 0
        plan.close()


def test_the_deconv_inputs_show_a_displaced_image_a_displaced_inner_image_and_a_stale_sentinel(synth):
    """For DC_LAYER's pattern: a top image stored 2^31 or 2^32 bytes or elements away from its place (the top image is 2^16
    elements: whole images, a count that is no multiple of the period), a T' image READ from that far away -- a T' image is
    73984 elements, no power of two, so the displaced read is a splice of two pattern images and the proof is run, not
    inferred -- and the sentinel left in place each violate the bound on at least one element of every image."""
    import d2s_common as dc
    want, B = lg.dc_reference(synth)
    s28, _, b = lg.dc_pattern()[:3]
    assert want.shape == (lg.PERIOD, s28.M) + dc.out_hw(s28) and want[0].size == lg.DC_TOP_IMAGE
    t = lg.dc_inner_top(synth)
    assert t[0].size == lg.DC_T_IMAGE
    honest = lg.dc_top_of(s28, t, b)
    assert (np.abs(honest - want) <= 1e-6 * B).all()       # (the same float64 sums: the proof below starts from the reference)
    for elems in (2 ** 29, 2 ** 30, 2 ** 31, 2 ** 32):
        assert elems % lg.DC_TOP_IMAGE == 0 and (elems // lg.DC_TOP_IMAGE) % lg.PERIOD != 0 and elems % t.size != 0
        for sign in (1, -1):
            assert lg.displaced_violates(want, B, sign * elems), (sign * elems, "top")
            moved = np.roll(t.reshape(-1), -sign * (elems % t.size)).reshape(t.shape)
            bad = np.abs(lg.dc_top_of(s28, moved, b) - want) > B
            assert bad.reshape(lg.PERIOD, -1).any(axis=1).all(), (sign * elems, "T'")
    assert (np.abs(lg.SENTINEL - want) > B).reshape(lg.PERIOD, -1).any(axis=1).all()
    # the data gradient likewise (bottom_diff images of 2^12 elements)
    bwant, bB = lg.dc_bwd_reference(synth)
    for elems in (2 ** 29, 2 ** 31):
        assert lg.displaced_violates(bwant, bB, elems) and lg.displaced_violates(bwant, bB, -elems), elems


def test_the_deconv_weight_and_bias_bounds_show_nothing_written_and_a_lost_tail(synth):
    """With the bound of the reduction's depth (large_common.dc_weight_reference) at the backward case's batch: a gradient of
    zeros violates the weight and the bias bound, and so does a batch that lost what lies past 2^31 bytes of top_diff -- one
    image, so the case's batch has a second size 512 images on for the weights (the suite's rule for an edge)."""
    import d2s_common as dc
    n = lg.DC_BACKWARD_N
    (ww, wb), (Bw, Bb) = lg.dc_weight_reference(n)
    assert _worst(0 * ww, ww, Bw) > 100 and _worst(0 * wb, wb, Bb) > 100
    w = lg.dc_pattern()[1]
    assert ww.shape == w.shape and (ww[w == 0] == 0).all() and np.isfinite(Bw).all()
    (lw, lb), _ = lg.dc_weight_reference(n + 512, lost_from=8192)
    (ww2, wb2), (Bw2, Bb2) = lg.dc_weight_reference(n + 512)
    assert _worst(lw, ww2, Bw2) > 10 and _worst(lb, wb2, Bb2) > 10
    # ... and the sum of the pattern images' gradients is the gradient of the batch itself
    s28, w, b, _, x28, _, td28 = lg.dc_pattern()
    idx = np.arange(61) % lg.PERIOD
    (w61, b61), (B61, Bb61) = lg.dc_weight_reference(61)
    _, wd, bsd = dc.ref_backward(s28, w, x28[idx], b, td28[idx])
    assert (np.abs(wd - w61) <= 1e-6 * B61).all() and (np.abs(bsd - b61) <= 1e-6 * Bb61).all() and np.abs(wd).max() > 0
