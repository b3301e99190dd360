"""Every forward kernel on activation blobs past 2 GiB and 4 GiB on the MI355X (large_common.py has the cases and what
each claims; test_large_blobs_host.py holds the rules to the claims and proves the inputs show a displaced image): every
element of the whole top blob within errbound.py's derived bound of the float64 reference, the top between two 1 MiB
guard zones of the sentinel that must stay intact, on partial batches the images past the call's untouched, and the kernel
that ran asserted by name, tiling line and stats.  The launch-time refusals run on really allocated blobs and must leave
the whole top at the sentinel.

The worst err / bound and the peak device memory per case are printed when the module ends (pytest -s;
profiles/errbound.md "Blobs past 2 and 4 GiB")."""
import re
import time

import numpy as np
import pytest

import errbound as eb
import large_common as lg
from large_common import DENSE_RANGE, GENERIC_GRID, REFUSALS, STRIDED_TOP
from wgrad_common import csr_positions

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

REPORT = []
_ON_DEVICE = {}


@pytest.fixture(scope="module")
def dev(pkg):
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        pytest.fail("no HIP device visible (these tests run on the MI355X)")
    yield torch.device("cuda:0")
    _ON_DEVICE.clear()
    torch.cuda.empty_cache()
    for line in REPORT:
        print(line)


def _layer_on_device(synth, dev, layer):
    """(weights, bias, base images, want, B) of a layer: the host arrays and, uploaded once, the device tensors."""
    if layer not in _ON_DEVICE:
        _, w, b, base, _ = lg.pattern(synth, layer)
        want, B = lg.reference(synth, layer)
        _ON_DEVICE[layer] = (w, torch.from_numpy(b).to(dev), torch.from_numpy(base).to(dev), torch.tensor(want, device=dev),
                             torch.tensor(B, device=dev))      # (the reference itself stays read-only on the host)
    return _ON_DEVICE[layer]


def _release():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _ran(pkg, c, plan):
    """The kernel the case names is the one the plan runs (before a launch) ..."""
    name, info = plan.kernel_name, plan.tiling_info
    if c.kernel == "AUTO":
        assert "jit" in name and "generated-code" in info and plan.stat("kernel_choice") == pkg.KERNEL_JIT, (name, info)
    elif c.kernel == "TILED":
        assert "tiled" in name and info.startswith("stream ") and plan.stat("kernel_choice") == pkg.KERNEL_TILED, (name, info)
    elif c.kernel == "GENERIC":
        assert "generic" in name and info == "" and plan.stat("kernel_choice") == pkg.KERNEL_GENERIC, (name, info)
    else:
        assert name == "escoin_dense_mfma_kernel" and plan.stat("kernel_choice") == pkg.KERNEL_DENSE and plan.stat("dense_variant") == 0, name
    return name, info


def _launched(c, plan):
    """... and after it: the compiled body of the last launch of a tiled plan, a variant of the dense kernel."""
    if c.kernel in ("AUTO", "TILED"):
        assert plan.stat("body_variant") == c.body[1], (lg.case_id(c), plan.stat("body_variant"))
        return "body_variant %d" % c.body[1]
    if c.kernel == "DENSE":
        v = plan.stat("dense_variant")
        assert v > 0 and plan.stat("streamk_gave_up") == 0, v
        return "dense_variant %d" % v
    return ""


@pytest.mark.parametrize("c", lg.FORWARD, ids=[lg.case_id(c) for c in lg.FORWARD])
def test_forward_every_element_of_a_large_blob_with_bias_and_relu(pkg, synth, dev, c):
    t0 = time.time()
    s = lg.shape(synth, c.layer, c.plan_n)
    oh, ow = synth.out_hw(s)
    per_in, per_out = s.C * s.H * s.W, s.M * oh * ow
    w, bd, base, want, B = _layer_on_device(synth, dev, c.layer)
    lg.require_memory(torch, pytest, lg.need_bytes(c.n * per_in, c.plan_n * per_out), lg.case_id(c))
    torch.cuda.reset_peak_memory_stats()
    x = torch.empty((c.n, s.C, s.H, s.W), device=dev, dtype=torch.float32)
    lg.fill_pattern(torch, x, base)
    buf, top = lg.guarded(torch, dev, (c.plan_n, s.M, oh, ow))
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=True), kernel=getattr(pkg, "KERNEL_" + c.kernel), **c.options)
    try:
        plan.weight_align(w)
        name, info = _ran(pkg, c, plan)
        plan.forward(x, bd, top[:c.n])
        torch.cuda.synchronize()
        variant = _launched(c, plan)
        ratio, bad = lg.worst_ratio(torch, top[:c.n], want, B)
        peak = torch.cuda.max_memory_allocated() + plan.workspace_bytes
        print("large forward %-40s %s | %s %s: worst err / bound %.3g, first violation %s, peak %.2f GiB, %.1f s" %
              (lg.case_id(c), name, info, variant, ratio, bad, peak / 2.0 ** 30, time.time() - t0))
        assert lg.guards_intact(buf), (lg.case_id(c), "a guard zone around the top was written")
        if c.plan_n > c.n:
            assert lg.all_sentinel(torch, top[c.n:]), (lg.case_id(c), "images past the call's were written")
        assert bad is None and ratio <= 1.0, "%s via %s %s: element %s is off by %.3g x its bound" % (lg.case_id(c), name, variant, bad, ratio)
        assert peak <= lg.MAX_CASE_BYTES, peak
        REPORT.append("large forward worst %-40s %-48s %-16s %.3g   peak %.2f GiB" % (lg.case_id(c), name, variant, ratio, peak / 2.0 ** 30))
    finally:
        plan.close()
        del x, top, buf
        _release()


# ---- plans that rearrange the bottom for an inner plan: s2d, s2b, b2s ------------------------------------------------------
@pytest.mark.parametrize("layer,n,option", lg.INNER, ids=[o for _, _, o in lg.INNER])
def test_forward_through_an_inner_plan_on_a_rearranged_large_bottom(pkg, synth, dev, layer, n, option):
    t0 = time.time()
    s = lg.shape(synth, layer, n)
    oh, ow = synth.out_hw(s)
    per_in, per_out = s.C * s.H * s.W, s.M * oh * ow
    w, bd, base, want, B = _layer_on_device(synth, dev, layer)
    torch.cuda.reset_peak_memory_stats()
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=True), **{option: 1})
    x = top = buf = None
    try:
        plan.weight_align(w)
        scratch = plan.stat(option + "_scratch_bytes")
        assert plan.stat(option) == 1 and scratch > 0, plan.kernel_name
        need = lg.need_bytes(n * per_in, n * per_out)
        assert need + scratch <= lg.MAX_CASE_BYTES, (need, scratch)
        lg.require_memory(torch, pytest, need, (layer, n, option))
        x = torch.empty((n, s.C, s.H, s.W), device=dev, dtype=torch.float32)
        lg.fill_pattern(torch, x, base)
        buf, top = lg.guarded(torch, dev, (n, s.M, oh, ow))
        plan.forward(x, bd, top)
        torch.cuda.synchronize()
        ratio, bad = lg.worst_ratio(torch, top, want, B)
        peak = torch.cuda.max_memory_allocated() + plan.workspace_bytes
        print("large forward %s-%d-%s %s | %s: scratch %.2f GiB, worst err / bound %.3g, first violation %s, peak %.2f GiB, %.1f s" %
              (layer, n, option, plan.kernel_name, plan.tiling_info, scratch / 2.0 ** 30, ratio, bad, peak / 2.0 ** 30, time.time() - t0))
        assert lg.guards_intact(buf), (option, "a guard zone around the top was written")
        assert bad is None and ratio <= 1.0, "%s via %s: element %s is off by %.3g x its bound" % (option, plan.kernel_name, bad, ratio)
        assert peak <= lg.MAX_CASE_BYTES, peak
        REPORT.append("large forward worst %-40s %-48s %-16s %.3g   peak %.2f GiB" % ("%s-%d-%s" % (layer, n, option), plan.kernel_name[:48], "", ratio,
                                                                                      peak / 2.0 ** 30))
    finally:
        plan.close()
        del x, top, buf
        _release()


# ---- the Backward: top_diff is the large blob ----------------------------------------------------------------------------
@pytest.mark.parametrize("n,kn", lg.BWD_DATA, ids=["%d-%s" % c for c in lg.BWD_DATA])
def test_backward_data_gradient_of_a_large_top_diff(pkg, synth, dev, n, kn):
    """bottom_diff of every image within errbound.backward_bound, under the transposed plan (AUTO, JIT, TILED: top_diff
    is its bottom, past 2^31 bytes in one launch at 8193 images, in two launches at 16385) and the gather kernel."""
    t0 = time.time()
    layer = lg.BWD_LAYER
    s = lg.shape(synth, layer, n)
    oh, ow = synth.out_hw(s)
    w = lg.pattern(synth, layer)[1]
    key = ("bwd", layer)
    if key not in _ON_DEVICE:
        ref = lg.bwd_reference(synth, layer)
        _ON_DEVICE[key] = (torch.from_numpy(lg.bwd_pattern(synth, layer)[0]).to(dev), torch.tensor(ref[0], device=dev), torch.tensor(ref[1], device=dev))
    tdbase, want, B = _ON_DEVICE[key]
    # (the transposed plan keeps a gated copy of top_diff's size for plans with a ReLU; this one has none)
    lg.require_memory(torch, pytest, lg.need_bytes(n * s.M * oh * ow, n * s.C * s.H * s.W), (layer, n, kn))
    torch.cuda.reset_peak_memory_stats()
    td = torch.empty((n, s.M, oh, ow), device=dev, dtype=torch.float32)
    lg.fill_pattern(torch, td, tdbase)
    buf, bdiff = lg.guarded(torch, dev, (n, s.C, s.H, s.W))
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s), backward_kernel=getattr(pkg, "KERNEL_" + kn))
    try:
        plan.weight_align(w)
        plan.backward(td, bottom_diff=bdiff)
        torch.cuda.synchronize()
        ran = plan.stat("bwd_data_kernel")
        assert ran == (pkg.KERNEL_JIT if kn == "AUTO" else getattr(pkg, "KERNEL_" + kn)), (kn, ran)
        ratio, bad = lg.worst_ratio(torch, bdiff, want, B)
        peak = torch.cuda.max_memory_allocated() + plan.workspace_bytes
        print("large backward data %d-%s bwd_data_kernel %d: worst err / bound %.3g, first violation %s, peak %.2f GiB, %.1f s" %
              (n, kn, ran, ratio, bad, peak / 2.0 ** 30, time.time() - t0))
        assert lg.guards_intact(buf), (n, kn, "a guard zone around bottom_diff was written")
        assert bad is None and ratio <= 1.0, "data gradient %d-%s: element %s is off by %.3g x its bound" % (n, kn, bad, ratio)
        assert peak <= lg.MAX_CASE_BYTES, peak
        REPORT.append("large backward data worst %-16s bwd_data_kernel %d   %.3g   peak %.2f GiB" % ("%d-%s" % (n, kn), ran, ratio, peak / 2.0 ** 30))
    finally:
        plan.close()
        del td, bdiff, buf
        _release()


@pytest.mark.parametrize("n,wk", lg.BWD_WGRAD, ids=["%d-%s" % c for c in lg.BWD_WGRAD])
def test_backward_weight_and_bias_gradient_of_a_large_top_diff(pkg, synth, dev, n, wk):
    """The weight gradient, dense and compact, and the bias gradient of the whole batch under each stage-1 kernel: the
    float64 reference is the sum of the 28 pattern images' gradients, each as often as it occurs in the batch."""
    t0 = time.time()
    layer = lg.BWD_LAYER
    s = lg.shape(synth, layer, n)
    oh, ow = synth.out_hw(s)
    w, _, base, _, _ = _layer_on_device(synth, dev, layer)
    tdbase = torch.from_numpy(lg.bwd_pattern(synth, layer)[0]).to(dev)
    (want_w, want_b), (B_w, B_b) = lg.weight_reference(synth, n, layer)
    lg.require_memory(torch, pytest, lg.need_bytes(n * s.M * oh * ow, n * s.C * s.H * s.W), (layer, n, wk))
    torch.cuda.reset_peak_memory_stats()
    td = torch.empty((n, s.M, oh, ow), device=dev, dtype=torch.float32)
    lg.fill_pattern(torch, td, tdbase)
    x = torch.empty((n, s.C, s.H, s.W), device=dev, dtype=torch.float32)
    lg.fill_pattern(torch, x, base)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s), backward_kernel=pkg.KERNEL_GENERIC, wgrad_kernel=getattr(pkg, "WGRAD_" + wk))
    try:
        plan.weight_align(w)
        if wk == "STAGED" and n > lg.STAGED_MAX_IMAGES:
            with pytest.raises(pkg.EscoinError, match=r"\(-1\): " + re.escape(lg.STAGED_REFUSAL)):
                plan.backward(td, bottom=x, bottom_diff=None, weight_diff=True, bias_diff=True)
            return
        _, wd, bsd = plan.backward(td, bottom=x, bottom_diff=None, weight_diff=True, bias_diff=True)
        _, vd, bsd2 = plan.backward(td, bottom=x, bottom_diff=None, values_diff=True, bias_diff=True)
        torch.cuda.synchronize()
        ran = plan.stat("wgrad_kernel")
        assert ran == getattr(pkg, "WGRAD_" + wk), (wk, ran)
        name = "wgrad_kernel %d" % ran
        wdn = wd.cpu().numpy()
        r = eb.within(wdn, want_w, B_w, name, what=(n, wk, "weights"))
        rb = eb.within(bsd.cpu().numpy(), want_b, B_b, name + " bias", what=(n, wk, "bias"))
        assert np.all(wdn[w == 0] == 0), (n, wk)
        pos = csr_positions(plan)
        rv = eb.within(vd.cpu().numpy(), want_w.reshape(-1)[pos], B_w.reshape(-1)[pos], name + " compact", what=(n, wk, "values"))
        eb.within(bsd2.cpu().numpy(), want_b, B_b, name + " compact bias", what=(n, wk, "bias"))
        peak = torch.cuda.max_memory_allocated() + plan.workspace_bytes
        print("large backward weight %d-%s %s: worst err / bound weights %.3g, bias %.3g, values %.3g, peak %.2f GiB, %.1f s" %
              (n, wk, name, r, rb, rv, peak / 2.0 ** 30, time.time() - t0))
        assert peak <= lg.MAX_CASE_BYTES, peak
        REPORT.append("large backward weight worst %-14s %s   weights %.3g  bias %.3g  values %.3g   peak %.2f GiB" %
                      ("%d-%s" % (n, wk), name, r, rb, rv, peak / 2.0 ** 30))
    finally:
        plan.close()
        del td, x
        _release()


# ---- the matrix-core gradients at the largest batch their plans take on a strided shape ------------------------------------
def test_mfma_data_gradient_at_its_largest_batch_and_refused_one_image_past_it(pkg, synth, dev):
    """1 -> 1 channels, 3x3, stride 2 on 256 x 256 at 32767 images: N*H*W = 2^31 - 2^16, the kernel's flattened pixel index
    at the top of its 31 bits, bottom_diff 8 GiB.  A plan for 32768 images refuses (dgm_plan) and writes nothing."""
    t0 = time.time()
    layer, n = lg.MFMA_LAYER, lg.MFMA_MAX_IMAGES
    s = lg.shape(synth, layer, n)
    oh, ow = synth.out_hw(s)
    w = lg.pattern(synth, layer)[1]
    ref = lg.bwd_reference(synth, layer)
    tdbase, want, B = torch.from_numpy(lg.bwd_pattern(synth, layer)[0]).to(dev), torch.tensor(ref[0], device=dev), torch.tensor(ref[1], device=dev)
    lg.require_memory(torch, pytest, lg.need_bytes(n * s.M * oh * ow, n * s.C * s.H * s.W), (layer, n, "BWD_MFMA"))
    torch.cuda.reset_peak_memory_stats()
    td = torch.empty((n, s.M, oh, ow), device=dev, dtype=torch.float32)
    lg.fill_pattern(torch, td, tdbase)
    buf, bdiff = lg.guarded(torch, dev, (n, s.C, s.H, s.W))
    past = pkg.Plan(pkg.ConvDesc.from_shape(lg.shape(synth, layer, n + 1)), backward_kernel=pkg.BWD_MFMA)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s), backward_kernel=pkg.BWD_MFMA)
    try:
        past.weight_align(w)
        with pytest.raises(pkg.EscoinError, match=r"\(-1\): " + re.escape(lg.DGM_REFUSAL)):
            past.backward(td, bottom_diff=bdiff)
        torch.cuda.synchronize()
        assert lg.all_sentinel(torch, bdiff) and lg.guards_intact(buf), "a refused backward wrote to bottom_diff"
        plan.weight_align(w)
        plan.backward(td, bottom_diff=bdiff)
        torch.cuda.synchronize()
        assert plan.stat("bwd_data_kernel") == pkg.BWD_MFMA, plan.stat("bwd_data_kernel")
        ratio, bad = lg.worst_ratio(torch, bdiff, want, B)
        peak = torch.cuda.max_memory_allocated() + plan.workspace_bytes
        print("large backward data %s-%d BWD_MFMA: worst err / bound %.3g, first violation %s, peak %.2f GiB, %.1f s" %
              (layer, n, ratio, bad, peak / 2.0 ** 30, time.time() - t0))
        assert lg.guards_intact(buf), "a guard zone around bottom_diff was written"
        assert bad is None and ratio <= 1.0, "MFMA data gradient: element %s is off by %.3g x its bound" % (bad, ratio)
        assert peak <= lg.MAX_CASE_BYTES, peak
        REPORT.append("large backward data worst %s-%d bwd_data_kernel 5   %.3g   peak %.2f GiB" % (layer, n, ratio, peak / 2.0 ** 30))
    finally:
        plan.close()
        past.close()
        del td, bdiff, buf
        _release()


def test_dense_weight_gradient_at_the_mfma_data_gradient_s_largest_batch(pkg, synth, dev):
    """escoin_dense_wgrad on the same layer and batch (an 8 GiB bottom; its own limit, N*OH*OW below 2^31, lies at
    131071 images of this layer, a bottom of 32 GiB): every element of the 3 x 3 gradient within the bound of the
    reduction's depth -- the plan's span of chunks in one accumulator set, then its splits."""
    t0 = time.time()
    layer, n = lg.MFMA_LAYER, lg.MFMA_MAX_IMAGES
    s = lg.shape(synth, layer, n)
    oh, ow = synth.out_hw(s)
    w, _, base, _, _ = _layer_on_device(synth, dev, layer)
    tdbase = torch.from_numpy(lg.bwd_pattern(synth, layer)[0]).to(dev)
    lg.require_memory(torch, pytest, lg.need_bytes(n * s.M * oh * ow, n * s.C * s.H * s.W), (layer, n, "dense_wgrad"))
    torch.cuda.reset_peak_memory_stats()
    td = torch.empty((n, s.M, oh, ow), device=dev, dtype=torch.float32)
    lg.fill_pattern(torch, td, tdbase)
    x = torch.empty((n, s.C, s.H, s.W), device=dev, dtype=torch.float32)
    lg.fill_pattern(torch, x, base)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
    try:
        plan.weight_align(w)
        got = plan.dense_wgrad(td, x)
        torch.cuda.synchronize()
        splits = plan.stat("dwg_splits")
        chunks = -(-n * oh * ow // 1024)
        span = -(-chunks // splits)
        assert splits >= 1, splits
        (want_w, _), (B_w, _) = lg.weight_reference(synth, n, layer, chunk_span=span)
        r = eb.within(got.cpu().numpy(), want_w, B_w, "dense_wgrad", what=(layer, n, "splits", splits, "span", span))
        peak = torch.cuda.max_memory_allocated() + plan.workspace_bytes
        print("large dense_wgrad %s-%d splits %d span %d: worst err / bound %.3g, peak %.2f GiB, %.1f s" %
              (layer, n, splits, span, r, peak / 2.0 ** 30, time.time() - t0))
        assert peak <= lg.MAX_CASE_BYTES, peak
        REPORT.append("large dense_wgrad worst %s-%d splits %d span %d   %.3g   peak %.2f GiB" % (layer, n, splits, span, r, peak / 2.0 ** 30))
    finally:
        plan.close()
        del td, x
        _release()


# ---- the refusals, on really allocated blobs ------------------------------------------------------------------------------
def _refused(pkg, synth, dev, layer, n, kernel, msg, weights=None, check=None, **options):
    """A forward of n images of `layer` under `kernel` fails with ESCOIN_EINVAL and `msg` and leaves the whole top, and the
    guard zones around it, at the sentinel."""
    s = lg.shape(synth, layer, n)
    oh, ow = synth.out_hw(s)
    per_in, per_out = s.C * s.H * s.W, s.M * oh * ow
    w, bd, base, _, _ = _layer_on_device(synth, dev, layer)
    lg.require_memory(torch, pytest, lg.need_bytes(n * per_in, n * per_out), (layer, n, kernel))
    x = torch.empty((n, s.C, s.H, s.W), device=dev, dtype=torch.float32)
    lg.fill_pattern(torch, x, base)
    buf, top = lg.guarded(torch, dev, (n, s.M, oh, ow))
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=True), kernel=getattr(pkg, "KERNEL_" + kernel), **options)
    try:
        plan.weight_align(w if weights is None else weights)
        if check is not None:
            check(plan)
        with pytest.raises(pkg.EscoinError, match=r"\(-1\): " + re.escape(msg)):
            plan.forward(x, bd, top)
        torch.cuda.synchronize()
        assert lg.all_sentinel(torch, top) and lg.guards_intact(buf), (layer, n, kernel, "a refused call wrote to the top")
        return plan.stat("dense_variant")
    finally:
        plan.close()
        del x, top, buf
        _release()


def test_the_dense_kernel_refuses_a_bottom_of_exactly_4_gib(pkg, synth, dev):
    layer, n, _, msg = REFUSALS[0]
    assert msg == DENSE_RANGE
    _refused(pkg, synth, dev, layer, n, "DENSE", msg)


@pytest.mark.parametrize("kernel", ["AUTO", "TILED"])
def test_a_strided_pointwise_layer_refuses_a_top_of_2_gib(pkg, synth, dev, kernel):
    layer, n, _, msg = REFUSALS[1]
    assert msg == STRIDED_TOP

    def tiled(plan):
        assert plan.stat("kernel_choice") in (pkg.KERNEL_JIT, pkg.KERNEL_TILED) and "dense" not in plan.kernel_name, plan.kernel_name
    _refused(pkg, synth, dev, layer, n, kernel, msg, check=tiled)


def test_the_generic_kernel_refuses_65536_images(pkg, synth, dev):
    layer, n, _, msg = REFUSALS[2]
    assert msg == GENERIC_GRID
    _refused(pkg, synth, dev, layer, n, "GENERIC", msg, weights=np.full((1, 1, 1, 1), 0.75, np.float32))


def test_a_refused_plan_of_dense_and_sparse_groups_has_launched_neither_half(pkg, synth, dev):
    """The strided pointwise layer in two conv groups, the first one dense: the plan runs its first group on the MFMA kernel
    and its second on the tiled kernels, whose launch refuses a top of 2 GiB.  The refusal comes before the dense half's
    launch: the top is untouched and the dense kernel has recorded no launch."""
    _, n, _, msg = REFUSALS[1]
    s = lg.shape(synth, "sp_mixed", lg.BASE)
    assert n * lg.top_image_elems(synth, "sp_mixed") * 4 == 2 ** 31
    w = lg.pattern(synth, "sp_mixed")[1].copy()
    mg = s.M // 2
    w[:mg] = np.where(w[:mg] != 0, w[:mg], np.float32(0.5))      # group 0: every weight a nonzero

    def mixed(plan):
        assert plan.kernel_name.endswith(" + escoin_dense_mfma_kernel") and plan.stat("kernel_choice") in (pkg.KERNEL_JIT, pkg.KERNEL_TILED), plan.kernel_name
    assert _refused(pkg, synth, dev, "sp_mixed", n, "AUTO", msg, weights=w, check=mixed) == 0, "the dense half was launched"


# ---- option "deconv": the top and the plan's own scratch T' past 2 and 4 GiB -------------------------------------------------
def _dc_on_device(synth, dev):
    if "dc" not in _ON_DEVICE:
        _, w, b, base, _, tdbase, _ = lg.dc_pattern()
        want, B = lg.dc_reference(synth)
        bwant, bB = lg.dc_bwd_reference(synth)
        up = lambda a: torch.tensor(a, device=dev)  # noqa: E731
        _ON_DEVICE["dc"] = (w, up(b), up(base), up(want), up(B), up(tdbase), up(bwant), up(bB))
    return _ON_DEVICE["dc"]


def _dc_plan(pkg, n, kernel, relu):
    import d2s_common as dc
    opts = {} if kernel == "AUTO" else dict(kernel=getattr(pkg, "KERNEL_" + kernel))
    return pkg.Plan(dc.desc(pkg, lg.dc_shape(n), True, relu), deconv=1, **opts)


@pytest.mark.parametrize("c", lg.DC_FORWARD, ids=[lg.dc_case_id(c) for c in lg.DC_FORWARD])
def test_deconv_forward_every_element_of_a_large_top_with_bias_and_relu(pkg, synth, dev, c):
    """The top just under, at and (16385 images) past 2^31 / 2^32 bytes with T', the plan's own scratch, past them as well:
    every top element within d2s_common.forward_bound of the 28 pattern images, the guard zones intact, the images past the
    call's at the sentinel.  An inner GENERIC that refuses the size at its launch is recorded and must leave the top
    untouched; under AUTO every size runs."""
    import d2s_common as dc
    t0 = time.time()
    s = lg.dc_shape(c.plan_n)
    w, bd, base, want, B = _dc_on_device(synth, dev)[:5]
    scratch = 4 * c.plan_n * lg.DC_T_IMAGE
    need = lg.need_bytes(c.n * s.C * s.H * s.W, c.plan_n * lg.DC_TOP_IMAGE)
    assert need + scratch <= lg.MAX_CASE_BYTES, (need, scratch)
    lg.require_memory(torch, pytest, need + scratch, lg.dc_case_id(c))
    torch.cuda.reset_peak_memory_stats()
    x = torch.empty((c.n, s.C, s.H, s.W), device=dev, dtype=torch.float32)
    lg.fill_pattern(torch, x, base)
    buf, top = lg.guarded(torch, dev, (c.plan_n, s.M) + dc.out_hw(s))
    plan = _dc_plan(pkg, c.plan_n, c.kernel, True)
    try:
        plan.weight_align(w)
        name = plan.kernel_name
        assert plan.stat("deconv") == 1 and plan.stat("deconv_scratch_bytes") == scratch and name.endswith(" + escoin_d2s_unpack_kernel"), name
        assert c.kernel == "AUTO" or ("generic" in name and plan.stat("kernel_choice") == pkg.KERNEL_GENERIC), name
        try:
            plan.forward(x, bd, top[:c.n])
        except pkg.EscoinError as e:
            torch.cuda.synchronize()
            assert c.kernel != "AUTO" and "(-1)" in str(e), (lg.dc_case_id(c), str(e))
            assert lg.all_sentinel(torch, top) and lg.guards_intact(buf), (lg.dc_case_id(c), "a refused call wrote to the top")
            print("large forward %-24s %s: the inner kernel refuses the size: %s" % (lg.dc_case_id(c), name, e))
            REPORT.append("large forward worst %-40s %-48s refused at the launch: %s" % (lg.dc_case_id(c), name[:48], str(e).split("): ")[-1]))
            return
        torch.cuda.synchronize()
        ratio, bad = lg.worst_ratio(torch, top[:c.n], want, B)
        peak = torch.cuda.max_memory_allocated() + plan.workspace_bytes
        print("large forward %-24s %s | %s: scratch %.2f GiB, worst err / bound %.3g, first violation %s, peak %.2f GiB, %.1f s" %
              (lg.dc_case_id(c), name, plan.tiling_info, scratch / 2.0 ** 30, ratio, bad, peak / 2.0 ** 30, time.time() - t0))
        assert lg.guards_intact(buf), (lg.dc_case_id(c), "a guard zone around the top was written")
        if c.plan_n > c.n:
            assert lg.all_sentinel(torch, top[c.n:]), (lg.dc_case_id(c), "images past the call's were written")
        assert bad is None and ratio <= 1.0, "%s via %s: element %s is off by %.3g x its bound" % (lg.dc_case_id(c), name, bad, ratio)
        assert peak <= lg.MAX_CASE_BYTES, peak
        REPORT.append("large forward worst %-40s %-48s %-16s %.3g   peak %.2f GiB" % (lg.dc_case_id(c), name[:48], "", ratio, peak / 2.0 ** 30))
    finally:
        plan.close()
        del x, top, buf
        _release()


def test_deconv_backward_of_a_large_top_diff(pkg, synth, dev):
    """top_diff past 2^31 bytes, packed into a G' of 2.26 GiB: bottom_diff of every image within
    d2s_common.backward_bound; the compact weight gradient and the bias gradient of the whole batch against the sum of the
    28 pattern images' gradients, bounded by the depth of the inner plan's two-stage reduction
    (large_common.dc_weight_reference)."""
    t0 = time.time()
    n = lg.DC_BACKWARD_N
    s = lg.dc_shape(n)
    w, _, base, _, _, tdbase, want, B = _dc_on_device(synth, dev)
    (want_w, want_b), (B_w, B_b) = lg.dc_weight_reference(n)
    scratch = 4 * n * lg.DC_T_IMAGE
    need = lg.need_bytes(n * lg.DC_TOP_IMAGE, n * s.C * s.H * s.W, n * s.C * s.H * s.W)
    lg.require_memory(torch, pytest, need + scratch, ("dc_top", n, "backward"))
    torch.cuda.reset_peak_memory_stats()
    td = torch.empty((n, s.M, 32, 32), device=dev, dtype=torch.float32)
    lg.fill_pattern(torch, td, tdbase)
    x = torch.empty((n, s.C, s.H, s.W), device=dev, dtype=torch.float32)
    lg.fill_pattern(torch, x, base)
    buf, bdiff = lg.guarded(torch, dev, (n, s.C, s.H, s.W))
    plan = _dc_plan(pkg, n, "AUTO", False)
    try:
        plan.weight_align(w)
        _, vd, bsd = plan.backward(td, bottom=x, bottom_diff=bdiff, values_diff=True, bias_diff=True)
        torch.cuda.synchronize()
        kernels = (plan.stat("bwd_data_kernel"), plan.stat("wgrad_kernel"))
        ratio, bad = lg.worst_ratio(torch, bdiff, want, B)
        pos = np.flatnonzero(w.reshape(-1))
        name = "deconv kernels %d / %d" % kernels
        rv = eb.within(vd.cpu().numpy(), want_w.reshape(-1)[pos], B_w.reshape(-1)[pos], name + " compact", what=(n, "values"))
        rb = eb.within(bsd.cpu().numpy(), want_b, B_b, name + " bias", what=(n, "bias"))
        peak = torch.cuda.max_memory_allocated() + plan.workspace_bytes
        print("large backward dc_top-%d %s, %s: worst err / bound data %.3g (first violation %s), values %.3g, bias %.3g, peak %.2f GiB, %.1f s" %
              (n, plan.kernel_name, name, ratio, bad, rv, rb, peak / 2.0 ** 30, time.time() - t0))
        assert lg.guards_intact(buf), "a guard zone around bottom_diff was written"
        assert bad is None and ratio <= 1.0, "deconv data gradient: element %s is off by %.3g x its bound" % (bad, ratio)
        assert peak <= lg.MAX_CASE_BYTES, peak
        REPORT.append("large backward worst dc_top-%d %s   data %.3g  values %.3g  bias %.3g   peak %.2f GiB" % (n, name, ratio, rv, rb, peak / 2.0 ** 30))
    finally:
        plan.close()
        del td, x, bdiff, buf
        _release()


def test_deconv_refuses_a_top_of_2_31_elements_at_the_align_and_leaves_nothing_behind(pkg, synth, dev):
    """From a descriptor alone: 32768 images of DC_LAYER are a top of exactly 2^31 elements, which d2s_plan refuses by name
    before anything is allocated; the plan stays unaligned, without a scratch, and the device's free memory is what it was."""
    w = lg.dc_pattern()[1]
    _release()
    plan = _dc_plan(pkg, lg.DC_REFUSED_N, "AUTO", True)
    free0 = torch.cuda.mem_get_info()[0]
    try:
        with pytest.raises(pkg.EscoinError, match=r"\(-1\): " + re.escape(lg.DC_TOP_REFUSAL)):
            plan.weight_align(w)
        torch.cuda.synchronize()
        assert plan.stat("deconv") == 0 and plan.stat("deconv_scratch_bytes") == 0
        assert torch.cuda.mem_get_info()[0] >= free0 - (64 << 20), (free0, torch.cuda.mem_get_info()[0])      # (a T' would be 9 GiB)
        with pytest.raises(pkg.EscoinError):
            plan.forward(torch.zeros((1, 16, 16, 16), device=dev), None)
    finally:
        plan.close()
