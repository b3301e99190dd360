"""Every layout class of the tiled kernels and every instantiation and store path of the dense MFMA kernel
(layout_cases.py) on the MI355X, every output element against the float64 reference within errbound.py's derived bound
on skewed inputs: the code that picks the channel, quad and image an accumulator is stored to is the layout-specific part
of a kernel, and the max-norm on uniformly scaled inputs does not see one slot stored to the wrong place
(test_errbound_layouts_cpu.py has that on record for every row).  Plus the exact metamorphic check on every row and the
data gradient of every BODY row, whose transposed plan (M' = 8 .. 64 output channels) takes layouts of its own.

Every case asserts the kernel that ran -- the dense kernel by stat "dense_variant".  The worst err / bound per kernel
name and per dense variant is printed when the module ends (pytest -s; profiles/errbound.md)."""
import numpy as np
import pytest

import errbound as eb
import layout_cases as lc
from test_body_variant_gpu import _tiling_or_skip
from test_errbound_gpu import ALL4, DIL, ON_OFF, STR2, _expect, _forward_cases, _layer, _ref, _up
from wgrad_common import seeded

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

BODY_IDS = [r.name for r in lc.BODY]
DENSE_IDS = [r.name for r in lc.DENSE]
WORST = {}


@pytest.fixture(scope="module")
def dev(pkg):
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        pytest.fail("no HIP device visible (these tests run on the MI355X)")
    yield torch.device("cuda:0")
    for k in sorted(WORST):
        print("errbound layouts worst %-48s %.3g" % (k, WORST[k]))


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dense_want(row, s, n_images, **aligned):
    """The dense_variant a launch of n_images must report: launch_dense's rule for this device, which on the device the
    table is named for gives a whole batch what the table says."""
    v = lc.dense_variant(s, n_images, _n_cu(), **aligned)
    if _n_cu() == lc.N_CU and n_images == s.N and not aligned:
        assert v == row.expect_variant, (row.name, v)
    return v


# ---- forward: the tiled kernels -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kn", ["AUTO", "TILED"])
@pytest.mark.parametrize("row", lc.BODY, ids=BODY_IDS)
def test_forward_every_body_layout_bias_relu_and_a_partial_batch(pkg, synth, dev, row, kn):
    s, sk, _ = lc.layer(synth, row)
    kernel = getattr(pkg, "KERNEL_" + kn)
    check_name = (lambda n: "jit" in n or pytest.fail(n)) if kn == "AUTO" else None
    for plan in _forward_cases(pkg, dev, s, sk, kernel, ALL4, partial=s.N // 2, check_name=check_name, worst=WORST,
                               tiling_batch=lc.TILING_BATCH, **row.options):
        info = plan.tiling_info
        print("    tiling: %s" % info)
        if kn == "AUTO":
            _tiling_or_skip(torch, info, row.expect)
            assert plan.stat("body_variant") == row.variant, info
        else:
            assert plan.stat("kernel_choice") == pkg.KERNEL_TILED and info.startswith("stream "), (plan.kernel_name, info)


# ---- forward: the dense MFMA kernel ---------------------------------------------------------------------------------------
def _dense_within(got, want, B, sk, variant, what):
    return eb.within(got.cpu().numpy(), want, B, "dense_variant %d" % variant, sk.row_exp, what=what, worst=WORST)


@pytest.mark.parametrize("row", lc.DENSE, ids=DENSE_IDS)
def test_forward_every_dense_variant_bias_relu_and_a_partial_batch(pkg, synth, dev, row):
    """The four (bias, ReLU) combinations and a partial batch, every launch reporting the variant the table names; the
    stream-K rows three times in a row (a kernel re-arms the flags between launches) and with N // 2 + 3 images, which
    cuts the runs elsewhere."""
    s, sk, _ = lc.layer(synth, row)
    split = row.name.startswith("sk_")
    xd, bd = _up(sk.x, dev), _up(sk.b, dev)
    partial = s.N // 2 + (3 if split else 0)
    for relu in (False, True):
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu), kernel=pkg.KERNEL_DENSE)
        plan.weight_align(sk.w)
        _expect(pkg, pkg.KERNEL_DENSE, plan.kernel_name)
        assert plan.stat("dense_variant") == 0      # no launch yet
        for bias in (False, True):
            want, B = _ref(s, sk, bias, relu)
            for rep in range(3 if split else 1):
                got = plan.forward(xd, bd if bias else None)
                torch.cuda.synchronize()
                v = plan.stat("dense_variant")
                assert v == _dense_want(row, s, s.N) and plan.stat("streamk") == v // 16 and plan.stat("streamk_gave_up") == 0, (row.name, v, rep)
                r = _dense_within(got, want, B, sk, v, (s.name, "bias", bias, "relu", relu, "launch", rep))
                print("errbound forward dense_variant %-2d %-8s bias=%d relu=%d launch %d: %.3g" % (v, s.name, bias, relu, rep, r))
        top = torch.full_like(got, -7.5)
        plan.forward(xd[:partial], bd, top[:partial])
        torch.cuda.synchronize()
        v = plan.stat("dense_variant")
        assert v == _dense_want(row, s, partial) and plan.stat("streamk_gave_up") == 0, (row.name, v, partial)
        r = _dense_within(top[:partial], want[:partial], B[:partial], sk, v, (s.name, "first images", partial))
        print("errbound forward dense_variant %-2d %-8s first %d images: %.3g" % (v, s.name, partial, r))
        assert bool((top[partial:] == -7.5).all()), (row.name, "images past the call's were written")
        plan.close()


@pytest.mark.parametrize("option,spec", [("s2b", DIL), ("s2d", STR2)], ids=["s2b", "s2d"])
def test_dense_variant_of_a_plan_that_runs_an_inner_plan_is_the_inner_plan_s(pkg, synth, dev, option, spec):
    """Under "s2b" / "s2d" the forward's kernel is the inner plan's: 0 before the first launch, then what the inner
    geometry takes -- 64-row tiles and a gathered operand on both (20 and 8 output channels, kernels of 3x3 and 2x2 taps),
    so 1 or 9 by the inner top's pixel count (s2b: 7 x 6 = 42 pixels, scalar stores)."""
    s, sk, _ = _layer(synth, spec)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s), kernel=pkg.KERNEL_DENSE, **{option: 1})
    plan.weight_align(sk.w)
    assert plan.stat(option) == 1 and "escoin_dense_mfma_kernel" in plan.kernel_name and plan.stat("dense_variant") == 0
    got = plan.forward(_up(sk.x, dev), _up(sk.b, dev))
    torch.cuda.synchronize()
    v = plan.stat("dense_variant")
    assert v in (1, 9) and (option != "s2b" or v == 1), (plan.kernel_name, v)
    want, B = _ref(s, sk, True, False)
    eb.within(got.cpu().numpy(), want, B, "dense_variant %d" % v, sk.row_exp, what=(s.name, option), worst=WORST)
    plan.close()


MARGIN = 64                                                   # elements on either side of a window
SENTINEL = np.array([0xC0F00000], np.uint32).view(np.int32)[0]      # -7.5


def _window(numel, off, fill, dev):
    """A window of numel floats that starts `off` floats past a 16-byte boundary, MARGIN or more elements inside an
    allocation filled with `fill`: (the allocation, the window, the mask of the elements around the window)."""
    buf = torch.full((2 * MARGIN + 4 + numel,), fill, device=dev)
    assert buf.data_ptr() % 16 == 0
    win = buf[MARGIN + off:MARGIN + off + numel]
    assert win.data_ptr() % 16 == 4 * off
    around = torch.ones(buf.numel(), dtype=torch.bool, device=dev)
    around[MARGIN + off:MARGIN + off + numel] = False
    return buf, win, around


@pytest.mark.parametrize("run,bottom_off,top_off,variant", lc.OFF_BOUNDARY, ids=["dn_pw64-" + o[0] for o in lc.OFF_BOUNDARY])
def test_forward_dense_blobs_off_a_16_byte_boundary(pkg, synth, dev, run, bottom_off, top_off, variant):
    """dn_pw64 with the bottom, then the top, a window 4 bytes off a 16-byte boundary inside a larger allocation: the
    16-byte operand path falls back to the gather, the 16-byte stores to scalar ones.  Around the bottom lie NaNs, of
    which none may reach the top; around the top a sentinel, which must be intact bit for bit."""
    row = next(r for r in lc.DENSE if r.name == "dn_pw64")
    s, sk, _ = lc.layer(synth, row)
    bd = _up(sk.b, dev)
    _, xw, _ = _window(sk.x.size, int(bottom_off), float("nan"), dev)
    xw.copy_(_up(sk.x, dev).reshape(-1))
    xw = xw.view(sk.x.shape)
    assert _dense_want(row, s, s.N, bottom_aligned=not bottom_off, top_aligned=not top_off) == variant
    for bias, relu in ON_OFF:
        want, B = _ref(s, sk, bias, relu)
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu), kernel=pkg.KERNEL_DENSE)
        plan.weight_align(sk.w)
        _expect(pkg, pkg.KERNEL_DENSE, plan.kernel_name)
        tbuf, tw, around = _window(want.size, int(top_off), -7.5, dev)
        plan.forward(xw, bd if bias else None, tw.view(want.shape))
        torch.cuda.synchronize()
        assert plan.stat("dense_variant") == variant, (run, plan.stat("dense_variant"))
        r = _dense_within(tw.view(want.shape), want, B, sk, variant, (s.name, run, "bias", bias, "relu", relu))
        print("errbound forward dense_variant %-2d %-8s %s bias=%d relu=%d: %.3g" % (variant, s.name, run, bias, relu, r))
        assert bool(torch.isfinite(tw).all())
        assert bool((tbuf.view(torch.int32)[around] == int(SENTINEL)).all()), (run, "the top's surroundings were written")
        plan.close()


# ---- the exact metamorphic check on every row: no reference, no tolerance -----------------------------------------------
def _scaling_is_exact(pkg, dev, synth, row, kernel, stats, **opts):
    """test_errbound_gpu.test_row_and_image_scaling_are_exact_on_every_kernel_family on a row: rows (and bias) scaled by
    2^e_m scale the output by 2^e_m bit for bit, and without a bias an image scaled by 2^g_n scales its output by 2^g_n.
    Two plans, the same kernel, tiling and `stats` on both; returns what they were."""
    s, sk, (w, x, b) = lc.layer(synth, row)
    rows = _up(np.ldexp(1.0, sk.row_exp), dev)[None, :, None, None]
    imgs = _up(np.ldexp(1.0, sk.img_exp), dev)[:, None, None, None]
    xd = _up(x, dev)
    outs, ran = {}, []
    for key, ww, bb in (("plain", w, b), ("rows", sk.w, sk.b)):
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s), kernel=kernel, **opts)
        plan.weight_align(ww)
        outs[key] = plan.forward(xd, _up(bb, dev)).clone()
        if key == "plain":
            outs["nobias"] = plan.forward(xd, None).clone()
            outs["images"] = plan.forward((xd * imgs).contiguous(), None).clone()
        torch.cuda.synchronize()
        ran.append((plan.kernel_name, plan.tiling_info) + tuple(plan.stat(k) for k in stats))
        plan.close()
    assert ran[0] == ran[1], ran
    _expect(pkg, kernel, ran[0][0])
    bad = (outs["plain"] * rows != outs["rows"]).nonzero()
    assert bad.numel() == 0, (row.name, ran[0], "rows", bad[0].tolist(), int(sk.row_exp[int(bad[0][1])]))
    bad = (outs["nobias"] * imgs != outs["images"]).nonzero()
    assert bad.numel() == 0, (row.name, ran[0], "images", bad[0].tolist(), int(sk.img_exp[int(bad[0][0])]))
    assert bool(torch.isfinite(outs["rows"]).all()) and float(outs["rows"].abs().max()) > 0
    return ran[0]


@pytest.mark.parametrize("kn", ["AUTO", "TILED"])
@pytest.mark.parametrize("row", lc.BODY, ids=BODY_IDS)
def test_row_and_image_scaling_are_exact_on_every_body_layout(pkg, synth, dev, row, kn):
    name, info, choice, variant = _scaling_is_exact(pkg, dev, synth, row, getattr(pkg, "KERNEL_" + kn), ("kernel_choice", "body_variant"),
                                                    tiling_batch=lc.TILING_BATCH, **row.options)
    if kn == "AUTO":
        assert "jit" in name, name
        _tiling_or_skip(torch, info, row.expect)
        assert variant == row.variant, info
    else:
        assert choice == pkg.KERNEL_TILED and info.startswith("stream "), (name, info)


@pytest.mark.parametrize("row", lc.DENSE, ids=DENSE_IDS)
def test_row_and_image_scaling_are_exact_on_every_dense_variant(pkg, synth, dev, row):
    s = lc.layer(synth, row)[0]
    ran = _scaling_is_exact(pkg, dev, synth, row, pkg.KERNEL_DENSE, ("dense_variant", "streamk_gave_up"))
    assert ran[2:] == (_dense_want(row, s, s.N), 0), ran


# ---- the data gradient of every BODY row ------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", lc.BODY, ids=BODY_IDS)
def test_backward_data_gradient_of_every_body_layout(pkg, synth, dev, row):
    """bottom_diff under backward_kernel AUTO and JIT, per element within errbound.backward_bound, on a skewed top_diff
    masked by one generic-kernel top.  The transposed plan's layout differs from the row's (printed, not asserted: the
    forward plan of the transposed geometry on the same pattern shows it)."""
    s, _, (w, x, b) = lc.layer(synth, row)
    k = sum(map(ord, row.name))
    oh, ow = synth.out_hw(s)
    sk = eb.skew(s, w, x, b, k + 3, top_diff=seeded((s.N, s.M, oh, ow), k + 4))
    xd, bd, tdd = _up(sk.x, dev), _up(sk.b, dev), _up(sk.top_diff, dev)
    desc = pkg.ConvDesc.from_shape(s, fuse_relu=True)
    plan = pkg.Plan(desc, kernel=pkg.KERNEL_GENERIC)      # one top for both plans: one mask, one reference
    plan.weight_align(sk.w)
    topd = plan.forward(xd, bd)
    torch.cuda.synchronize()
    plan.close()
    want, Bs = eb.backward_bound(s, sk.w, sk.x, sk.b, sk.top_diff, topd.cpu().numpy())
    st = synth.shape(row.name + "_t", s.N, s.M, oh, ow, s.C, s.KH, pad=s.KH - 1 - s.pad_h, bias=False)
    wt = np.ascontiguousarray(sk.w[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))
    for kn in ("AUTO", "JIT"):
        kernel = getattr(pkg, "KERNEL_" + kn)
        opts = dict(tiling_batch=lc.TILING_BATCH, **row.options)
        shown = pkg.Plan(pkg.ConvDesc.from_shape(st), kernel=kernel, **opts)
        shown.weight_align(wt)
        print("    transposed geometry, kernel %s: %s | %s" % (kn, shown.kernel_name, shown.tiling_info))
        shown.close()
        plan = pkg.Plan(desc, backward_kernel=kernel, **opts)
        plan.weight_align(sk.w)
        if kn == "JIT" and row.name in lc.BWD_JIT_REFUSALS:
            with pytest.raises(pkg.EscoinError, match=lc.BWD_JIT_REFUSALS[row.name]):
                plan.backward(tdd, top=topd, bottom_diff=True)
            plan.close()
            continue
        bdiff = plan.backward(tdd, top=topd, bottom_diff=True)[0]
        torch.cuda.synchronize()
        ran = plan.stat("bwd_data_kernel")
        # (AUTO: the rules give every row's transposed geometry generated code on the device the table is named for)
        assert ran == pkg.KERNEL_JIT if kn == "JIT" or _n_cu() == lc.N_CU else ran in (pkg.KERNEL_TILED, pkg.KERNEL_JIT, pkg.KERNEL_DENSE,
                                                                                      pkg.KERNEL_GENERIC), (row.name, kn, ran)
        r = eb.within(bdiff.cpu().numpy(), want[0], Bs[0], "bwd_data_kernel %d" % ran, sk.chan_exp, what=(row.name, kn), worst=WORST)
        print("errbound backward data   kernel %d (%s) %-12s: %.3g" % (ran, kn, row.name, r))
        plan.close()
