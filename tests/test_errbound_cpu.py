"""The per-element error bound of errbound.py without a GPU: the checker checks itself (three corruptions that the suite's
max-norm passes must exceed the bound), the CPU mode runs within it on skewed inputs, and two exact metamorphic checks."""
import numpy as np
import pytest

import errbound as eb
from conftest import rel_err
from wgrad_common import csr_positions, make_shape, seeded

# (N, C, H, W, M, K), kwargs of synth.shape
LAYERS = [
    ((3, 24, 9, 11, 20, 3), dict(pad=1, sparsity=0.9)),
    ((2, 256, 7, 7, 40, 3), dict(pad=1, sparsity=0.9)),
    ((3, 96, 7, 9, 33, 1), dict(sparsity=0.95)),
    ((2, 16, 12, 10, 12, 5), dict(pad=2, group=2, sparsity=0.8)),
    ((2, 512, 5, 5, 24, 3), dict(pad=1, sparsity=0.3)),
]
DISTS = ("uniform", "filters_tail")
PARAMS = [(i, d) for i in range(len(LAYERS)) for d in DISTS]
IDS = ["layer%d-%s" % p for p in PARAMS]
TOL = 1e-4      # the suite's max-norm tolerance


def _layer(synth, i, dist, skewed=True):
    dims, kw = LAYERS[i]
    s = synth.shape("eb%d" % i, *dims, **kw)
    w, x, b = synth.pruned_weights(s, 40 + i, dist=dist), synth.activations(s, 50 + i), synth.bias_vector(s, 60 + i)
    return s, (eb.skew(s, w, x, b, 70 + i) if skewed else None), (w, x, b)


def _geom(oracle, s):
    return oracle.geom(s.C, s.H, s.W, s.M, s.KH, s.KW, s.pad_h, s.pad_w, s.stride_h, s.stride_w, s.dil_h, s.dil_w, s.group)


@pytest.mark.parametrize("i,dist", PARAMS, ids=IDS)
def test_the_checker_passes_the_oracle_and_fails_three_corruptions_that_rel_err_passes(oracle, synth, i, dist):
    """The gap this module closes, on record: a dropped bias, a 2^-30 leak from a high-scale neighbour row and two swapped
    images, each on one low-scale channel, pass rel_err <= 1e-4 and exceed the per-element bound."""
    s, sk, _ = _layer(synth, i, dist)
    out = oracle.conv_forward(_geom(oracle, s), sk.x, sk.w, sk.b, gate=False)
    want, B = eb.forward_bound(s, sk.w, sk.x, sk.b)
    ratio = eb.within(out, want, B, "the fp32 oracle", sk.row_exp, what=s.name)
    # a low-scale channel that has nonzeros and a bias (filters_tail leaves some rows empty) and a high-scale neighbour
    m, src = eb.corruption_target(want, sk.w, sk.b)
    mag = eb.low_channels(want)[1]
    assert mag[src] >= 2.0 ** 20 * mag[m], (mag[m], mag[src])
    bad = {"bias dropped": eb.drop_bias(out, sk.b, m), "2^-30 of row %d" % src: eb.leak_from(out, m, src),
           "images 0 and 1 swapped": eb.swap_images(out, m)}
    print("%s %s: oracle at %.3g of the bound; channel %d (2^%d)" % (s.name, dist, ratio, m, sk.row_exp[m]))
    for what, c in bad.items():
        r, idx = eb.check(c, want, B)
        print("    %-24s rel_err %.3g   err / bound %.3g at %s" % (what, rel_err(c, want), r, idx))
        assert rel_err(c, want) <= TOL, (what, "the max-norm was expected to pass this")
        assert r > 1.0 and idx[1] == m, (what, r, idx)


@pytest.mark.parametrize("i,dist", PARAMS, ids=IDS)
def test_cpu_mode_forward_float_and_double_within_the_bound(pkg, synth, i, dist):
    s, sk, _ = _layer(synth, i, dist)
    for dt in (np.float32, np.float64):
        for relu in (False, True):
            plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu))
            plan.weight_align_cpu(sk.w.astype(dt))
            got = plan.forward_cpu(sk.x.astype(dt), sk.b.astype(dt), n_threads=3)
            plan.close()
            want, B = eb.forward_bound(s, sk.w, sk.x, sk.b, relu=relu, f64=dt == np.float64)
            eb.within(got, want, B, "forward_cpu %s" % np.dtype(dt).name, sk.row_exp, what=(s.name, dist, relu))


@pytest.mark.parametrize("name", ["straddle3x3", "small7x7g2", "pointwise", "stride2"])
def test_cpu_mode_backward_dense_and_compact_within_the_bound(pkg, synth, name):
    s = make_shape(synth, name)
    w, x, b = synth.pruned_weights(s, 81), synth.activations(s, 82), synth.bias_vector(s, 83)
    td = seeded((s.N, s.M) + synth.out_hw(s), 84)
    sk = eb.skew(s, w, x, b, 85, top_diff=td)
    for dt in (np.float32, np.float64):
        for relu in (False, True):
            plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu))
            plan.weight_align_cpu(sk.w.astype(dt))
            xs, bs, tds = sk.x.astype(dt), sk.b.astype(dt), sk.top_diff.astype(dt)
            top = plan.forward_cpu(xs, bs) if relu else None
            bd, wd, bsd = plan.backward_cpu(tds, bottom=xs, top=top, weight_diff=True, bias_diff=True)
            _, vd, _ = plan.backward_cpu(tds, bottom=xs, top=top, bottom_diff=None, values_diff=True)
            pos = csr_positions(plan)
            plan.close()
            want, Bs = eb.backward_bound(s, sk.w, sk.x, sk.b, sk.top_diff, top, f64=dt == np.float64)
            what = (name, np.dtype(dt).name, relu)
            eb.within(bd, want[0], Bs[0], "backward_cpu bottom_diff", sk.chan_exp, what=what)
            eb.within(wd, want[1], Bs[1], "backward_cpu weight_diff", sk.td_row_exp, axis=0, what=what)
            eb.within(bsd, want[2], Bs[2], "backward_cpu bias_diff", sk.td_row_exp, axis=0, what=what)
            eb.within(vd, want[1].reshape(-1)[pos], Bs[1].reshape(-1)[pos], "backward_values_cpu values_diff", what=what)
            assert np.all(wd[sk.w == 0] == 0)


@pytest.mark.parametrize("i,dist", PARAMS, ids=IDS)
def test_row_and_image_scaling_are_exact_in_cpu_mode(pkg, synth, i, dist):
    """Zero tolerance, no reference: a plan whose rows (and bias) were scaled by 2^e_m gives 2^e_m x the unscaled plan's
    output bit for bit, and with no bias an image scaled by 2^g_n gives its output scaled by 2^g_n."""
    s, _, (w, x, b) = _layer(synth, i, dist, skewed=False)
    sk = eb.skew(s, w, x, b, 70 + i)
    for dt in (np.float32, np.float64):
        outs = {}
        for key, ww, bb in (("plain", w, b), ("rows", sk.w, sk.b)):
            plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
            plan.weight_align_cpu(ww.astype(dt))
            outs[key] = plan.forward_cpu(x.astype(dt), bb.astype(dt))
            if key == "plain":
                outs["nobias"] = plan.forward_cpu(x.astype(dt), None)
                xi = (x * np.ldexp(1.0, sk.img_exp).astype(np.float32)[:, None, None, None]).astype(dt)
                outs["images"] = plan.forward_cpu(xi, None)
            plan.close()
        rows = np.ldexp(1.0, sk.row_exp).astype(dt)[None, :, None, None]
        imgs = np.ldexp(1.0, sk.img_exp).astype(dt)[:, None, None, None]
        assert (outs["plain"] * rows).tobytes() == outs["rows"].tobytes(), (s.name, dt)
        assert (outs["nobias"] * imgs).tobytes() == outs["images"].tobytes(), (s.name, dt)


def test_skew_is_seeded_exact_and_spans_the_row_range(synth):
    s = synth.shape("sk", 3, 8, 5, 5, 12, 3, pad=1, sparsity=0.5)
    w, x, b = synth.pruned_weights(s, 1), synth.activations(s, 2), synth.bias_vector(s, 3)
    a, c = eb.skew(s, w, x, b, 9, top_diff=x[:, :1].repeat(12, 1)[:, :, :5, :5]), eb.skew(s, w, x, b, 9)
    assert a.w.tobytes() == c.w.tobytes() and a.x.tobytes() == c.x.tobytes() and a.b.tobytes() == c.b.tobytes()
    assert a.w.dtype == np.float32 and set(a.row_exp) == set(eb.ROW_EXPONENTS)
    assert np.abs(a.chan_exp).max() <= 8 and np.abs(a.img_exp).max() <= 10
    # exact powers of two: dividing the scales out again gives the inputs back bit for bit
    back = a.w / np.ldexp(1.0, a.row_exp).astype(np.float32)[:, None, None, None]
    assert back.tobytes() == w.tobytes()
    assert np.all(np.abs(a.x[a.x != 0]) >= 2.0 ** -100) and np.all(np.isfinite(a.x))
    assert eb.check(np.array([1.0, np.nan]), np.array([1.0, 1.0]), np.array([1.0, 1.0])) == (np.inf, (1,))
