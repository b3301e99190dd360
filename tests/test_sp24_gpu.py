"""Plan option "sp24" on the MI355X: escoin_dense_sp24_kernel (v_smfmac_f32_32x32x32_bf16) under KERNEL_DENSE on 2:4 weights.

The reference is the float64 convolution of the operands rounded to bf16 in numpy; the bound is errbound.forward_bound's fp32
accumulation bound on the rounded operands, unscaled (the bf16 dense mode's contract).  The worst ratio measured over these
cases is in profiles/sp24_mi355x.md.  On small integers every sum is exact, so the kernel must give the fp32 kernel's bits."""
from collections import namedtuple

import numpy as np
import pytest

import errbound as eb
from dense_bf16_common import bf16_rne
from test_errbound_gpu import _up, dev  # noqa: F401

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

# name, (N, C, H, W, M, K), kwargs of synth.shape, images per call, the fp32 kernel's dense_variant, what the case reaches
Case = namedtuple("Case", "name dims kw n_images variant reaches")
CASES = [
    Case("sp_3x3", (3, 8, 9, 11, 130, 3), dict(pad=1), 2, 2, "K = 72: a second k-step half past K; BM 128, two channel tiles, a row tail; two of three images"),
    Case("sp_pw", (2, 40, 8, 8, 24, 1), {}, 2, 13, "K = 40, K % 16 = 8; BM 64, the direct B path, vector stores"),
    Case("sp_pwg", (3, 40, 5, 5, 48, 1), dict(group=2), 3, 1, "K = 20 < one instruction's k; two conv groups, the gathered B path, scalar stores"),
    Case("sp_s2", (2, 3, 9, 9, 16, 3), dict(pad=1, stride=2), 2, 1, "K = 27: a short last group of 4, stride-2 window origins"),
    Case("sp_dil", (2, 24, 13, 16, 20, 3), dict(pad=2, dil=2), 2, 9, "K = 216: four k-steps, the last past ktab's end"),
    Case("sp_csr", (3, 8, 9, 11, 130, 3), dict(pad=1), 3, 2, "sp_3x3's geometry through set_csr: empty groups, 1-entry groups, explicit zeros"),
]
_LAYERS = {}
WORST = {}


def _csr(s, w, extra=None):
    """set_csr's arguments for the positions where w != 0 or `extra` is set."""
    mg, k = s.M // s.group, w[0].size
    on = (w != 0).reshape(s.M, k) | (False if extra is None else extra.reshape(s.M, k))
    rowptr = np.concatenate([np.concatenate([[0], np.cumsum(on[g * mg:(g + 1) * mg].sum(1))]) for g in range(s.group)])
    return rowptr, np.nonzero(on)[1], w.reshape(s.M, k)[on], [int(on[g * mg:(g + 1) * mg].sum()) for g in range(s.group)]


def _layer(synth, c):
    """(shape, skewed 2:4 inputs, explicit-zero positions or None, want and B of the rounded operands with and without bias)"""
    if c.name not in _LAYERS:
        s = synth.shape(c.name, *c.dims, sparsity=0.0, **c.kw)
        k = sum(map(ord, c.name))
        w, extra = synth.pattern_2of4(synth.pruned_weights(s, k)), None
        if c.name == "sp_csr":
            g = w.reshape(s.M, -1, 4)                       # K = 72: 18 whole groups
            g[0::3, 0::2] = 0                               # empty groups
            g[1::3, :, 0] = 0                               # groups that lose position 0: 1 entry, or none
            g[2::3, 5, 3] = 0
            extra = np.zeros(g.shape, bool)
            extra[0::3, 0, 2] = True                        # explicit zeros: one in an empty group, two in another,
            extra[0::3, 2, 1:3] = True
            extra[1::3, :, 0] = (g[1::3] != 0).sum(2) == 1    # ... and next to a lone entry
        sk = eb.skew(s, w, synth.activations(s, k + 1), synth.bias_vector(s, k + 2), k + 3)
        w_r, x_r = bf16_rne(sk.w), bf16_rne(sk.x)
        _LAYERS[c.name] = (s, sk, extra, {b: eb.forward_bound(s, w_r, x_r, sk.b if b else None) for b in (False, True)})
    return _LAYERS[c.name]


def _plan(pkg, s, w, relu=False, extra=None, **opts):
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu), kernel=pkg.KERNEL_DENSE, **opts)
    if extra is None:
        plan.weight_align(w)
    else:
        plan.set_csr(*_csr(s, w, extra))
    return plan


def _within(got, ref, n, relu, sk, what):
    want, B = ref
    want = np.maximum(want[:n], 0.0) if relu else want[:n]
    r = eb.within(got.cpu().numpy(), want, B[:n], "escoin_dense_sp24_kernel", sk.row_exp, what=what, worst=WORST)
    print("dense_sp24 %s: err / bound %.3g (worst so far %.3g)" % (what, r, WORST["escoin_dense_sp24_kernel"]))


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_bound_stats_exactness_and_the_way_back(pkg, synth, dev, c):
    s, sk, extra, refs = _layer(synth, c)
    xd, n = _up(sk.x, dev), c.n_images
    for bias, relu in ((False, False), (True, True)):
        plan = _plan(pkg, s, sk.w, relu, extra, sp24=1)
        assert (plan.stat("sp24_pattern"), plan.stat("dense_sp24"), plan.stat("dense_variant")) == (1, 0, 0)     # no launch yet
        top = torch.full((s.N,) + refs[bias][0].shape[1:], -7.5, device=dev)
        bd = _up(sk.b, dev) if bias else None
        plan.forward(xd[:n], bd, top[:n])
        torch.cuda.synchronize()
        _within(top[:n], refs[bias], n, relu, sk, (c.name, "bias", bias, "relu", relu))
        assert bool((top[n:] == -7.5).all()), "images past the call's were written"
        assert [plan.stat(k) for k in ("dense_sp24", "dense_variant", "dense_math", "sp24_pattern")] == [1, c.variant + 64, 1, 1]
        plan.set_option("sp24", 0)
        plan.forward(xd[:n], bd)
        assert [plan.stat(k) for k in ("dense_sp24", "dense_variant", "dense_math", "sp24_pattern")] == [0, c.variant, 0, 1]
        plan.close()
    # small integers (weights in [-3, 3] on the pattern, activations in [-4, 4], bias in [-8, 8]: bf16 exactly, every partial sum
    # below 2^24): the fp32 kernel computes the same exact sums, so a wrong lane, k, index field, swizzle or tail changes bits
    rs = np.random.RandomState(sum(map(ord, c.name)))
    x = _up(rs.randint(-4, 5, (n, s.C, s.H, s.W)).astype(np.float32), dev)
    b = _up(rs.randint(-8, 9, s.M).astype(np.float32), dev)
    wi = rs.randint(-3, 4, sk.w.shape).astype(np.float32) * (sk.w != 0)
    plan = _plan(pkg, s, wi, False, extra, sp24=1)
    got = plan.forward(x, b).clone()
    assert plan.stat("dense_sp24") == 1
    plan.set_option("sp24", 0)
    want = plan.forward(x, b)
    assert plan.stat("dense_sp24") == 0
    assert float(want.abs().max()) > 8 and torch.equal(got, want), (c.name, (got != want).nonzero()[:1].tolist())
    plan.set_option("sp24", 1)                                 # ... and back on while the table exists
    assert torch.equal(plan.forward(x, b), got) and plan.stat("dense_sp24") == 1
    plan.close()


def test_a_pattern_that_is_not_2of4_runs_as_without_the_option(pkg, synth, dev):
    s = synth.shape("sp_unstructured", 2, 8, 9, 11, 130, 3, pad=1, sparsity=0.5)
    w, x = synth.pruned_weights(s, 3), _up(synth.activations(s, 4), dev)
    plan, plain = _plan(pkg, s, w, sp24=1), _plan(pkg, s, w)
    assert plan.stat("sp24_pattern") == 0 and plan.stat("device_bytes") == plain.stat("device_bytes")
    assert torch.equal(plan.forward(x, None), plain.forward(x, None))
    assert (plan.stat("dense_sp24"), plan.stat("dense_variant")) == (0, plain.stat("dense_variant"))
    plan.close()
    plain.close()


def test_set_values_and_set_csr_reach_the_next_forward(pkg, synth, dev):
    """No stale value copy and no stale index table: set_values, then set_csr to another 2:4 pattern, on the same plan."""
    c = CASES[0]
    s, sk, _, refs = _layer(synth, c)
    xd = _up(sk.x, dev)
    plan = _plan(pkg, s, (sk.w * np.float32(0.5) + np.float32(1.0)) * (sk.w != 0), sp24=1)
    plan.forward(xd, None)
    plan.set_values(sk.w[sk.w != 0])
    _within(plan.forward(xd, None), refs[False], s.N, False, sk, "after set_values")
    w2 = np.roll(sk.w.reshape(s.M, -1), 1, axis=0).reshape(sk.w.shape)        # every row takes its neighbour's pattern
    plan.set_csr(*_csr(s, w2))
    assert plan.stat("sp24_pattern") == 1
    got = plan.forward(xd, None)
    assert plan.stat("dense_sp24") == 1
    _within(got, eb.forward_bound(s, bf16_rne(w2), bf16_rne(sk.x), None), s.N, False, sk._replace(row_exp=np.roll(sk.row_exp, 1)), "after set_csr")
    plan.close()


def test_inner_plan_of_b2s_runs_the_2of4_kernel(pkg, synth, dev):
    s = synth.shape("sp_ip", 130, 40, 1, 1, 24, 1, sparsity=0.0)
    sk = eb.skew(s, synth.pattern_2of4(synth.pruned_weights(s, 5)), synth.activations(s, 6), synth.bias_vector(s, 7), 8)
    plan = _plan(pkg, s, sk.w, b2s=1, sp24=1)
    assert plan.stat("b2s") == 1 and plan.stat("sp24_pattern") == 1
    got = plan.forward(_up(sk.x, dev), _up(sk.b, dev))
    _within(got, eb.forward_bound(s, bf16_rne(sk.w), bf16_rne(sk.x), sk.b), s.N, False, sk, "b2s inner plan")
    assert plan.stat("dense_sp24") == 1 and plan.stat("dense_variant") >= 64
    plan.close()
