"""Every kernel on the MI355X at the edges of the number formats: subnormal inputs, weights and results and sums next to
the largest finite number, every element within errbound's bound of the float64 reference computed from the rounded
arrays (no kernel flushes: test_fp32_edges_cpu.py proves these inputs put a flushing kernel orders of magnitude outside);
the reach of a non-finite bottom or top_diff element, as a set; the solver rule on special values.

Every case asserts the kernel that ran.  The worst err / bound per family and kind is printed when the module ends
(pytest -s; profiles/errbound.md, "The edges of fp32")."""
import numpy as np
import pytest

import edges_common as ec
import errbound as eb
import layout_cases as lc
import solver_common as sc
from test_b2s_sequence_gpu import LAYER as IP_SPEC
from test_body_variant_gpu import CASES as BODY_CASES
from test_fp32_edges_cpu import finite_specials, masked_top_case
from wgrad_common import csr_positions

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

WORST = {}
S2B_PACK, S2B_UNPACK, S2D_PACK = "escoin_s2b_pack_kernel", "escoin_s2b_unpack_kernel", "escoin_s2d_pack_kernel"
DENSE_NAME = "escoin_dense_mfma_kernel"
B2S_PACK = "escoin_b2s_pack_kernel"


@pytest.fixture(scope="module")
def dev(pkg):
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        pytest.fail("no HIP device visible (these tests run on the MI355X)")
    yield torch.device("cuda:0")
    for k in sorted(WORST):
        print("edges worst %-28s %-9s %.3g" % (k[0], k[1], WORST[k]))


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _up(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _within(got, want, B, family, kind, what):
    r = eb.within(got, want, B, family, what=what)
    WORST[(family, kind)] = max(WORST.get((family, kind), 0.0), r)
    return r


# ---- the families: (id, layer, Plan options -- a string names a constant of the package --, f64, what must have run) -----------
class Family(object):
    def __init__(self, id, layer, f64=False, name=(), exact=None, stats=None, spec=None, **options):
        self.id, self.layer, self.f64, self.name, self.exact, self.stats, self.spec = id, layer, f64, name, exact, stats or {}, spec
        self.options = options

    def plan(self, pkg, s, relu):
        o = {k: getattr(pkg, v) if isinstance(v, str) else v for k, v in self.options.items()}
        return pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu), **o)

    def ran(self, pkg, plan):
        """The kernel under test is the one that ran: substrings of kernel_name (all of them), or the whole name; stats."""
        name = plan.kernel_name
        assert all(t in name for t in self.name) and (self.exact is None or name == self.exact), (self.id, name)
        assert ("f64" in name) == self.f64, (self.id, name)
        for option in ("s2d", "s2b", "b2s", "deconv"):
            assert plan.stat(option) == self.options.get(option, 0), (self.id, option, name)
        for k, v in self.stats.items():
            assert plan.stat(k) == (getattr(pkg, v) if isinstance(v, str) else v), (self.id, k, plan.stat(k), name)

    def __repr__(self):
        return self.id


_CHAIN = min((c for c in BODY_CASES if c[3] == 1), key=lambda c: c[1][0] * c[1][1] * c[1][2] * c[1][3])      # seg7_5
_CHAIN_SPEC = ("chain_" + _CHAIN[0], _CHAIN[1][:6], dict(pad=_CHAIN[1][6], sparsity=_CHAIN[1][7]))

SPARSE = [
    Family("generic_3x3", "L3X3", kernel="KERNEL_GENERIC", name=("generic",)),
    Family("tiled_3x3", "L3X3", kernel="KERNEL_TILED", name=("tiled",)),
    Family("tiled_3x3_tb256", "L3X3", kernel="KERNEL_TILED", tiling_batch=256, name=("tiled",)),
    Family("jit_3x3", "L3X3", kernel="KERNEL_JIT", name=("jit",)),
    Family("jit_3x3_tb256", "L3X3", kernel="KERNEL_JIT", tiling_batch=256, name=("jit",)),
    Family("lowered_sparse", "L3X3", conv_mode="CONV_MODE_LOWERED_SPARSE", exact="escoin_csrmm_kernel"),
    Family("tiled_pointwise", "PW_B", kernel="KERNEL_TILED", tiling_batch=256, name=("tiled",)),
    Family("jit_pointwise", "PW_B", kernel="KERNEL_JIT", tiling_batch=256, name=("jit",)),
    Family("tiled_5x5_groups", "G5X5", kernel="KERNEL_TILED", tiling_batch=256, name=("tiled",)),
    Family("jit_5x5_groups", "G5X5", kernel="KERNEL_JIT", tiling_batch=256, name=("jit",)),
    Family("generic_stride2", "STR2", kernel="KERNEL_GENERIC", name=("generic",)),
    Family("s2d_stride2", "STR2", s2d=1, name=(S2D_PACK,)),
    Family("s2b_jit_dilated", "DIL", kernel="KERNEL_JIT", s2b=1, name=(S2B_PACK, "jit", S2B_UNPACK)),
    Family("chained_body", "CHAIN", spec=_CHAIN_SPEC, tiling_batch=256, name=("jit",), stats=dict(body_variant=1), **_CHAIN[4]),
    Family("double", "L3X3", f64=True, name=("f64",), stats=dict(is_f64=1)),
    # option "b2s" on the sequence suite's inner-product layer: 70 images are two inner images, and 58 of the second one's 64
    # positions are padding
    Family("b2s_jit", "IP", spec=IP_SPEC, b2s=1, kernel="KERNEL_JIT", tiling_batch=4096, name=(B2S_PACK, "jit"),
           stats=dict(kernel_choice="KERNEL_JIT")),
    Family("b2s_generic", "IP", spec=IP_SPEC, b2s=1, kernel="KERNEL_GENERIC", name=(B2S_PACK, "generic")),
]
DENSE = [
    Family("dense_3x3", "L3X3", kernel="KERNEL_DENSE", exact=DENSE_NAME),
    Family("lowered_gemm", "L3X3", conv_mode="CONV_MODE_LOWERED_GEMM", exact=DENSE_NAME),
    Family("dense_stride2", "STR2", kernel="KERNEL_DENSE", exact=DENSE_NAME),
    Family("s2b_dense_dilated", "DIL", kernel="KERNEL_DENSE", s2b=1, name=(S2B_PACK, DENSE_NAME, S2B_UNPACK)),
    Family("b2s_dense", "IP", spec=IP_SPEC, b2s=1, kernel="KERNEL_DENSE", name=(B2S_PACK, DENSE_NAME)),
]
MIXED = Family("mixed_groups", "MIXED", dense_threshold_pct=30, tiling_batch=256, name=(" + ", DENSE_NAME))
FORWARD = SPARSE + DENSE + [MIXED]
IDS = lambda fams: [f.id for f in fams]  # noqa: E731


# ---- forward: four kinds x (bias, ReLU) ------------------------------------------------------------------------------------------
def _forward_kind(pkg, synth, dev, fam, kind, combos=ec.ALL4):
    s, e = ec.edge(synth, fam.layer, kind, f64=fam.f64, spec=fam.spec)
    xd, bd = _up(e.x, dev), _up(e.b, dev)
    for relu in sorted(set(r for _, r in combos)):
        plan = fam.plan(pkg, s, relu)
        plan.weight_align(e.w)
        for bias in sorted(set(b for b, r in combos if r == relu)):
            got = plan.forward(xd, bd if bias else None)
            torch.cuda.synchronize()
            fam.ran(pkg, plan)
            got = got.cpu().numpy()
            want, B = ec.forward_ref(synth, fam.layer, kind, bias, relu, fam.f64, spec=fam.spec)
            r = _within(got, want, B, fam.id, kind, (fam.id, kind, "bias", bias, "relu", relu, plan.kernel_name))
            print("edges forward %-20s %-8s bias=%d relu=%d %s: %.3g" % (fam.id, kind, bias, relu, plan.kernel_name, r))
            if kind == "near_max":
                assert np.all(np.isfinite(got)), (fam.id, "a sum bounded by 2^127 overflowed")
        yield plan
        plan.close()


@pytest.mark.parametrize("kind", ec.KINDS)
@pytest.mark.parametrize("fam", FORWARD, ids=IDS(FORWARD))
def test_forward_at_the_edges_within_the_bound(pkg, synth, dev, fam, kind):
    for _ in _forward_kind(pkg, synth, dev, fam, kind):
        pass


@pytest.mark.parametrize("kind", ["sub_out", "near_max"])
def test_forward_stream_k_fixup_adds_subnormal_partials_and_partials_near_the_top(pkg, synth, dev, kind):
    fam = Family("dense_stream_k", "GK", kernel="KERNEL_DENSE", exact=DENSE_NAME)
    for plan in _forward_kind(pkg, synth, dev, fam, kind, combos=[(False, False), (True, True)]):
        assert plan.stat("streamk") == 1 and plan.stat("streamk_gave_up") == 0
        assert _n_cu() != lc.N_CU or plan.stat("dense_variant") == lc.GK_VARIANT


ROWS = [(r, "AUTO") for r in lc.BODY + lc.DENSE] + [(r, "TILED") for r in lc.BODY] + [(r, "DENSE") for r in lc.DENSE]


def _row_family(row, kn):
    """A row of layout_cases as a family: the 23 BODY rows tiled as for a batch of 256, generated code under AUTO with
    the row's body variant, the stream kernel under TILED; the eight DENSE rows on the dense kernel."""
    if isinstance(row, lc.DenseRow):
        return Family("%s-%s" % (row.name, kn), row.name, spec=lc.spec(row), kernel="KERNEL_" + kn, exact=DENSE_NAME)
    if kn == "TILED":
        return Family("%s-TILED" % row.name, row.name, spec=lc.spec(row), kernel="KERNEL_TILED", tiling_batch=lc.TILING_BATCH,
                      name=("tiled",), stats=dict(kernel_choice="KERNEL_TILED"), **row.options)
    stats = dict(body_variant=row.variant) if _n_cu() == lc.N_CU else {}
    return Family("%s-AUTO" % row.name, row.name, spec=lc.spec(row), tiling_batch=lc.TILING_BATCH, name=("jit",), stats=stats, **row.options)


@pytest.mark.parametrize("row,kn", ROWS, ids=["%s-%s" % (r.name, k) for r, k in ROWS])
def test_forward_subnormal_results_on_every_layout_row(pkg, synth, dev, row, kn):
    fam = _row_family(row, kn)
    for plan in _forward_kind(pkg, synth, dev, fam, "sub_out", combos=[(True, False), (True, True)]):
        if isinstance(row, lc.DenseRow) and _n_cu() == lc.N_CU:
            assert plan.stat("dense_variant") == row.expect_variant, (row.name, plan.stat("dense_variant"))


# ---- backward ---------------------------------------------------------------------------------------------------------------------
BACKWARD = [
    Family("gather_entry", "L3X3", backward_kernel="KERNEL_GENERIC", wgrad_kernel="WGRAD_ENTRY",
           stats=dict(bwd_data_kernel="KERNEL_GENERIC", wgrad_kernel="WGRAD_ENTRY")),
    Family("tiled_staged", "L3X3", backward_kernel="KERNEL_TILED", wgrad_kernel="WGRAD_STAGED",
           stats=dict(bwd_data_kernel="KERNEL_TILED", wgrad_kernel="WGRAD_STAGED")),
    Family("jit_mfma", "L3X3", backward_kernel="KERNEL_JIT", tiling_batch=256, wgrad_kernel="WGRAD_MFMA",
           stats=dict(bwd_data_kernel="KERNEL_JIT", wgrad_kernel="WGRAD_MFMA")),
    Family("dense_entry", "L3X3", backward_kernel="KERNEL_DENSE", wgrad_kernel="WGRAD_ENTRY",
           stats=dict(bwd_data_kernel="KERNEL_DENSE", wgrad_kernel="WGRAD_ENTRY")),
    Family("dgrad_mfma_3x3", "L3X3", backward_kernel="BWD_MFMA", wgrad_kernel="WGRAD_MFMA",
           stats=dict(bwd_data_kernel="BWD_MFMA", wgrad_kernel="WGRAD_MFMA")),
    Family("dgrad_mfma_stride2", "STR2", backward_kernel="BWD_MFMA", wgrad_kernel="WGRAD_ENTRY",
           stats=dict(bwd_data_kernel="BWD_MFMA", wgrad_kernel="WGRAD_ENTRY")),
    Family("s2d_inner", "STR2", s2d=1, name=(S2D_PACK,)),
    Family("s2b_inner", "DIL", s2b=1, name=(S2B_PACK, S2B_UNPACK)),
    Family("s2b_inner_jit", "DIL", s2b=1, kernel="KERNEL_JIT", backward_kernel="KERNEL_JIT", tiling_batch=256,
           name=(S2B_PACK, "jit", S2B_UNPACK), stats=dict(bwd_data_kernel="KERNEL_JIT")),
    Family("double", "L3X3", f64=True, wgrad_kernel="WGRAD_ENTRY", name=("f64",),
           stats=dict(bwd_data_kernel="KERNEL_GENERIC", wgrad_kernel="WGRAD_ENTRY")),
    Family("b2s_jit", "IP", spec=IP_SPEC, b2s=1, kernel="KERNEL_JIT", tiling_batch=4096, backward_kernel="KERNEL_JIT", name=(B2S_PACK, "jit"),
           stats=dict(bwd_data_kernel="KERNEL_JIT")),
    Family("b2s_dense", "IP", spec=IP_SPEC, b2s=1, kernel="KERNEL_DENSE", backward_kernel="KERNEL_DENSE", wgrad_kernel="WGRAD_MFMA",
           name=(B2S_PACK, DENSE_NAME), stats=dict(bwd_data_kernel="KERNEL_DENSE", wgrad_kernel="WGRAD_MFMA")),
    Family("b2s_generic", "IP", spec=IP_SPEC, b2s=1, kernel="KERNEL_GENERIC", backward_kernel="KERNEL_GENERIC", wgrad_kernel="WGRAD_ENTRY",
           name=(B2S_PACK, "generic"), stats=dict(bwd_data_kernel="KERNEL_GENERIC", wgrad_kernel="WGRAD_ENTRY")),
]


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("kind", ec.KINDS)
@pytest.mark.parametrize("fam", BACKWARD, ids=IDS(BACKWARD))
def test_backward_at_the_edges_within_the_bound(pkg, synth, dev, fam, kind, relu):
    """Data gradient, dense and compact weight gradient, bias gradient and (float plans) the dense weight gradient.  The
    ReLU runs use the top of the same plan's forward on the sub_out inputs: the mask sees positive subnormal tops."""
    s, e = ec.edge(synth, fam.layer, kind, backward=True, f64=fam.f64, spec=fam.spec)
    plan = fam.plan(pkg, s, relu)
    topd = top = None
    if relu:
        so = ec.edge(synth, fam.layer, "sub_out", f64=fam.f64, spec=fam.spec)[1]
        plan.weight_align(so.w)
        topd = plan.forward(_up(so.x, dev), _up(so.b, dev)).clone()
        torch.cuda.synchronize()
        top = topd.cpu().numpy()
        assert ec.positive_subnormal(top, fam.f64).sum() > 0.25 * top.size, (fam.id, "the mask needs positive subnormal tops")
    plan.weight_align(e.w)
    xd, tdd = _up(e.x, dev), _up(e.top_diff, dev)
    bd, wd, bsd = plan.backward(tdd, bottom=xd, top=topd, bottom_diff=True, weight_diff=True, bias_diff=True)
    _, vd, _ = plan.backward(tdd, bottom=xd, top=topd, bottom_diff=None, values_diff=True)
    dw = None if fam.f64 else plan.dense_wgrad(tdd, xd, topd)
    torch.cuda.synchronize()
    fam.ran(pkg, plan)
    pos = csr_positions(plan)
    plan.close()
    want, Bs = eb.backward_bound(s, e.w, e.x, e.b, e.top_diff, top, f64=fam.f64)
    what = (fam.id, kind, "relu", relu)
    got = [a.cpu().numpy() for a in (bd, wd, bsd, vd)]
    rs = [_within(got[0], want[0], Bs[0], fam.id + " data", kind, what), _within(got[1], want[1], Bs[1], fam.id + " weights", kind, what),
          _within(got[2], want[2], Bs[2], fam.id + " bias", kind, what),
          _within(got[3], want[1].reshape(-1)[pos], Bs[1].reshape(-1)[pos], fam.id + " compact", kind, what)]
    assert np.all(got[1][e.w == 0] == 0), what
    if dw is not None:
        dwant, dB = eb.backward_bound(s, e.w, e.x, None, e.top_diff, top, mask=np.ones(e.w.shape, bool))
        got.append(dw.cpu().numpy())
        rs.append(_within(got[4], dwant[1], dB[1], "dense_wgrad " + fam.layer, kind, what))
    print("edges backward %-20s %-8s relu=%d: data %.3g weights %.3g bias %.3g compact %.3g dense_wgrad %s" %
          ((fam.id, kind, relu) + tuple(rs[:4]) + (rs[4] if dw is not None else "-",)))
    if kind == "near_max":
        assert all(np.all(np.isfinite(a)) for a in got), what


# ---- reach, forward ---------------------------------------------------------------------------------------------------------------
def _reach_forward(pkg, synth, dev, fam, reach_of, relu_too=True):
    """NaN at poison_positions: the non-finite set is reach_of(s, pattern, poisoned) exactly and every other element is
    within the bound of the poison-free reference; on a fuse_relu plan every reached element is +0."""
    s, sk = ec.skewed(synth, fam.layer, fam.spec)
    dt = np.float64 if fam.f64 else np.float32
    pos = eb.poison_positions(s, sk.w)
    bad, _ = ec.poisoned_bottom(sk.x.astype(dt), pos, np.nan)
    reach = reach_of(s, sk.w, eb.poisoned(bad.shape, pos))
    assert 0 < reach.sum() < reach.size, (fam.id, reach.sum())
    xd, bd = _up(bad, dev), _up(sk.b.astype(dt), dev)
    for relu in (False, True) if relu_too else (False,):
        plan = fam.plan(pkg, s, relu)
        plan.weight_align(sk.w.astype(dt))
        got = plan.forward(xd, bd)
        torch.cuda.synchronize()
        fam.ran(pkg, plan)
        got = got.cpu().numpy()
        what = (fam.id, "relu", relu, plan.kernel_name, plan.tiling_info)
        plan.close()
        want, B = ec.skewed_forward_ref(synth, fam.layer, relu, fam.f64, fam.spec)
        nonfinite = ~np.isfinite(got)
        if relu:
            assert not nonfinite.any(), (what, "a NaN survived the ReLU at", np.argwhere(nonfinite)[:4].tolist())
            assert np.all(got[reach] == 0) and not np.any(np.signbit(got[reach])), (what, "a reached NaN is +0 under ReLU")
        else:
            leaked, missed = nonfinite & ~reach, reach & ~nonfinite
            assert not leaked.any() and not missed.any(), \
                (what, "reach %d, leaked to %d elements %s, missed %d %s; poisoned %s" %
                 (reach.sum(), leaked.sum(), np.argwhere(leaked)[:6].tolist(), missed.sum(), np.argwhere(missed)[:6].tolist(), pos))
            assert np.all(np.isnan(got[reach]))
        _within(np.where(reach, 0, got), np.where(reach, 0, want), B, fam.id, "reach", what)


def _sparse_reach(s, w, poisoned):
    return eb.reach_forward(s, w, poisoned)


def _dense_reach(s, w, poisoned):
    return eb.reach_forward_dense(s, poisoned)


def _mixed_reach(s, w, poisoned):
    """The dense reach on the output channels of conv group 0 (the dense kernel's), the sparse reach on group 1's."""
    r = eb.reach_forward(s, w, poisoned)
    mg = s.M // s.group
    r[:, :mg] = eb.reach_forward_dense(s, poisoned)[:, :mg]
    return r


@pytest.mark.parametrize("fam", SPARSE, ids=IDS(SPARSE))
def test_nan_in_the_bottom_reaches_exactly_the_outputs_whose_nonzeros_read_it(pkg, synth, dev, fam):
    _reach_forward(pkg, synth, dev, fam, _sparse_reach)


B2S = [f for f in SPARSE + DENSE if f.id.startswith("b2s_")]


@pytest.mark.parametrize("fam", B2S, ids=IDS(B2S))
def test_nan_in_one_image_of_an_inner_product_layer_reaches_only_that_image(pkg, synth, dev, fam):
    """Option "b2s" lays the batch out as positions of inner images: a NaN in image 37's bottom (an interior position of the
    first inner image) and in image 69's (the last used position of the second, 58 padding positions behind it) reaches only
    outputs of those two images -- the ones errbound's reach names -- and nothing of their neighbours in the inner row."""
    s, sk = ec.skewed(synth, fam.layer, fam.spec)
    live = int(np.flatnonzero((sk.w != 0).any(axis=(0, 2, 3)))[0])
    pos = [(37, live, 0, 0), (s.N - 1, live, 0, 0)]
    bad, _ = ec.poisoned_bottom(sk.x, pos, np.nan)
    ind = eb.poisoned(bad.shape, pos)
    reach = eb.reach_forward_dense(s, ind) if fam in DENSE else eb.reach_forward(s, sk.w, ind)
    assert reach[[37, s.N - 1]].any(axis=(1, 2, 3)).all() and not np.delete(reach, [37, s.N - 1], axis=0).any()
    plan = fam.plan(pkg, s, False)
    plan.weight_align(sk.w)
    got = plan.forward(_up(bad, dev), _up(sk.b, dev))
    torch.cuda.synchronize()
    fam.ran(pkg, plan)
    plan.close()
    got = got.cpu().numpy()
    assert np.array_equal(~np.isfinite(got), reach), (fam.id, np.argwhere(~np.isfinite(got) != reach)[:6].tolist())
    want, B = ec.skewed_forward_ref(synth, fam.layer, False, spec=fam.spec)
    _within(np.where(reach, 0, got), np.where(reach, 0, want), B, fam.id, "reach", fam.id)


@pytest.mark.parametrize("kn", ["AUTO", "TILED"])
@pytest.mark.parametrize("row", lc.BODY, ids=[r.name for r in lc.BODY])
def test_nan_in_the_bottom_on_every_tiled_layout_row(pkg, synth, dev, row, kn):
    """Multi-image tiles, band mode, row ends with W % 4 != 0: the epilogue's shifts across quad neighbours and its row-end
    masks must select, never multiply."""
    _reach_forward(pkg, synth, dev, _row_family(row, kn), _sparse_reach, relu_too=row.name in ("seg7_5", "seg13", "five14", "pw7x7"))


@pytest.mark.parametrize("fam", DENSE + [MIXED], ids=IDS(DENSE + [MIXED]))
def test_nan_in_the_bottom_reaches_every_tap_of_its_conv_group_on_the_dense_kernel(pkg, synth, dev, fam):
    _reach_forward(pkg, synth, dev, fam, _mixed_reach if fam is MIXED else _dense_reach)


INF_FAMILIES = [f for f in SPARSE if f.id in ("generic_3x3", "tiled_3x3_tb256", "jit_3x3_tb256", "lowered_sparse", "jit_pointwise",
                                              "jit_5x5_groups", "s2d_stride2", "s2b_jit_dilated", "double")] + DENSE[:1]


@pytest.mark.parametrize("fam", INF_FAMILIES, ids=IDS(INF_FAMILIES))
def test_one_infinity_arrives_with_the_sign_of_the_weight_that_reads_it(pkg, synth, dev, fam):
    """A single +inf in the interior: each output that a nonzero reads it through is +inf or -inf by the weight's sign (-inf
    is +0 under ReLU); on the dense kernel the pruned positions of its taps give 0 x inf = NaN; nothing else is touched."""
    s, sk = ec.skewed(synth, fam.layer, fam.spec)
    dt = np.float64 if fam.f64 else np.float32
    pos = eb.poison_positions(s, sk.w)[-1]
    bad, _ = ec.poisoned_bottom(sk.x.astype(dt), [pos], np.inf)
    hit, sg = ec.reader_sign(s, sk.w, pos, bad.shape)
    assert (sg > 0).sum() > 0 and (sg < 0).sum() > 0, (fam.id, "the interior element needs readers of both signs")
    dense = fam in DENSE
    pruned = eb.reach_forward_dense(s, eb.poisoned(bad.shape, [pos])) & ~hit
    for relu in (False, True):
        plan = fam.plan(pkg, s, relu)
        plan.weight_align(sk.w.astype(dt))
        got = plan.forward(_up(bad, dev), _up(sk.b.astype(dt), dev))
        torch.cuda.synchronize()
        fam.ran(pkg, plan)
        got = got.cpu().numpy()
        plan.close()
        what = (fam.id, "relu", relu)
        assert np.all(got[sg > 0] == np.inf), what
        if relu:
            assert np.all(got[sg < 0] == 0) and not np.any(np.signbit(got[sg < 0])), what
        else:
            assert np.all(got[sg < 0] == -np.inf), what
        if dense:
            assert np.all(got[pruned] == 0) if relu else np.all(np.isnan(got[pruned])), what
            assert np.all(np.isfinite(got[~hit & ~pruned])), what
        else:
            assert np.all(np.isfinite(got[~hit])), what


PARTIAL = [f for f in FORWARD if f.id in ("generic_3x3", "tiled_3x3", "tiled_3x3_tb256", "jit_3x3", "jit_3x3_tb256", "dense_3x3",
                                          "jit_pointwise", "s2b_jit_dilated", "s2d_stride2", "b2s_jit", "b2s_dense", "b2s_generic")]


@pytest.mark.parametrize("fam", PARTIAL, ids=IDS(PARTIAL))
def test_a_poisoned_image_past_the_call_s_batch_reaches_nothing(pkg, synth, dev, fam):
    """The first images of the plan's batch; every element of the images behind them in the bottom blob is NaN."""
    s, sk = ec.skewed(synth, fam.layer, fam.spec)
    n = max(1, s.N // 2)
    bad = sk.x.copy()
    bad[n:] = np.nan
    plan = fam.plan(pkg, s, False)
    plan.weight_align(sk.w)
    xd = _up(bad, dev)
    top = torch.full((s.N, s.M) + ec.out_hw(s), -7.5, device=dev)
    plan.forward(xd[:n], _up(sk.b, dev), top[:n])
    torch.cuda.synchronize()
    fam.ran(pkg, plan)
    plan.close()
    want, B = ec.skewed_forward_ref(synth, fam.layer, False, spec=fam.spec)
    _within(top[:n].cpu().numpy(), want[:n], B[:n], fam.id, "partial", (fam.id, "first images", n))
    assert bool((top[n:] == -7.5).all()), (fam.id, "images past the call's were written")


# ---- reach, data gradient -----------------------------------------------------------------------------------------------------------
DATA_EXACT = [f for f in BACKWARD if f.id in ("gather_entry", "tiled_staged", "jit_mfma", "s2b_inner_jit", "double")]
DATA_DENSE = [f for f in BACKWARD if f.id in ("dense_entry", "dgrad_mfma_3x3", "dgrad_mfma_stride2")]


def _reach_data(pkg, synth, dev, fam):
    s, sk = ec.skewed(synth, fam.layer)
    dt = np.float64 if fam.f64 else np.float32
    pos = eb.poison_positions_top(s, sk.w, ec.out_hw(s))
    bad, clean = ec.poisoned_bottom(sk.top_diff.astype(dt), pos, np.nan)
    plan = fam.plan(pkg, s, False)
    plan.weight_align(sk.w.astype(dt))
    got = plan.backward(_up(bad, dev), bottom_diff=True)[0]
    torch.cuda.synchronize()
    assert plan.stat("bwd_data_kernel") == getattr(pkg, fam.stats["bwd_data_kernel"]), (fam.id, plan.stat("bwd_data_kernel"))
    plan.close()
    return s, sk, pos, clean, got.cpu().numpy()


@pytest.mark.parametrize("fam", DATA_EXACT, ids=IDS(DATA_EXACT))
def test_nan_in_top_diff_reaches_exactly_the_bottom_diff_elements_whose_nonzeros_read_it(pkg, synth, dev, fam):
    s, sk, pos, clean, got = _reach_data(pkg, synth, dev, fam)
    reach = eb.reach_data(s, sk.w, eb.poisoned(clean.shape, pos))
    assert 0 < reach.sum() < reach.size
    nonfinite = ~np.isfinite(got)
    leaked, missed = nonfinite & ~reach, reach & ~nonfinite
    assert not leaked.any() and not missed.any(), (fam.id, "reach %d, leaked %d %s, missed %d %s" % (
        reach.sum(), leaked.sum(), np.argwhere(leaked)[:6].tolist(), missed.sum(), np.argwhere(missed)[:6].tolist()))
    want, Bs = eb.backward_bound(s, sk.w, sk.x, None, clean, f64=fam.f64)
    _within(np.where(reach, 0, got), np.where(reach, 0, want[0]), Bs[0], fam.id + " data", "reach", fam.id)


@pytest.mark.parametrize("fam", DATA_DENSE, ids=IDS(DATA_DENSE))
def test_nan_in_top_diff_on_the_dense_data_gradient_kernels_stays_inside_the_dense_reach(pkg, synth, dev, fam):
    """0 x G inside a live step (include/escoin.h): at least the sparse reach, at most the dense one."""
    s, sk, pos, clean, got = _reach_data(pkg, synth, dev, fam)
    ind = eb.poisoned(clean.shape, pos)
    lo, hi = eb.reach_data(s, sk.w, ind), eb.reach_data_dense(s, ind)
    nonfinite = ~np.isfinite(got)
    print("edges reach %-20s: %d non-finite elements; sparse reach %d, dense reach %d" % (fam.id, nonfinite.sum(), lo.sum(), hi.sum()))
    assert not (lo & ~nonfinite).any() and not (nonfinite & ~hi).any(), (fam.id, (lo & ~nonfinite).sum(), (nonfinite & ~hi).sum())
    want, Bs = eb.backward_bound(s, sk.w, sk.x, None, clean)
    _within(np.where(nonfinite, 0, got), np.where(nonfinite, 0, want[0]), Bs[0], fam.id + " data", "reach", fam.id)


MASKED = [f for f in BACKWARD if f.id in ("gather_entry", "tiled_staged", "jit_mfma", "dense_entry", "dgrad_mfma_3x3", "dgrad_mfma_stride2",
                                          "s2d_inner", "s2b_inner", "s2b_inner_jit", "double", "b2s_jit", "b2s_dense", "b2s_generic")]


@pytest.mark.parametrize("fam", MASKED, ids=IDS(MASKED))
def test_nan_in_top_diff_under_a_masked_top_reaches_nothing(pkg, synth, dev, fam):
    """fuse_relu: a top of 0, -1, NaN or -0.0 masks its top_diff element in the gather kernel, the ReLU mask kernel of the
    transposed plans, the s2b pack, the MFMA data gradient, the three weight-gradient kernels and the dense weight
    gradient: every gradient is finite and within the bound of the reference without the poison."""
    s, sk = ec.skewed(synth, fam.layer, fam.spec)
    dt = np.float64 if fam.f64 else np.float32
    plan = fam.plan(pkg, s, True)
    plan.weight_align(sk.w.astype(dt))
    xd = _up(sk.x.astype(dt), dev)
    top = plan.forward(xd, _up(sk.b.astype(dt), dev)).cpu().numpy()
    bad, clean, t = masked_top_case(s, sk, top, sk.w, ec.out_hw(s))
    tdd, topd = _up(bad.astype(dt), dev), _up(t, dev)
    bd, wd, bsd = plan.backward(tdd, bottom=xd, top=topd, bottom_diff=True, weight_diff=True, bias_diff=True)
    _, vd, _ = plan.backward(tdd, bottom=xd, top=topd, bottom_diff=None, values_diff=True)
    dw = None if fam.f64 else plan.dense_wgrad(tdd, xd, topd)
    torch.cuda.synchronize()
    fam.ran(pkg, plan)
    pos = csr_positions(plan)
    plan.close()
    want, Bs = eb.backward_bound(s, sk.w, sk.x, sk.b, clean, t, f64=fam.f64)
    _within(bd.cpu().numpy(), want[0], Bs[0], fam.id + " data", "masked", fam.id)
    _within(wd.cpu().numpy(), want[1], Bs[1], fam.id + " weights", "masked", fam.id)
    _within(bsd.cpu().numpy(), want[2], Bs[2], fam.id + " bias", "masked", fam.id)
    _within(vd.cpu().numpy(), want[1].reshape(-1)[pos], Bs[1].reshape(-1)[pos], fam.id + " compact", "masked", fam.id)
    if dw is not None:
        dwant, dB = eb.backward_bound(s, sk.w, sk.x, None, clean, t, mask=np.ones(sk.w.shape, bool))
        _within(dw.cpu().numpy(), dwant[1], dB[1], "dense_wgrad " + fam.layer, "masked", fam.id)


# ---- the solver rule on special values ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["float", "double"])
@pytest.mark.parametrize("rule,reg", ec.RULE_REG, ids=["%s-%s" % p for p in ec.RULE_REG])
def test_array_step_on_the_grid_of_special_values(pkg, dev, rule, reg, dt):
    w, g, h, h2 = ec.solver_grid(dt)
    for i in range(len(ec.HYPERS)):
        hy = ec.hyper(i, rule, reg)
        want = sc.step(w, g, h, h2 if rule == "adam" else None, **hy)
        data, diff, hh = _up(w, dev), _up(g, dev), _up(h, dev)
        hh2 = _up(h2, dev) if rule == "adam" else None
        pkg.solver_array_step(data, diff, hh, hh2, **hy)
        torch.cuda.synchronize()
        for what, a, b in (("data", data, want[0]), ("history", hh, want[1]), ("history2", hh2, want[2])):
            if b is not None:
                a = a.cpu().numpy()
                if not sc.equal_up_to_nan_payload(a, b):
                    bad = np.flatnonzero((np.isnan(a) != np.isnan(b)) | (~np.isnan(a) & ~np.isnan(b) & (a.view(np.uint8).reshape(a.size, -1) !=
                                                                                               b.view(np.uint8).reshape(b.size, -1)).any(axis=1)))
                    k = int(bad[0])
                    pytest.fail("%s %s hyper %d %s: %d elements differ; first: w %r g %r h %r h2 %r -> got %r, want %r" %
                                (rule, reg, i, what, bad.size, w[k], g[k], h[k], h2[k], a[k], b[k]))


@pytest.mark.parametrize("rule", ["sgd", "nesterov", "adam"])
def test_plan_solver_step_on_the_finite_special_values(pkg, synth, dev, rule):
    """The generated-code plan on L3X3 with the finite specials as values, gradient and histories: the step equals the
    restatement, and the plan's forward afterwards equals a fresh plan's on the same values bit for bit."""
    s, w0, x, b, _ = ec.base(synth, "L3X3")
    opts = dict(kernel=pkg.KERNEL_JIT, tiling_batch=256)
    plan, fresh = pkg.Plan(pkg.ConvDesc.from_shape(s), **opts), pkg.Plan(pkg.ConvDesc.from_shape(s), **opts)
    plan.weight_align(w0)
    fresh.weight_align(w0)
    assert "jit" in plan.kernel_name and plan.kernel_name == fresh.kernel_name
    n = plan.nnz()
    dt = np.float32
    w, g, h = finite_specials(n, dt), finite_specials(n, dt, 5), finite_specials(n, dt, 11)
    h2 = np.abs(finite_specials(n, dt, 3)) if rule == "adam" else None
    plan.set_values(_up(w, dev))
    hy = ec.hyper(1, rule, "L1")
    want = sc.step(w, g, h, h2, **hy)
    hh, hh2 = _up(h, dev), _up(h2, dev)
    plan.solver_step(_up(g, dev), hh, hh2, **hy)
    torch.cuda.synchronize()
    got = plan.get_csr()[2]
    assert sc.equal_up_to_nan_payload(got, want[0]) and sc.equal_up_to_nan_payload(hh.cpu().numpy(), want[1])
    assert h2 is None or sc.equal_up_to_nan_payload(hh2.cpu().numpy(), want[2])
    fresh.set_values(_up(got, dev))
    xd, bd = _up(x, dev), _up(b, dev)
    a, c = plan.forward(xd, bd).cpu().numpy(), fresh.forward(xd, bd).cpu().numpy()
    assert sc.equal_up_to_nan_payload(a, c)
    plan.close()
    fresh.close()
