"""layout_cases.py without a GPU: on every row the checker passes the fp32 oracle and fails three corruptions of one
low-scale channel that the suite's max-norm passes (so the GPU module's per-element check can see an accumulator stored
to the wrong channel, quad or image on that row), and the table says what the code does -- the host rules give every
BODY row the tiling it names on 256 compute units and accept it on the stream kernel, launch_dense's rule gives every
DENSE row the variant it names."""
import numpy as np
import pytest

import errbound as eb
import layout_cases as lc
from conftest import rel_err
from test_align_rules import build_host_rules, host_rules

TOL = 1e-4      # the suite's max-norm tolerance
ROWS = lc.BODY + lc.DENSE
KERNEL_AUTO, KERNEL_TILED, KERNEL_JIT = 0, 2, 4


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_the_checker_sees_three_corruptions_of_a_low_channel_on_every_row(oracle, synth, row):
    s, sk, _ = lc.layer(synth, row)
    g = oracle.geom(s.C, s.H, s.W, s.M, s.KH, s.KW, s.pad_h, s.pad_w, s.stride_h, s.stride_w, s.dil_h, s.dil_w, s.group)
    out = oracle.conv_forward(g, sk.x, sk.w, sk.b, gate=False, threads=4)
    want, B = eb.forward_bound(s, sk.w, sk.x, sk.b)
    ratio = eb.within(out, want, B, "the fp32 oracle", sk.row_exp, what=s.name)
    m, src = eb.corruption_target(want, sk.w, sk.b)
    mag = eb.low_channels(want)[1]
    assert eb.row_nnz(sk.w)[m] > 0 and sk.b[m] != 0 and mag[src] >= 2.0 ** 20 * mag[m], (m, src, mag[m], mag[src])
    bad = {"bias dropped": eb.drop_bias(out, sk.b, m), "2^-30 of row %d" % src: eb.leak_from(out, m, src),
           "images 0 and 1 swapped": eb.swap_images(out, m)}
    print("%s: oracle at %.3g of the bound; channel %d (2^%d)" % (s.name, ratio, m, sk.row_exp[m]))
    for what, c in bad.items():
        r, idx = eb.check(c, want, B)
        print("    %-24s rel_err %.3g   err / bound %.3g at %s" % (what, rel_err(c, want), r, idx))
        assert rel_err(c, want) <= TOL, (what, "the max-norm was expected to pass this")
        assert r > 1.0 and idx[1] == m, (what, r, idx)


def _case(synth, row, kernel):
    """The row as a case of tools/align_fingerprint.py (what host_rules takes): layer()'s weights, by their seed.  Of the
    row's options the rules read none ("stream_stores" picks the epilogue's store instruction at launch)."""
    s = synth.shape(row.name, *row.dims, **row.kw)
    shape = {k: int(getattr(s, k)) for k in s._fields if k not in ("name", "sparsity", "count")}
    return dict(name=row.name, shape=shape, sparsity=s.sparsity, seed=sum(map(ord, row.name)), dist="uniform",
                options=dict(kernel=kernel, tiling_batch=lc.TILING_BATCH))


def test_the_host_rules_give_every_body_row_the_tiling_it_names(tmp_path, synth):
    exe = build_host_rules(tmp_path)
    assert np.array_equal(lc.layer(synth, lc.BODY[0])[2][0] != 0, lc.layer(synth, lc.BODY[0])[1].w != 0)     # skew keeps the pattern
    auto = host_rules(exe, tmp_path, synth, [_case(synth, r, KERNEL_AUTO) for r in lc.BODY], lc.N_CU)
    tiled = host_rules(exe, tmp_path, synth, [_case(synth, r, KERNEL_TILED) for r in lc.BODY], lc.N_CU)
    assert len(lc.BODY) == 23
    for row, a, t in zip(lc.BODY, auto, tiled):
        print("%-10s %s\n           %s" % (row.name, a["tiling_info"], t["tiling_info"]))
        assert a["kernel_choice"] == KERNEL_JIT, (row.name, a)
        missing = [e for e in row.expect if e not in a["tiling_info"]]
        assert not missing, (row.name, missing, a["tiling_info"])
        assert t["kernel_choice"] == KERNEL_TILED and t["tiling_info"].startswith("stream "), (row.name, t)


def test_launch_dense_gives_every_dense_row_the_variant_it_names(synth):
    seen = set()
    for row in lc.DENSE:
        s = synth.shape(row.name, *row.dims, **row.kw)
        assert s.bias and s.sparsity == 0.0
        assert lc.dense_variant(s, s.N) == row.expect_variant, row.name
        seen.add(row.expect_variant)
    s = synth.shape("dn_pw64", *lc.DENSE[2].dims, **lc.DENSE[2].kw)
    for _, b_off, t_off, v in lc.OFF_BOUNDARY:
        assert lc.dense_variant(s, s.N, bottom_aligned=not b_off, top_aligned=not t_off) == v
        seen.add(v)
    gk = synth.shape("gk", 64, 1024, 7, 7, 512, 1, sparsity=0.0)
    assert lc.dense_variant(gk, gk.N) == lc.GK_VARIANT
    assert seen | {lc.GK_VARIANT} == {1, 2, 5, 9, 10, 13, 14, 18, 29, 30}
    # stream-K is a matter of the images of the call too: the GPU module's partial batch of sk_pw64 (83 images: 42 tiles x
    # 32 k-steps, fewer than four per slot) runs whole tiles, that of sk_pw128 (35 images: 72 tiles) splits K again
    sk64, sk128 = (synth.shape(r.name, *r.dims, **r.kw) for r in lc.DENSE[6:8])
    assert lc.dense_variant(sk64, sk64.N // 2 + 3) == 13 and lc.dense_variant(sk128, sk128.N // 2 + 3) == 30
