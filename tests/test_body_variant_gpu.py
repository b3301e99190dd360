"""The two compiled bodies around generated code (csrc/sconv_tiled.hip): the chained instantiation that
launch_tiled_once picks for chained plans (align_rules.h body_variant) against the generic body (plan option
"body_variant" = 0) -- needs an MI355X.

Both run the same generated code and the same epilogue asm on the same registers, so their outputs must be EQUAL bit
for bit; against the CPU oracle both keep test_gpu_parity.py's tolerance for generated code (1e-4 relative).
Every case is tiled as for a batch of 256 and run on a few images, with bias and ReLU off and on.  The tilings named
below are what the host rules give on 256 compute units; on another device a case whose tiling differs is skipped."""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4

# (N, C, H, W, M, K, pad, sparsity), what the tiling must say, the variant the rule must pick
CASES = [
    # band mode, one-block tiles: the unit stages the NEXT tile at entry
    ("band56", (2, 8, 56, 56, 64, 3, 1, 0.9), ("band=1", "bands=7", "n_icb=1", "chained=1"), 1),
    ("band28_1", (3, 16, 28, 28, 64, 3, 1, 0.9), ("band=1", "bands=2", "n_icb=1", "chained=1"), 1),
    ("band28_2", (3, 40, 28, 28, 64, 3, 1, 0.9), ("band=1", "bands=2", "n_icb=2", "chained=1"), 1),
    # whole images per workgroup; the last tile holds one image
    ("seg14_2", (5, 24, 14, 14, 64, 3, 1, 0.9), ("nseg=2", "columns=2", " G=4", "n_icb=2", "chained=1"), 1),
    # odd block count: the buffer rotation moves on across tiles
    ("seg14_3", (5, 40, 14, 14, 64, 3, 1, 0.9), ("nseg=2", "n_icb=3", "chained=1"), 1),
    ("seg14_4", (5, 56, 14, 14, 64, 3, 1, 0.9), ("nseg=2", "n_icb=4", "chained=1"), 1),
    # OW % 4 = 3, partial second tile
    ("seg7_5", (9, 20, 7, 7, 64, 3, 1, 0.9), ("nseg=5", "chained=1"), 1),
    ("seg7_8", (17, 64, 7, 7, 128, 3, 1, 0.9), ("nseg=8", "columns=8", "n_icb=5", "chained=1"), 1),
    # OW % 4 = 1
    ("seg13", (5, 24, 13, 13, 64, 3, 1, 0.9), ("cut=13x13", "chained=1"), 1),
    ("seg9", (5, 24, 9, 9, 64, 3, 1, 0.9), ("cut=9x9", "chained=1"), 1),
    ("g8", (5, 32, 14, 14, 128, 3, 1, 0.9), (" G=8", "chained=1"), 1),
    # 15 oc-groups on 8 waves: not chained -- the generic body, and still the same result
    ("unchained", (5, 24, 14, 14, 72, 3, 1, 0.9), ("chained=0",), 0),
    # pointwise chain with three plane buffers
    ("pointwise", (5, 64, 14, 14, 64, 1, 0, 0.95), ("nbuf=3", "chained=1"), 1),
    ("five", (4, 16, 13, 13, 32, 5, 2, 0.8), ("chained=1",), 1),
    # the asm epilogue families the two bodies share (sconv_tiled.hip epi_asm_*), one row per family and OW % 4; a fifth
    # element holds further plan options
    # pointwise, rows of whole quads (ESC_EPI1S), both tiles; the same with non-temporal stores (ESC_EPI1SN)
    ("pw28", (3, 64, 28, 28, 64, 1, 0, 0.95), ("cut=98x8", "band=1", "n_icb=4", "chained=1"), 1),
    ("pw28_nt", (3, 64, 28, 28, 64, 1, 0, 0.95), ("cut=98x8", "band=1", "n_icb=4", "chained=1"), 1, {"stream_stores": 1}),
    # pointwise, rows ending in a partial quad (ESC_EPI1SP): OW % 4 = 1, 2, 3
    ("pw7x7", (9, 64, 7, 7, 128, 1, 0, 0.95), ("cut=1x49", "chained=1"), 1),
    ("pw6x7", (9, 64, 6, 7, 64, 1, 0, 0.95), ("cut=1x42", "chained=1"), 1),
    ("pw5x7", (9, 64, 5, 7, 64, 1, 0, 0.95), ("cut=1x35", "chained=1"), 1),
    # one quad per lane, 32 channels per wave: slots 24 .. 47 come out of tile B's registers -- partial and whole quads
    ("pw_tail_p", (17, 64, 7, 7, 768, 1, 0, 0.95), ("cut=1x49", "tpl=1", " G=32", "chained=1"), 1),
    ("pw_tail_w", (5, 64, 8, 8, 768, 1, 0, 0.95), ("cut=1x64", "tpl=1", " G=32", "chained=1"), 1),
    # 5x5: OW % 4 = 2; band mode with OW % 4 = 0
    ("five14", (4, 16, 14, 14, 32, 5, 2, 0.8), ("cut=14x14", "chained=1"), 1),
    ("five28", (3, 16, 28, 28, 32, 5, 2, 0.8), ("cut=28x28", "band=1", "chained=1"), 1),
]
CASES = [c if len(c) == 5 else c + ({},) for c in CASES]


@pytest.fixture(scope="module")
def torch_cuda(pkg):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert pkg.device_count() >= 1
    return torch


def _shape(synth, name, dims, bias):
    N, C, H, W, M, K, pad, sp = dims
    return synth.shape(name, N, C, H, W, M, K, pad=pad, sparsity=sp, bias=bias)


def _plan(pkg, s, w, relu, **options):
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu), kernel=pkg.KERNEL_AUTO, tiling_batch=256, **options)
    plan.weight_align(w)
    return plan


def _tiling_or_skip(torch, info, expect):
    missing = [e for e in expect if e not in info]
    if missing and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("another tiling on this device: %s" % info)
    assert not missing, (missing, info)


@pytest.mark.parametrize("name,dims,expect,variant,options", CASES, ids=[c[0] for c in CASES])
def test_chained_body_equals_generic_body(pkg, oracle, synth, torch_cuda, name, dims, expect, variant, options):
    torch = torch_cuda
    dev = torch.device("cuda:0")
    for k, on in enumerate((False, True)):          # bias and ReLU off, then on
        s = _shape(synth, name, dims, on)
        w, b, x = synth.pruned_weights(s, 4100 + k), synth.bias_vector(s, 4200 + k), synth.activations(s, 4300 + k)
        g = oracle.geom(s.C, s.H, s.W, s.M, s.KH, s.KW, s.pad_h, s.pad_w, 1, 1, 1, 1, 1)
        want = oracle.conv_forward(g, x, w, b, relu=on, gate=False, threads=4)
        xd = torch.from_numpy(x).to(dev)
        bd = torch.from_numpy(b).to(dev) if b is not None else None
        auto, generic = _plan(pkg, s, w, on, **options), _plan(pkg, s, w, on, body_variant=0, **options)
        assert "jit" in auto.kernel_name and auto.kernel_name == generic.kernel_name
        assert auto.tiling_info == generic.tiling_info
        _tiling_or_skip(torch, auto.tiling_info, expect)
        got_a, got_g = auto.forward(xd, bd), generic.forward(xd, bd)
        torch.cuda.synchronize()
        assert auto.stat("body_variant") == variant and generic.stat("body_variant") == 0, auto.tiling_info
        assert torch.equal(got_a, got_g), (name, on, float((got_a - got_g).abs().max()))
        err = rel_err(got_a.cpu().numpy(), want)
        print("%s bias/relu=%d: rel_err %.3g (%s)" % (name, on, err, auto.tiling_info))
        assert err <= TOL, (name, on, err)
        auto.close()
        generic.close()


def test_chained_body_in_a_hip_graph(pkg, oracle, synth, torch_cuda):
    """The chained body's launch is capturable like the generic one's: captured once, replayed twice on new data."""
    torch = torch_cuda
    dev = torch.device("cuda:0")
    s = _shape(synth, "graph", (5, 40, 14, 14, 64, 3, 1, 0.9), True)
    w, b = synth.pruned_weights(s, 4500), synth.bias_vector(s, 4501)
    plan = _plan(pkg, s, w, True)
    _tiling_or_skip(torch, plan.tiling_info, ("n_icb=3", "chained=1"))
    x = torch.zeros((s.N, s.C, s.H, s.W), device=dev)
    y = torch.zeros((s.N, s.M) + tuple(plan.out_hw), device=dev)
    bd = torch.from_numpy(b).to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        plan.forward(x, bd, y)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.forward(x, bd, y)
    assert plan.stat("body_variant") == 1
    g = oracle.geom(s.C, s.H, s.W, s.M, s.KH, s.KW, s.pad_h, s.pad_w, 1, 1, 1, 1, 1)
    for rnd in range(2):
        xs = synth.activations(s, 4510 + rnd)
        x.copy_(torch.from_numpy(xs).to(dev))
        y.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert rel_err(y.cpu().numpy(), oracle.conv_forward(g, xs, w, b, relu=True, gate=False, threads=4)) <= TOL, rnd
    plan.close()
