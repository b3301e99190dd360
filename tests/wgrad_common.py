"""Shared by the Backward's tests (test_backward_cpu.py, test_backward_gpu.py, test_backward_values_cpu.py,
test_wgrad_staged_gpu.py) and tools/fuzz_backward.py: the shapes, the torch float64 reference and the map from compact CSR
entries to positions of the dense weight blob."""
import numpy as np
import torch

F = torch.nn.functional

# name: (N, C, H, W, M, KH, kwargs of synth.shape) -- the smallest shapes that still cross each boundary of the chunked
# reduction (1024 flattened (n, oh, ow) pixels per chunk)
SHAPES = {
    "straddle3x3": (3, 20, 19, 19, 12, 3, dict(pad=1, sparsity=0.6)),            # 1083 px: the boundary falls mid-row in image 2
    "small7x7g2": (43, 8, 7, 7, 8, 3, dict(pad=1, group=2, sparsity=0.5)),       # ~21 images per chunk, 3 chunks, groups
    "pointwise": (6, 24, 14, 14, 16, 1, dict(sparsity=0.8)),                     # no halo, rows of 2-9 entries
    "wide_rows": (2, 6, 5, 70, 10, 3, dict(pad=1, sparsity=0.5)),                # an image row longer than a wave
    "big_image": (2, 4, 40, 40, 6, 5, dict(pad=2, sparsity=0.7)),                # a chunk is a fraction of an image
    "dil2_asym": (3, 6, 21, 18, 8, 3, dict(KW=2, pad=2, pad_w=1, dil=2, group=2, sparsity=0.5)),   # OW != W
    "dense_rows": (2, 32, 24, 24, 4, 3, dict(pad=1, sparsity=0.3)),              # ~200 entries per row
    "stride2": (5, 8, 31, 31, 8, 3, dict(pad=1, stride=2, sparsity=0.6)),        # no staged kernel: the entry kernel
}


def make_shape(synth, name):
    N, C, H, W, M, K, kw = SHAPES[name]
    return synth.shape(name, N, C, H, W, M, K, **kw)


def seeded(shape, seed, dt=np.float32):
    return np.random.RandomState(seed).uniform(-1, 1, shape).astype(dt)


def torch_backward(x, w, bias, s, top_diff, top=None, mask=None):
    """torch float64 autograd: (bottom_diff, weight_diff masked by the pattern, bias_diff); with `top` the gradient is
    top_diff x [top > 0]."""
    X = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    Wt = torch.tensor(np.asarray(w, np.float64), requires_grad=True)
    B = torch.tensor(np.asarray(bias, np.float64), requires_grad=True) if bias is not None else None
    y = F.conv2d(X, Wt, B, stride=(s.stride_h, s.stride_w), padding=(s.pad_h, s.pad_w),
                 dilation=(s.dil_h, s.dil_w), groups=s.group)
    g = torch.tensor(np.asarray(top_diff, np.float64))
    if top is not None:
        g = g * torch.tensor((np.asarray(top) > 0).astype(np.float64))
    y.backward(g)
    m = (np.asarray(w) != 0) if mask is None else mask
    return X.grad.numpy(), Wt.grad.numpy() * m, B.grad.numpy() if B is not None else None


# Directed edges of the Backward (test_backward_gpu.py on the device, test_backward_cpu.py through backward_cpu):
# name: (N, C, H, W, M, KH, kwargs of synth.shape)
EDGES = {
    "mg40000": (2, 1, 2, 2, 40000, 1, dict(sparsity=0.5)),               # Mg > 32767: no transposed plan, ocl above 15 bits
    "lenet5x5_pad0": (3, 6, 12, 12, 10, 5, dict(sparsity=0.5)),          # transposed pad 4
    "5x5_pad4": (3, 6, 12, 12, 10, 5, dict(pad=4, sparsity=0.5)),        # transposed pad 0
    "3x5_pad2x0": (3, 6, 12, 12, 10, 3, dict(KW=5, pad=2, pad_w=0, sparsity=0.5)),   # transposed pads (0, 4)
    "relu3x3_n7": (7, 8, 9, 10, 12, 3, dict(pad=1, sparsity=0.6)),       # partial batches at tiling_batch 256
    "chunked": (11, 6, 9, 10, 8, 3, dict(pad=1, sparsity=0.7)),          # test_batches_beyond_one_buffer_descriptor's
    "overpad3x3": (3, 6, 9, 11, 8, 3, dict(pad=3, sparsity=0.5)),        # pad > dil * (K - 1)
    "nopad3x3": (3, 6, 20, 19, 8, 3, dict(sparsity=0.5)),                # pad 0 < K - 1: OW != W, 918 px in one chunk
    "nopad3x3_n4": (4, 6, 20, 19, 8, 3, dict(sparsity=0.5)),             # 1224 px: the chunk boundary falls mid-row
    "group_pruned": (2, 8, 10, 11, 12, 3, dict(pad=1, group=2, sparsity=0.3)),   # group 0 without a nonzero
    # tools/fuzz_backward.py 2000 4242, k = 24: the transposed plan has 36 input and 2 output channels per group, 70 %
    # dense 5 x 5: at tiling_batch 256 its weight stream exceeds the stream kernel's LDS budget
    "stream_budget": (182, 8, 1, 6, 144, 5, dict(pad=4, pad_w=2, group=4, sparsity=0.3)),
}


def edge_inputs(synth, name):
    """(shape, weights, activations, bias) of a directed edge."""
    N, C, H, W, M, K, kw = EDGES[name]
    s = synth.shape(name, N, C, H, W, M, K, **kw)
    w = synth.pruned_weights(s, 1024 if name == "stream_budget" else 31)     # (1024: the fuzzer's weights of that case)
    if name == "group_pruned":
        w[:M // 2] = 0          # every input channel of the transposed plan's first group: empty rows next to full ones
    return s, w, synth.activations(s, 32), synth.bias_vector(s, 33)


def tiled_ok(d):
    """The geometries the two LDS-tiled kernel families (KERNEL_TILED, KERNEL_JIT) cover; `d`: a ConvDesc, a Golden or a
    synth shape.  A forced TILED can still be refused when its weight stream exceeds the LDS budget: that depends on the
    nonzeros, not on the geometry."""
    return (d.stride_h == 1 and d.stride_w == 1 and d.dil_h == 1 and d.dil_w == 1 and d.KW <= 5 and
            max(d.W, d.W + 2 * d.pad_w - d.KW + 1) <= 256 and d.pad_w <= 4 and d.KW - 1 - d.pad_w <= 4)


def csr_positions(plan):
    """wpos[e] = (grp * Mg + m) * Cg * KH * KW + colidx[e] for every entry of get_csr(), groups concatenated."""
    d = plan.desc
    rp, ci, _, ng = plan.get_csr()
    mg, kdim = d.M // d.group, (d.C // d.group) * d.KH * d.KW
    pos = np.zeros(len(ci), np.int64)
    base = 0
    for grp in range(d.group):
        r = rp[grp * (mg + 1):(grp + 1) * (mg + 1)]
        for m in range(mg):
            e = np.arange(r[m], r[m + 1]) + base
            pos[e] = (grp * mg + m) * kdim + ci[e]
        base += int(ng[grp])
    return pos
