"""Shared by test_backward_values_cpu.py and test_wgrad_staged_gpu.py: the shapes, the torch float64 reference and the
map from compact CSR entries to positions of the dense weight blob."""
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
