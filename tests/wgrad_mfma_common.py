"""Shared by test_wgrad_mfma_host.py and test_wgrad_mfma_gpu.py: the shapes the MFMA weight-gradient kernel is tested on --
wgrad_common.SHAPES (all sparse) plus dense ones at the kernel's tile edges (tiles of 64 output channels x 64 columns,
chunks of 1024 pixels, steps of 32 pixels, two pixels per matrix instruction)."""
from wgrad_common import SHAPES

# name: (N, C, H, W, M, KH, kwargs of synth.shape)
DENSE = {
    "d_pw": (3, 40, 19, 19, 70, 1, dict(sparsity=0.0)),        # 1083 px: chunk boundary mid-row of image 2, odd pixel count, Mg = 2 x 32 + 6, Kd = 40
    "d_3x3": (2, 20, 24, 24, 36, 3, dict(pad=1, sparsity=0.0)),                    # halo, Kd = 180
    "d_conv1": (2, 3, 37, 37, 24, 7, dict(pad=3, stride=2, sparsity=0.0)),         # Cg = 3, Kd = 147, stride 2, one chunk
    "d_s2pw": (5, 48, 15, 15, 40, 1, dict(stride=2, sparsity=0.0)),                # pointwise, stride 2
    "d_g3": (4, 18, 9, 10, 15, 3, dict(pad=1, group=3, sparsity=0.3)),             # Mg = 5, groups, masked positions inside a dense tile
    "d_onepx": (1, 5, 3, 3, 4, 3, dict(sparsity=0.0)),                             # a single output pixel
}
ALL = dict(SHAPES)
ALL.update(DENSE)


def make(synth, name):
    N, C, H, W, M, K, kw = ALL[name]
    return synth.shape(name, N, C, H, W, M, K, **kw)
