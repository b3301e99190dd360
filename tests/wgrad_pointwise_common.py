"""Shared by test_wgrad_pointwise_host.py, test_wgrad_pointwise_gpu.py and test_wgrad_pointwise_sequence_gpu.py: the
shapes plan option "wgrad_pointwise" is tested on -- small, at the pointwise kernel's edges (chunks of 1024 flattened
pixels, steps of 32 pixels, tiles of at most 4096 entries, 256 lanes of up to 16 entries) -- and the kernel's constants as
include/escoin.h and csrc/align_rules.h state them."""
import b2s_common
import d2s_common

CHUNK = 1024             # pixels per chunk
STEP = 32                # pixels per LDS step
PITCH = STEP + 4         # floats per staged row
THREADS = 256
MAX_LANE_ENTRIES = 16
MAX_TILE_ENTRIES = THREADS * MAX_LANE_ENTRIES
LDS_BUDGET = 64 * 1024
MAX_LDS_ROWS = LDS_BUDGET // (4 * PITCH)
MAX_CHANNEL_BLOCK = 256
MAX_SLICE_ROWS = THREADS
MIN_SLICE_ROWS = 8
SPLIT_WORK = 1 << 16     # (entry, chunk) pairs below which the rule does not split slices for more workgroups
WGRAD_POINTWISE = 4

# name: (N, C, H, W, M, KH, kwargs of synth.shape)
CONV = {
    # 1083 px: two chunks, the boundary mid-row of image 2; the last chunk has 59 pixels: one partial step, then dead ones
    "pw_straddle": (3, 40, 19, 19, 70, 1, dict(sparsity=0.8)),
    "pw_dense": (3, 40, 19, 19, 70, 1, dict(sparsity=0.0)),              # 2800 entries: E = 16, more than one entry per lane
    "pw_g3": (4, 18, 9, 10, 15, 1, dict(group=3, sparsity=0.3)),         # Mg = 5, Cg = 6; the tests empty rows and a group
    "pw_s2": (5, 48, 15, 15, 40, 1, dict(stride=2, sparsity=0.6)),       # the stride gather
    "pw_onepx": (1, 5, 1, 1, 4, 1, dict(sparsity=0.0)),                  # a single pixel
}
# not served: a 3x3 pad-1 layer and a 1x1 pad-1 layer
NOT_PW = {
    "not_pw_3x3": (3, 8, 9, 10, 12, 3, dict(pad=1, sparsity=0.6)),
    "not_pw_pad1": (3, 8, 9, 10, 12, 1, dict(pad=1, sparsity=0.6)),
}
FC = ("pw_fc", 70, 300, 33)                    # InnerProduct N, K, M under "b2s": inner images of 1 x 64, the second with 6 live pixels
DECONV = d2s_common.DShape("pw_deconv", 2, 5, 6, 5, 7, 2, 2, 2, 2, 0, 0, 1)     # 2x2 stride 2, 5 -> 7 channels: 28 inner channels
CHANNEL_BLOCKS = (0, 1, 7)
TILE_ENTRIES = (0, 64, 300)


def make(synth, name):
    """The synth shape of a CONV / NOT_PW name, or of "pw_fc" (the layer as the caller describes it: N images of one pixel)."""
    if name == "pw_fc":
        return b2s_common.ip_shape(synth, name, FC[1], FC[2], FC[3], sparsity=0.7)
    N, C, H, W, M, K, kw = dict(CONV, **NOT_PW)[name]
    return synth.shape(name, N, C, H, W, M, K, **kw)


def fc_inner(synth):
    """The pointwise inner layer "b2s" runs "pw_fc" as: ceil(70 / 64) images of 1 x 64."""
    B = b2s_common.rule_block(FC[1])
    return synth.shape("pw_fc_inner", -(-FC[1] // B), FC[2], 1, B, FC[3], 1, sparsity=0.7)


def emptied(w, s):
    """pw_g3's weights with group 0 and a row of group 1 emptied."""
    w = w.copy()
    mg = s.M // s.group
    w[:mg] = 0
    w[mg + 1] = 0
    return w


def chunks(s, synth, n=None):
    oh, ow = synth.out_hw(s)
    return -(-(s.N if n is None else n) * oh * ow // CHUNK)
