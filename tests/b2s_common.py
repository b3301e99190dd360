"""Plan option "b2s" (include/escoin.h "Batch-to-space"), for test_b2s_host.py, test_b2s_gpu.py and test_b2s_sequence_gpu.py:
the inner-product shapes, the block rule and the two transposes restated in numpy from the header alone."""
import numpy as np

MAX_INNER_IMAGES = 65535
TILE = 64                # the edge of b2s.hip's LDS tile: shapes named 63 / 64 / 65 sit one below, at and one above it


def ip_shape(synth, name, N, K, M, group=1, bias=True, sparsity=0.6):
    """An InnerProduct layer of K inputs and M outputs at batch N: N images of K channels and one pixel, a 1x1 kernel."""
    return synth.shape(name, N, K, 1, 1, M, 1, group=group, bias=bias, sparsity=sparsity)


# name -> (N, K, M, group, bias, sparsity): odd sizes, no multiple of the tile or of the block, more than one inner image
# under the rule (N > 64), group 2, M of 1 / 10 / 65
SHAPES = {
    "ip_small": (6, 40, 10, 1, True, 0.6),
    "ip_m1": (9, 33, 1, 1, True, 0.5),
    "ip_m65": (65, 70, 65, 1, False, 0.7),
    "ip_g2": (70, 48, 26, 2, True, 0.6),
    "ip_wide": (130, 96, 24, 1, True, 0.8),
}


def make(synth, name):
    N, K, M, group, bias, sparsity = SHAPES[name]
    return ip_shape(synth, name, N, K, M, group, bias, sparsity)


def rule_block(N):
    """The shipped rule: 64; where that gives more than 65535 inner images, the smaller of 128 and 256 that does not.
    None: no block serves the batch."""
    for B in (64, 128, 256):
        if -(-N // B) <= MAX_INNER_IMAGES:
            return B
    return None


def plan_row(s, block=0, f64=False):
    """b2s_plan's output line (tests/cpp/b2s_plan_check.cpp) for a shape, from include/escoin.h alone: [0] where the option
    does not serve it."""
    if f64 or (s.H, s.W, s.KH, s.KW, s.pad_h, s.pad_w) != (1, 1, 1, 1, 0, 0):
        return [0]
    B = block or rule_block(s.N)
    if B is None or B % 4 or not 4 <= B <= 256:
        return [0]
    np_ = -(-s.N // B)
    x_floats, t_floats = np_ * s.C * B, np_ * s.M * B
    if np_ > MAX_INNER_IMAGES or x_floats >= 2 ** 31 or t_floats >= 2 ** 31:
        return [0]
    return [1, B, x_floats, t_floats, np_, s.C, 1, B, s.M, 1, 1, 0, 0, 1, 1, 1, 1, s.group, int(bool(s.bias)), 0]


def pack(a, B, n_images, mask=None, out=None):
    """inner[n'][ch][j] = a[n' * B + j][ch] (mask > 0 ? that : 0) for n' * B + j < n_images, +0 for the rest of the
    ceil(n_images / B) touched inner images; `out` (flat, any length at least that) keeps what lies past them."""
    ch = a.shape[1]
    touched = -(-n_images // B)
    v = a[:n_images].astype(np.float32)
    if mask is not None:
        with np.errstate(invalid="ignore"):
            v = np.where(mask[:n_images] > 0, v, np.float32(0))
    full = np.zeros((touched * B, ch), np.float32)
    full[:n_images] = v
    inner = np.ascontiguousarray(full.reshape(touched, B, ch).transpose(0, 2, 1))
    if out is None:
        return inner
    res = out.copy().reshape(-1)
    res[:inner.size] = inner.reshape(-1)
    return res


def unpack(inner_flat, B, n_images, ch, relu=False, out=None):
    """out[n][c] = inner[n / B][c][n % B] for n < n_images (v > 0 ? v : 0 with relu); the rows of `out` at or past n_images
    are kept."""
    touched = -(-n_images // B)
    inner = inner_flat.reshape(-1)[:touched * ch * B].reshape(touched, ch, B)
    rows = inner.transpose(0, 2, 1).reshape(touched * B, ch)[:n_images]
    if relu:
        with np.errstate(invalid="ignore"):
            rows = np.where(rows > 0, rows, np.float32(0))
    res = out.copy()
    res[:n_images] = rows
    return res
