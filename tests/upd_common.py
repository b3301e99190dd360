"""Shared by the weight-update tests (test_update_values_cpu.py, test_update_values_gpu.py): the new weights of a case."""
import numpy as np


def new_weights(w, seed, zeros=True, mask=None):
    """The old blob with every nonzero (or, with `mask`, every position of the mask: the pattern of a plan that already
    holds explicit zeros) replaced by a seeded random value -- with `zeros`, a few of them exactly 0 and one
    -0.0 (explicit zeros of the pattern) -- and the same blob with NaN at every position outside the pattern (an update
    must not read those).  Returns (w_new, w_new_with_nan_outside)."""
    rs = np.random.RandomState(seed)
    mask = (w != 0) if mask is None else mask
    v = rs.uniform(-1, 1, w.shape).astype(w.dtype)
    v[v == 0] = 0.5
    idx = np.flatnonzero(mask.ravel())
    if zeros and idx.size >= 8:
        pick = rs.choice(idx, size=min(5, idx.size // 2), replace=False)
        flat = v.ravel()
        flat[pick[1:]] = 0.0
        flat[pick[0]] = -0.0
    w_new = np.where(mask, v, w.dtype.type(0)).astype(w.dtype)
    w_nan = np.where(mask, v, w.dtype.type(np.nan)).astype(w.dtype)
    return w_new, w_nan


def values_at(plan, w_new):
    """w_new's values at the plan's CSR positions, in get_csr()'s order (bits kept: -0.0 stays -0.0)."""
    d = plan.desc
    mg, kdim = d.M // d.group, (d.C // d.group) * d.KH * d.KW
    rp, ci, _, ng = plan.get_csr()
    flat = np.ascontiguousarray(w_new).reshape(d.M, kdim)
    out = np.empty(ci.size, w_new.dtype)
    base = 0
    for grp in range(d.group):
        r = rp[grp * (mg + 1):(grp + 1) * (mg + 1)]
        rows = np.repeat(np.arange(mg), np.diff(r)) + grp * mg
        n = int(ng[grp])
        out[base:base + n] = flat[rows, ci[base:base + n]]
        base += n
    return rp, ci, out, ng


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
