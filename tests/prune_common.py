"""Shared by the pruning tests (test_prune_host.py, test_prune_gpu.py, test_prune_rules_san.py): the selection rule of
include/escoin.h "Pruning" restated in numpy, and the scores the cases rank.  Imports nothing from the library.

The rule: key(s) = the bits of s with the sign bit cleared, an unsigned integer.  KEEP keeps the first min(keep, n)
entries of a STABLE sort by descending key (equal keys: the lower entry index first); THRESHOLD keeps key >= key(thr).
entry_map[e] = the entry's index among the kept ones, or -1."""
import numpy as np


def keys(score):
    s = np.ascontiguousarray(score)
    assert s.dtype in (np.float32, np.float64)
    u = s.view(np.uint32 if s.dtype == np.float32 else np.uint64)
    return u & (u.dtype.type(~u.dtype.type(0)) >> u.dtype.type(1))


def ref_kept(score, keep=None, threshold=None):
    """The boolean keep mask."""
    k = keys(score)
    n = k.size
    kept = np.zeros(n, bool)
    if keep is not None:
        order = np.argsort(np.iinfo(k.dtype).max - k, kind="stable")      # descending key, ascending index among equals
        kept[order[:min(int(keep), n)]] = True
    else:
        kept[:] = k >= keys(np.array([threshold], score.dtype))[0]
    return kept


def ref_map(score, keep=None, threshold=None):
    kept = ref_kept(score, keep, threshold)
    m = np.full(kept.size, -1, np.int32)
    m[kept] = np.arange(int(kept.sum()), dtype=np.int32)
    return m


def ref_csr(desc, rowptr, colidx, values, nnz_per_group, entry_map):
    """The CSR (get_csr()'s flat form) restricted to the entries the map keeps."""
    mg = desc.M // desc.group
    kept = np.asarray(entry_map) >= 0
    rp = np.zeros_like(rowptr)
    ng = np.zeros_like(nnz_per_group)
    base = 0
    for grp in range(desc.group):
        r = rowptr[grp * (mg + 1):(grp + 1) * (mg + 1)]
        n = int(nnz_per_group[grp])
        rows = np.repeat(np.arange(mg), np.diff(r))
        cnt = np.bincount(rows[kept[base:base + n]], minlength=mg)
        rp[grp * (mg + 1) + 1:(grp + 1) * (mg + 1)] = np.cumsum(cnt)
        ng[grp] = cnt.sum()
        base += n
    return rp, colidx[kept], values[kept], ng


def positions(desc, rowptr, colidx, nnz_per_group):
    """The flat index into blobs_[0] of every entry of a CSR in get_csr()'s form, in its order (ascending)."""
    mg, kdim = desc.M // desc.group, (desc.C // desc.group) * desc.KH * desc.KW
    out, base = [], 0
    for grp in range(desc.group):
        r = np.asarray(rowptr[grp * (mg + 1):(grp + 1) * (mg + 1)])
        n = int(nnz_per_group[grp])
        rows = np.repeat(np.arange(mg, dtype=np.int64), np.diff(r)) + grp * mg
        out.append(rows * kdim + np.asarray(colidx[base:base + n], np.int64))
        base += n
    pos = np.concatenate(out) if out else np.zeros(0, np.int64)
    assert np.all(np.diff(pos) > 0), "a CSR's positions ascend"
    return pos


def pattern_csr(desc, positions):
    """rowptr, colidx, nnz_per_group of the pattern that holds the given flat positions of blobs_[0] (ascending)."""
    mg, kdim = desc.M // desc.group, (desc.C // desc.group) * desc.KH * desc.KW
    pos = np.asarray(positions, np.int64)
    assert np.all(np.diff(pos) > 0) and (pos.size == 0 or pos[-1] < desc.M * kdim)
    rows, cols = pos // kdim, (pos % kdim).astype(np.int32)
    cnt = np.bincount(rows, minlength=desc.M).reshape(desc.group, mg)
    rp = np.zeros((desc.group, mg + 1), np.int32)
    rp[:, 1:] = np.cumsum(cnt, axis=1)
    return rp.ravel(), cols, cnt.sum(axis=1).astype(np.int32)


def masked_dense(desc, rowptr, colidx, values, nnz_per_group):
    """blobs_[0] with the CSR's values at its positions and +0 elsewhere."""
    mg, kdim = desc.M // desc.group, (desc.C // desc.group) * desc.KH * desc.KW
    w = np.zeros((desc.M, kdim), values.dtype)
    base = 0
    for grp in range(desc.group):
        r = rowptr[grp * (mg + 1):(grp + 1) * (mg + 1)]
        n = int(nnz_per_group[grp])
        rows = np.repeat(np.arange(mg), np.diff(r)) + grp * mg
        w[rows, colidx[base:base + n]] = values[base:base + n]
        base += n
    return w.reshape(desc.M, desc.C // desc.group, desc.KH, desc.KW)


def _from_bits(bits, dt):
    return np.ascontiguousarray(bits).view(dt)


def score_cases(n, dt, seed):
    """name -> n scores of dtype dt.  Each case is built so that a wrong tie rule, a floating-point comparison or a wrong
    digit pass of the radix select changes the keep set."""
    rs = np.random.RandomState(seed)
    dt = np.dtype(dt)
    ut = np.uint32 if dt == np.float32 else np.uint64
    nbytes = dt.itemsize
    out = {}
    # many equal magnitudes of both signs: any boundary inside a class is a tie boundary
    mags = np.array([0.125, 0.25, 0.5, 0.75, 1.0, 1.5], dt)
    out["ties"] = (mags[rs.randint(0, mags.size, n)] * rs.choice(np.array([-1, 1], dt), n)).astype(dt)
    # explicit +0.0 / -0.0, one NaN, +inf, -inf, denormals among ordinary values
    v = rs.uniform(-1, 1, n).astype(dt)
    v[v == 0] = 0.5
    tiny = np.finfo(dt).tiny
    special = [0.0, -0.0, np.nan, np.inf, -np.inf, tiny / 2, -tiny / 4, tiny / 2, np.nextafter(dt.type(0), dt.type(1)), -0.0, 0.0]
    where = rs.permutation(n)[:len(special)]
    v[where] = np.array(special[:where.size], dt)
    out["specials"] = v
    # scores that differ in ONE byte of the key only, each byte in turn (byte 0: the lowest mantissa byte; the top byte:
    # the high exponent bits, 7 bits wide since the sign is no part of the key).  Few distinct digits: ties straddle too.
    base = np.array([1.2345678901234567], dt).view(ut)[0]
    for j in range(nbytes):
        width = 7 if j == nbytes - 1 else 8
        digit = rs.randint(0, 1 << width, n).astype(ut)
        bits = (base & ~(ut(0xff) << ut(8 * j))) | (digit << ut(8 * j))
        sign = rs.randint(0, 2, n).astype(ut) << ut(8 * nbytes - 1)
        out["byte%d" % j] = _from_bits((bits | sign).astype(ut), dt)
    # all keys equal: only the entry index decides
    out["all_equal"] = (dt.type(0.37) * rs.choice(np.array([-1, 1], dt), n)).astype(dt)
    for name, s in out.items():
        assert s.dtype == dt and s.size == n, name
    return out


def tie_boundary_keep(score, near):
    """A keep count close to `near` whose boundary falls between two entries of EQUAL key (so the entry index decides),
    or `near` itself if the scores have no such boundary."""
    k = np.sort(keys(score))[::-1]
    n = k.size
    for d in range(n):
        for keep in (near - d, near + d):
            if 1 <= keep < n and k[keep - 1] == k[keep]:
                return int(keep)
    return int(near)
