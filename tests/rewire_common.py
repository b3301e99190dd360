"""Shared by the rewiring tests (test_rewire_host.py, test_rewire_gpu.py): the rule of include/escoin.h "Rewiring"
restated in numpy.  Imports nothing from the library.

The rule: a position is p = oc * kdim + colidx, D = M * kdim of them.  The drop is prune_common's rule over the entries.
The candidates are the positions outside the OLD pattern; they are ordered by a STABLE sort on descending integer key of
score[p] (equal keys: the lower position first) and the first min(grow, D - nnz) are grown.  The new pattern is kept +
grown in ascending p; kept entries keep their bits, grown entries are +0.0 or init[p]."""
import os
import re

import numpy as np

import prune_common as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tile_positions():
    """The positions one workgroup of the count / map kernels covers per step (csrc/prune_rules.h, which rewire_rules.h
    takes its tiles from), the scanning workgroup's width and the grid cap."""
    with open(os.path.join(ROOT, "caffe-escoin_amd", "csrc", "prune_rules.h")) as f:
        text = f.read()
    threads = int(re.search(r"kThreads = (\d+);", text).group(1))
    items = int(re.search(r"kItems = (\d+);", text).group(1))
    max_grid = int(re.search(r"kMaxGrid = (\d+);", text).group(1))
    return threads * items, threads, max_grid


def score_cases(D, dt, seed):
    """prune_common's score cases over the D dense positions: ties of both signs, +-0 / NaN / +-inf / denormals, a deciding
    difference in each key byte in turn, all keys equal."""
    return pc.score_cases(D, dt, seed)


def dense_size(desc):
    return desc.M * (desc.C // desc.group) * desc.KH * desc.KW


def candidates(D, pos):
    free = np.ones(D, bool)
    free[pos] = False
    return np.flatnonzero(free)


def ref_grown(score, pos, grow):
    """The grown positions, ascending."""
    score = np.ascontiguousarray(score).ravel()
    cand = candidates(score.size, pos)
    k = pc.keys(score[cand])
    order = np.argsort(np.iinfo(k.dtype).max - k, kind="stable")       # descending key, ascending position among equals
    return np.sort(cand[order[:min(int(grow), cand.size)]])


def ref_rewire(desc, csr, grow, score, init=None, drop_keep=None, drop_threshold=None, drop_score=None):
    """csr: get_csr()'s (rowptr, colidx, values, nnz_per_group).  Returns a dict: entry_map, grown (int32), grown_pos,
    csr (the new CSR in the same form), pos (the new pattern's positions)."""
    rp, ci, va, ng = csr
    pos = pc.positions(desc, rp, ci, ng)
    D = dense_size(desc)
    kept = np.ones(pos.size, bool)
    if drop_keep is not None or drop_threshold is not None:
        s = va if drop_score is None else drop_score
        kept = pc.ref_kept(s, drop_keep, None if drop_threshold is None else va.dtype.type(drop_threshold))
    grown_pos = ref_grown(score, pos, grow) if grow > 0 else np.zeros(0, np.int64)
    new_pos = np.sort(np.concatenate([pos[kept], grown_pos]))
    entry_map = np.full(pos.size, -1, np.int32)
    entry_map[kept] = np.searchsorted(new_pos, pos[kept]).astype(np.int32)
    grown = np.searchsorted(new_pos, grown_pos).astype(np.int32)
    values = np.zeros(new_pos.size, va.dtype)                              # +0.0
    values[entry_map[kept]] = va[kept]
    if init is not None:
        values[grown] = np.ascontiguousarray(init).ravel()[grown_pos]
    n_rp, n_ci, n_ng = pc.pattern_csr(desc, new_pos)
    assert new_pos.size == int(kept.sum()) + min(int(grow), D - pos.size)
    return dict(entry_map=entry_map, grown=grown, grown_pos=grown_pos, csr=(n_rp, n_ci, values, n_ng), pos=new_pos)


def grow_counts(score, pos):
    """0, 1, a count whose boundary falls between two candidates of equal key, every candidate, more than that."""
    score = np.ascontiguousarray(score).ravel()
    cand = candidates(score.size, pos)
    n = cand.size
    tie = pc.tie_boundary_keep(score[cand], max(n // 2, 1)) if n > 1 else 0
    return sorted(set([0, 1, tie, n, n + 7]))


def reindex(entry_map, new_nnz, arr):
    """What escoin_compact_entries into zeros gives: kept entries carry their element, grown ones start at +0."""
    out = np.zeros(new_nnz, arr.dtype)
    kept = entry_map >= 0
    out[entry_map[kept]] = arr[kept]
    return out
