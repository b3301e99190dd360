"""Shared by test_dense_wgrad_host.py and test_dense_wgrad_gpu.py: the split rule of include/escoin.h "Dense weight
gradient" (csrc/align_rules.h dwg_plan) restated in Python.  Imports nothing from the library."""
TILE = 64             # output channels x columns of a workgroup's tile
CHUNK = 1024          # flattened (n, oh, ow) pixels per chunk
LDS = 2 * 2 * 32 * 65 * 4
RESIDENT_PER_CU = 4   # workgroups of the MFMA kernel a CU holds at once
MAX_ROUNDS = 4        # rounds of resident workgroups a split may ask for
SPLITS_PER_CHUNK = 512  # splits whose serial sum costs what one chunk of a workgroup's walk costs


def split_cost(tiles, chunks, span, n_cu):
    """The rule's cost of cutting `chunks` into spans of `span`, in 1 / 1024 chunk walks: the rounds of resident workgroups
    (what they fill, plus half of what the last round leaves empty; one at least) x the span, plus the sum's serial walk."""
    s = -(-chunks // span)
    resident = RESIDENT_PER_CU * max(n_cu, 1)
    filled, whole = tiles * s * 1024 // resident, -(-tiles * s // resident) * 1024
    return max(1024, (filled + whole) // 2) * span + (1024 // SPLITS_PER_CHUNK) * s


def rule(s, out_hw, n_cu, max_splits=0):
    """(mtiles, ktiles, chunks, span, splits, positions, slab_bytes) for a synth shape s whose output is out_hw."""
    oh, ow = out_hw
    mg, kdim = s.M // s.group, (s.C // s.group) * s.KH * s.KW
    mtiles, ktiles = -(-mg // TILE), -(-kdim // TILE)
    chunks = -(-s.N * oh * ow // CHUNK)
    tiles = s.group * mtiles * ktiles
    resident = RESIDENT_PER_CU * max(n_cu, 1)
    best = None
    for span in range(chunks, 0, -1):           # the longest span first: a later one must be strictly cheaper
        n = -(-chunks // span)
        if n > 1 and ((max_splits > 0 and n > max_splits) or tiles * n > MAX_ROUNDS * resident):
            continue
        cost = split_cost(tiles, chunks, span, n_cu)
        if best is None or cost < best[0]:
            best = (cost, span)
    span = best[1]
    splits = -(-chunks // span)
    return mtiles, ktiles, chunks, span, splits, s.M * kdim, 4 * splits * s.M * kdim
