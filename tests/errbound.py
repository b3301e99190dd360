"""The float64 reference and the derived per-element error bound of the suite (test_errbound_cpu.py, test_errbound_gpu.py):
skew, forward_bound, backward_bound, check, within, the three corruptions of the self-check, and the inputs, flush
models and reach sets of the fp32-edge tests (test_fp32_edges_cpu.py, test_fp32_edges_gpu.py).  The code and its
derivation are in tools/error_bound.py, which the two fuzzers share; this module gives it the name the tests use."""
import os
import sys

_TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if _TOOLS not in sys.path:
    sys.path.insert(0, _TOOLS)
from error_bound import (EDGE_KINDS, ROW_EXPONENTS, SUB_W_PATTERNS, TINY, TINY64, U32, U64, Edge, Skewed,  # noqa: E402,F401
                         accumulated_bound, backward_bound, check, conv64, corruption_target, drop_bias, edge_inputs, flush_inputs,
                         flush_results, forward_bound, gamma, leak_from, low_channels, poison_positions,
                         poison_positions_top, poisoned, reach_data, reach_data_dense, reach_forward, reach_forward_dense,
                         row_nnz, skew, swap_images, tiny, within)
