"""The float64 reference and the derived per-element error bound of the suite (test_errbound_cpu.py, test_errbound_gpu.py):
skew, forward_bound, backward_bound, check, within and the three corruptions of the self-check.  The code and its
derivation are in tools/error_bound.py, which the two fuzzers share; this module gives it the name the tests use."""
import os
import sys

_TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if _TOOLS not in sys.path:
    sys.path.insert(0, _TOOLS)
from error_bound import (ROW_EXPONENTS, TINY, U32, U64, Skewed, accumulated_bound, backward_bound, check,  # noqa: E402,F401
                         corruption_target, drop_bias, forward_bound, gamma, leak_from, low_channels, row_nnz, skew,
                         swap_images, within)
