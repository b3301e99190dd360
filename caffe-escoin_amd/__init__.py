"""caffe-escoin_amd: MI355X-native direct sparse convolution forward (Escoin's SCONV path).

The product is the C-ABI shared library ``libescoin_hip.so`` (hand-written HIP kernels for
gfx950, see ``csrc/`` and ``include/escoin.h``) plus the C++ Caffe-compatible Layer/Blob shim
in ``caffe_shim/``.  This Python module is only a ctypes binding of that C ABI, used by the
tests and ``bench.py``; torch supplies device memory, streams and ``torch.distributed`` --
plumbing, not the product.

No silent CPU fallback: if the library is missing, or no HIP device is visible, the GPU entry
points raise.  Caffe::CPU mode is its own explicit set of entry points (``Plan.weight_align_cpu`` /
``Plan.forward_cpu``), implemented in the same library and usable without a GPU.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import shard, synth  # noqa: F401  (re-exported)

_HERE = os.path.dirname(os.path.abspath(__file__))
# ESCOIN_LIB: A/B experiments against another build of the library
LIB_PATH = os.environ.get("ESCOIN_LIB") or os.path.join(_HERE, "libescoin_hip.so")

KERNEL_AUTO, KERNEL_GENERIC, KERNEL_TILED, KERNEL_DENSE, KERNEL_JIT = 0, 1, 2, 3, 4
WGRAD_AUTO, WGRAD_ENTRY, WGRAD_STAGED, WGRAD_MFMA = 0, 1, 2, 3   # option / stat "wgrad_kernel"
WGRAD_POINTWISE = 4    # stat "wgrad_kernel" only: the pointwise kernel of option "wgrad_pointwise" ran
BWD_MFMA = 5   # option "backward_kernel" / stat "bwd_data_kernel": the fp32-MFMA data-gradient kernel (never "kernel")
CONV_MODE_LOWERED_GEMM, CONV_MODE_LOWERED_SPARSE, CONV_MODE_SCONV, CONV_MODE_SCONV_PAR = 0, 1, 2, 3

# every symbol include/escoin.h declares (tests check the library exports all of them)
API_SYMBOLS = [
    "escoin_last_error", "escoin_device_count", "escoin_out_shape", "escoin_padded_len",
    "escoin_plan_create", "escoin_plan_destroy", "escoin_plan_set_option",
    "escoin_weight_align", "escoin_plan_set_csr", "escoin_plan_nnz", "escoin_plan_get_csr",
    "escoin_plan_workspace_bytes", "escoin_plan_kernel_name", "escoin_plan_tiling_info", "escoin_forward",
    "escoin_plan_export_aligned", "escoin_plan_import_aligned", "escoin_plan_import_aligned_dev", "escoin_plan_stat",
    "escoin_gpu_sconv", "escoin_gpu_stretch", "escoin_copy_input_data",
    "escoin_gpu_sparse_dense2csr", "escoin_gpu_sparse_csrmm",
    # Dtype = double
    "escoin_weight_align_f64", "escoin_plan_set_csr_f64", "escoin_plan_get_csr_f64", "escoin_forward_f64",
    "escoin_gpu_sconv_f64", "escoin_copy_input_data_f64", "escoin_gpu_sparse_csrmm_f64",
    "escoin_gpu_sparse_dense2csr_f64",
    # Caffe::CPU mode
    "escoin_cpu_kernel_name", "escoin_cpu_kernel_select", "escoin_weight_align_cpu", "escoin_weight_align_cpu_f64",
    "escoin_forward_cpu", "escoin_forward_cpu_f64", "escoin_cpu_sconv", "escoin_cpu_sconv_f64",
    "escoin_cpu_sparse_dense2csr", "escoin_cpu_sparse_dense2csr_f64",
    # Backward (pattern-preserving)
    "escoin_backward", "escoin_backward_f64", "escoin_backward_cpu", "escoin_backward_cpu_f64",
    "escoin_backward_values", "escoin_backward_values_f64", "escoin_backward_values_cpu", "escoin_backward_values_cpu_f64",
    # Weight updates in place
    "escoin_update_values", "escoin_update_values_f64", "escoin_plan_set_values", "escoin_plan_set_values_f64",
    "escoin_update_values_cpu", "escoin_update_values_cpu_f64",
    # Solver step
    "escoin_solver_step", "escoin_solver_step_f64", "escoin_solver_step_cpu", "escoin_solver_step_cpu_f64",
    "escoin_solver_array_step", "escoin_solver_array_step_f64", "escoin_solver_array_step_cpu", "escoin_solver_array_step_cpu_f64",
    # Pruning
    "escoin_plan_prune", "escoin_plan_prune_cpu", "escoin_compact_entries",
    # Rewiring
    "escoin_plan_rewire", "escoin_plan_rewire_cpu",
    # Dense weight gradient (rewire's grow score)
    "escoin_dense_wgrad", "escoin_dense_wgrad_f64", "escoin_dense_wgrad_cpu", "escoin_dense_wgrad_cpu_f64",
    # Space-to-depth (option "s2d")
    "escoin_plan_s2d_pack",
    # Space-to-batch (option "s2b")
    "escoin_plan_s2b_pack",
    "escoin_plan_s2b_unpack",
    # Batch-to-space (option "b2s")
    "escoin_plan_b2s_pack",
    "escoin_plan_b2s_unpack",
    # Deconvolution (option "deconv")
    "escoin_deconv_out_shape",
    "escoin_plan_d2s_pack",
    "escoin_plan_d2s_unpack",
]
SOLVER_SGD, SOLVER_NESTEROV, SOLVER_ADAM = 0, 1, 2
REG_NONE, REG_L2, REG_L1 = 0, 1, 2
PRUNE_KEEP, PRUNE_THRESHOLD = 0, 1


class EscoinError(RuntimeError):
    pass


class ConvDesc(C.Structure):
    """Mirror of escoin_conv_desc (include/escoin.h)."""
    _fields_ = [(n, C.c_int) for n in
                ("N", "C", "H", "W", "M", "KH", "KW", "pad_h", "pad_w", "stride_h", "stride_w",
                 "dil_h", "dil_w", "group", "has_bias", "fuse_relu")]

    @classmethod
    def from_shape(cls, s, N=None, fuse_relu=False):
        """From a synth.ConvShape."""
        return cls(s.N if N is None else N, s.C, s.H, s.W, s.M, s.KH, s.KW, s.pad_h, s.pad_w,
                   s.stride_h, s.stride_w, s.dil_h, s.dil_w, s.group, int(bool(s.bias)),
                   int(bool(fuse_relu)))

    @classmethod
    def inner_product(cls, N, K, M, bias=True, relu=False):
        """An InnerProduct layer of K inputs and M outputs at batch N: N images of K channels and one pixel, a 1x1 kernel
        (include/escoin.h "Batch-to-space")."""
        return cls(N, K, 1, 1, M, 1, 1, 0, 0, 1, 1, 1, 1, 1, int(bool(bias)), int(bool(relu)))

    @classmethod
    def deconvolution(cls, N, C, H, W, M, kernel, stride=1, pad=0, group=1, bias=True, relu=False):
        """A Deconvolution layer for Plan(..., deconv=1): C bottom channels of H x W, M = num_output; kernel, stride and
        pad as one int or an (h, w) pair (include/escoin.h "Deconvolution")."""
        def hw(v):
            return (int(v), int(v)) if np.isscalar(v) else (int(v[0]), int(v[1]))
        (kh, kw), (sh, sw), (ph, pw) = hw(kernel), hw(stride), hw(pad)
        return cls(N, C, H, W, M, kh, kw, ph, pw, sh, sw, 1, 1, group, int(bool(bias)), int(bool(relu)))


class SolverDesc(C.Structure):
    """Mirror of escoin_solver_desc (include/escoin.h "Solver step").  type / regularization also by name:
    SolverDesc.make(type="adam", regularization="L2", rate=1e-3, ...); rate_dev: an address, or a one-element tensor /
    array of the plan's Dtype (which the caller keeps alive)."""
    _fields_ = [("type", C.c_int), ("regularization", C.c_int), ("rate", C.c_double), ("momentum", C.c_double),
                ("momentum2", C.c_double), ("delta", C.c_double), ("decay", C.c_double), ("diff_scale", C.c_double),
                ("rate_dev", C.c_void_p), ("diff_is_dense", C.c_int), ("clear_diff", C.c_int)]
    TYPES = {"sgd": SOLVER_SGD, "nesterov": SOLVER_NESTEROV, "adam": SOLVER_ADAM}
    REGS = {"none": REG_NONE, "l2": REG_L2, "l1": REG_L1}

    @classmethod
    def make(cls, type=SOLVER_SGD, regularization=REG_NONE, rate=0.0, momentum=0.0, momentum2=0.999, delta=1e-8, decay=0.0,
             diff_scale=1.0, rate_dev=None, diff_is_dense=0, clear_diff=0):
        if isinstance(type, str):
            type = cls.TYPES[type.lower()]
        if isinstance(regularization, str):
            regularization = cls.REGS[regularization.lower()]
        if rate_dev is not None and not isinstance(rate_dev, int):
            rate_dev = rate_dev.data_ptr() if hasattr(rate_dev, "data_ptr") else rate_dev.ctypes.data
        return cls(int(type), int(regularization), rate, momentum, momentum2, delta, decay, diff_scale, rate_dev,
                   int(bool(diff_is_dense)), int(bool(clear_diff)))


class PruneDesc(C.Structure):
    """Mirror of escoin_prune_desc (include/escoin.h "Pruning")."""
    _fields_ = [("mode", C.c_int), ("keep", C.c_long), ("threshold", C.c_double), ("score", C.c_void_p)]


class RewireDesc(C.Structure):
    """Mirror of escoin_rewire_desc (include/escoin.h "Rewiring")."""
    _fields_ = [("drop", C.POINTER(PruneDesc)), ("grow", C.c_long), ("score", C.c_void_p), ("init", C.c_void_p)]


def compact_entries(entry_map, src, out=None, stream=None):
    """escoin_compact_entries: out[entry_map[e]] = src[e] wherever entry_map[e] >= 0.  entry_map (int32) and src (4- or
    8-byte elements) are both torch CUDA tensors (one launch on `stream`, default torch's current stream) or both numpy
    arrays (a host loop).  out: the destination (at least as many elements as the map keeps; never src itself); None = a
    new zeroed array of exactly the kept count, which costs a read of the map on the device route."""
    on_device = not isinstance(entry_map, np.ndarray)
    if on_device:
        import torch
        assert entry_map.is_cuda and entry_map.dtype == torch.int32 and entry_map.is_contiguous()
        assert src.is_cuda and src.is_contiguous() and src.element_size() in (4, 8) and src.numel() == entry_map.numel()
        if out is None:
            out = torch.zeros(int((entry_map >= 0).sum().item()), dtype=src.dtype, device=src.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == src.dtype
        if stream is None:
            stream = C.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)
        check(lib().escoin_compact_entries(C.c_void_p(entry_map.data_ptr()), entry_map.numel(), src.element_size(),
                                           C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr()), 1, stream),
              "escoin_compact_entries")
        return out
    m = np.ascontiguousarray(entry_map, np.int32)
    s = np.ascontiguousarray(src)
    assert s.dtype.itemsize in (4, 8) and s.size == m.size
    if out is None:
        out = np.zeros(int((m >= 0).sum()), s.dtype)
    assert out.dtype == s.dtype and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"] and out.size > (int(m.max()) if m.size else -1)
    check(lib().escoin_compact_entries(_np_ptr(m), m.size, s.dtype.itemsize, _np_ptr(s), _np_ptr(out), 0, None),
          "escoin_compact_entries")
    return out


def _solver_desc(desc, kw):
    if desc is not None and kw:
        raise EscoinError("solver step: pass a SolverDesc or keyword fields, not both")
    return desc if desc is not None else SolverDesc.make(**kw)


def _solver_arrays(arrays, on_device):
    """Checks one solver call's arrays (None allowed): all numpy or all torch CUDA, one dtype, contiguous (they are written
    in place).  Returns (their addresses, is_f64)."""
    some = [a for a in arrays if a is not None]
    if on_device:
        import torch
        assert all(a.is_cuda and a.is_contiguous() for a in some), "solver step: contiguous torch CUDA tensors"
        assert some[0].dtype in (torch.float32, torch.float64) and all(a.dtype == some[0].dtype for a in some)
        return [None if a is None else C.c_void_p(a.data_ptr()) for a in arrays], some[0].dtype == torch.float64
    assert all(isinstance(a, np.ndarray) and a.flags["C_CONTIGUOUS"] and a.flags["WRITEABLE"] for a in some), "solver step: contiguous numpy arrays"
    assert some[0].dtype in (np.float32, np.float64) and all(a.dtype == some[0].dtype for a in some)
    return [None if a is None else _np_ptr(a) for a in arrays], some[0].dtype == np.float64


def solver_array_step(data, diff, history, history2=None, stream=None, desc=None, **kw):
    """escoin_solver_array_step: the solver's rule on a plain blob (the bias), torch CUDA tensors updated in place on
    `stream` (default torch's current stream).  The rule: a SolverDesc, or its fields as keywords."""
    import torch
    d = _solver_desc(desc, kw)
    ptrs, f64 = _solver_arrays([data, diff, history, history2], True)
    if stream is None:
        stream = C.c_void_p(torch.cuda.current_stream(data.device).cuda_stream)
    fn = lib().escoin_solver_array_step_f64 if f64 else lib().escoin_solver_array_step
    check(fn(C.byref(d), data.numel(), *ptrs, stream), "escoin_solver_array_step")


def solver_array_step_cpu(data, diff, history, history2=None, desc=None, **kw):
    """escoin_solver_array_step_cpu: the same on numpy arrays, in place."""
    d = _solver_desc(desc, kw)
    ptrs, f64 = _solver_arrays([data, diff, history, history2], False)
    fn = lib().escoin_solver_array_step_cpu_f64 if f64 else lib().escoin_solver_array_step_cpu
    check(fn(C.byref(d), data.size, *ptrs), "escoin_solver_array_step_cpu")


def build(verbose=False):
    """Compile libescoin_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "-j4"], stdout=out)
    return LIB_PATH


_lib = None


def lib():
    """The loaded C-ABI library; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EscoinError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`"
                          " (there is no CPU fallback)" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, ip, cp = C.c_void_p, C.c_int, C.c_char_p
    dp = C.POINTER(ConvDesc)
    L.escoin_last_error.restype = cp
    L.escoin_last_error.argtypes = []
    L.escoin_device_count.restype = ip
    L.escoin_device_count.argtypes = []
    L.escoin_out_shape.restype = ip
    L.escoin_out_shape.argtypes = [dp, C.POINTER(ip), C.POINTER(ip)]
    L.escoin_padded_len.restype = C.c_long
    L.escoin_padded_len.argtypes = [dp]
    L.escoin_plan_create.restype = ip
    L.escoin_plan_create.argtypes = [dp, C.POINTER(vp)]
    L.escoin_plan_destroy.restype = ip
    L.escoin_plan_destroy.argtypes = [vp]
    L.escoin_plan_set_option.restype = ip
    L.escoin_plan_set_option.argtypes = [vp, cp, ip]
    L.escoin_weight_align.restype = ip
    L.escoin_weight_align.argtypes = [vp, vp, ip, vp]
    L.escoin_plan_set_csr.restype = ip
    L.escoin_plan_set_csr.argtypes = [vp, vp, vp, vp, vp, vp]
    L.escoin_plan_nnz.restype = C.c_long
    L.escoin_plan_nnz.argtypes = [vp, ip]
    L.escoin_plan_get_csr.restype = ip
    L.escoin_plan_get_csr.argtypes = [vp, vp, vp, vp, ip]
    L.escoin_plan_workspace_bytes.restype = C.c_size_t
    L.escoin_plan_workspace_bytes.argtypes = [vp]
    L.escoin_plan_kernel_name.restype = cp
    L.escoin_plan_kernel_name.argtypes = [vp]
    L.escoin_plan_tiling_info.restype = cp
    L.escoin_plan_tiling_info.argtypes = [vp]
    L.escoin_plan_s2d_pack.restype = ip
    L.escoin_plan_s2d_pack.argtypes = [vp, vp, ip, vp]
    L.escoin_plan_s2b_pack.restype = ip
    L.escoin_plan_s2b_pack.argtypes = [vp, vp, ip, vp]
    L.escoin_plan_s2b_unpack.restype = ip
    L.escoin_plan_s2b_unpack.argtypes = [vp, vp, ip, vp]
    L.escoin_plan_b2s_pack.restype = ip
    L.escoin_plan_b2s_pack.argtypes = [vp, vp, vp, vp, ip, ip, vp]
    L.escoin_plan_b2s_unpack.restype = ip
    L.escoin_plan_b2s_unpack.argtypes = [vp, vp, vp, ip, ip, ip, vp]
    L.escoin_deconv_out_shape.restype = ip
    L.escoin_deconv_out_shape.argtypes = [vp, vp, vp]
    L.escoin_plan_d2s_pack.restype = ip
    L.escoin_plan_d2s_pack.argtypes = [vp, vp, vp, vp, ip, vp]
    L.escoin_plan_d2s_unpack.restype = ip
    L.escoin_plan_d2s_unpack.argtypes = [vp, vp, vp, vp, ip, vp]
    L.escoin_forward.restype = ip
    L.escoin_forward.argtypes = [vp, vp, vp, vp, ip, vp]
    L.escoin_plan_export_aligned.restype = ip
    L.escoin_plan_export_aligned.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.escoin_plan_import_aligned.restype = ip
    L.escoin_plan_import_aligned.argtypes = [vp, vp, C.c_size_t, vp]
    L.escoin_plan_import_aligned_dev.restype = ip
    L.escoin_plan_import_aligned_dev.argtypes = [vp, vp, C.c_size_t, vp]
    L.escoin_plan_stat.restype = C.c_long
    L.escoin_plan_stat.argtypes = [vp, cp]
    L.escoin_gpu_sconv.restype = ip
    L.escoin_gpu_sconv.argtypes = [ip, ip, vp, ip, vp, vp, vp, vp] + [ip] * 10 + [vp, ip, ip, vp]
    L.escoin_gpu_stretch.restype = ip
    L.escoin_gpu_stretch.argtypes = [vp, vp] + [ip] * 7 + [vp]
    L.escoin_copy_input_data.restype = ip
    L.escoin_copy_input_data.argtypes = [vp, vp] + [ip] * 5 + [vp]
    L.escoin_gpu_sparse_dense2csr.restype = ip
    L.escoin_gpu_sparse_dense2csr.argtypes = [ip, ip, vp, vp, vp, vp, vp, C.POINTER(ip), vp]
    L.escoin_gpu_sparse_csrmm.restype = ip
    L.escoin_gpu_sparse_csrmm.argtypes = [ip, ip, ip, ip, C.c_float, vp, vp, vp, vp, C.c_float, vp, vp]
    for suffix in ("", "_f64"):
        real = C.c_float if suffix == "" else C.c_double
        f = getattr(L, "escoin_weight_align_cpu" + suffix)
        f.restype, f.argtypes = ip, [vp, vp]
        f = getattr(L, "escoin_forward_cpu" + suffix)
        f.restype, f.argtypes = ip, [vp, vp, vp, vp, ip, ip]
        f = getattr(L, "escoin_cpu_sconv" + suffix)
        f.restype, f.argtypes = ip, [vp] + [ip] * 9 + [vp, vp, vp, ip, ip, vp, vp, ip, ip]
        f = getattr(L, "escoin_cpu_sparse_dense2csr" + suffix)
        f.restype, f.argtypes = ip, [ip, ip, vp, vp, vp, vp]
        if suffix:
            L.escoin_weight_align_f64.restype = ip
            L.escoin_weight_align_f64.argtypes = [vp, vp, ip, vp]
            L.escoin_plan_set_csr_f64.restype = ip
            L.escoin_plan_set_csr_f64.argtypes = [vp, vp, vp, vp, vp, vp]
            L.escoin_plan_get_csr_f64.restype = ip
            L.escoin_plan_get_csr_f64.argtypes = [vp, vp, vp, vp, ip]
            L.escoin_forward_f64.restype = ip
            L.escoin_forward_f64.argtypes = [vp, vp, vp, vp, ip, vp]
            L.escoin_gpu_sconv_f64.restype = ip
            L.escoin_gpu_sconv_f64.argtypes = L.escoin_gpu_sconv.argtypes
            L.escoin_copy_input_data_f64.restype = ip
            L.escoin_copy_input_data_f64.argtypes = L.escoin_copy_input_data.argtypes
            L.escoin_gpu_sparse_dense2csr_f64.restype = ip
            L.escoin_gpu_sparse_dense2csr_f64.argtypes = L.escoin_gpu_sparse_dense2csr.argtypes
            L.escoin_gpu_sparse_csrmm_f64.restype = ip
            L.escoin_gpu_sparse_csrmm_f64.argtypes = [ip, ip, ip, ip, real, vp, vp, vp, vp, real, vp, vp]
    for name in ("escoin_backward", "escoin_backward_f64", "escoin_backward_cpu", "escoin_backward_cpu_f64",
                 "escoin_backward_values", "escoin_backward_values_f64", "escoin_backward_values_cpu",
                 "escoin_backward_values_cpu_f64"):
        f = getattr(L, name)
        f.restype, f.argtypes = ip, [vp] * 7 + [ip, vp if "cpu" not in name else ip]
    for name in ("escoin_update_values", "escoin_update_values_f64", "escoin_plan_set_values", "escoin_plan_set_values_f64"):
        f = getattr(L, name)
        f.restype, f.argtypes = ip, [vp, vp, ip, vp]
    for name in ("escoin_update_values_cpu", "escoin_update_values_cpu_f64"):
        f = getattr(L, name)
        f.restype, f.argtypes = ip, [vp, vp]
    sp = C.POINTER(SolverDesc)
    for suffix in ("", "_f64"):
        f = getattr(L, "escoin_solver_step" + suffix)
        f.restype, f.argtypes = ip, [vp, sp, vp, vp, vp, vp, vp]
        f = getattr(L, "escoin_solver_step_cpu" + suffix)
        f.restype, f.argtypes = ip, [vp, sp, vp, vp, vp, vp]
        f = getattr(L, "escoin_solver_array_step" + suffix)
        f.restype, f.argtypes = ip, [sp, C.c_long, vp, vp, vp, vp, vp]
        f = getattr(L, "escoin_solver_array_step_cpu" + suffix)
        f.restype, f.argtypes = ip, [sp, C.c_long, vp, vp, vp, vp]
    pp = C.POINTER(PruneDesc)
    L.escoin_plan_prune.restype = ip
    L.escoin_plan_prune.argtypes = [vp, pp, vp, C.POINTER(C.c_long), vp]
    L.escoin_plan_prune_cpu.restype = ip
    L.escoin_plan_prune_cpu.argtypes = [vp, pp, vp, C.POINTER(C.c_long)]
    rp = C.POINTER(RewireDesc)
    L.escoin_plan_rewire.restype = ip
    L.escoin_plan_rewire.argtypes = [vp, rp, vp, vp, C.POINTER(C.c_long), C.POINTER(C.c_long), vp]
    L.escoin_plan_rewire_cpu.restype = ip
    L.escoin_plan_rewire_cpu.argtypes = [vp, rp, vp, vp, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    for name in ("escoin_dense_wgrad", "escoin_dense_wgrad_f64", "escoin_dense_wgrad_cpu", "escoin_dense_wgrad_cpu_f64"):
        f = getattr(L, name)
        f.restype, f.argtypes = ip, [vp] * 5 + [ip, ip, vp if "cpu" not in name else ip]
    L.escoin_compact_entries.restype = ip
    L.escoin_compact_entries.argtypes = [vp, C.c_long, ip, vp, vp, ip, vp]
    L.escoin_cpu_kernel_name.restype = cp
    L.escoin_cpu_kernel_name.argtypes = []
    L.escoin_cpu_kernel_select.restype = ip
    L.escoin_cpu_kernel_select.argtypes = [cp]
    _lib = L
    return L


def check(rc, what="escoin call"):
    if rc != 0:
        raise EscoinError("%s failed (%d): %s" % (what, rc, lib().escoin_last_error().decode()))


def device_count():
    return lib().escoin_device_count()


def cpu_kernel_select(which):
    """Pin the host kernel's flavour ("avx2", "avx512", "auto"); raises when this CPU lacks it."""
    check(lib().escoin_cpu_kernel_select(which.encode()), "escoin_cpu_kernel_select(%s)" % which)


def cpu_kernel_name():
    """Which flavour of the host kernel Caffe::CPU mode runs on this machine."""
    return lib().escoin_cpu_kernel_name().decode()


def out_shape(desc):
    oh, ow = C.c_int(), C.c_int()
    check(lib().escoin_out_shape(C.byref(desc), C.byref(oh), C.byref(ow)), "escoin_out_shape")
    return oh.value, ow.value


def deconv_out_shape(desc):
    """The top image of the Deconvolution layer `desc` describes: stride * (in - 1) + kernel - 2 * pad per axis."""
    oh, ow = C.c_int(), C.c_int()
    check(lib().escoin_deconv_out_shape(C.byref(desc), C.byref(oh), C.byref(ow)), "escoin_deconv_out_shape")
    return oh.value, ow.value


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Plan(object):
    """escoin_plan: one ConvolutionLayer's sparse state (CSR + weight streams) on one device."""

    def __init__(self, desc, kernel=KERNEL_AUTO, conv_mode=CONV_MODE_SCONV_PAR, **options):
        self.desc = desc
        self._h = C.c_void_p()
        check(lib().escoin_plan_create(C.byref(desc), C.byref(self._h)), "escoin_plan_create")
        if kernel != KERNEL_AUTO:
            self.set_option("kernel", kernel)
        if conv_mode != CONV_MODE_SCONV_PAR:
            self.set_option("conv_mode", conv_mode)
        for k, v in options.items():      # e.g. tiling_batch=256, dense_gate=1, dense_threshold_pct=30
            self.set_option(k, v)
        # option "deconv": the descriptor is a Deconvolution layer's -- another top image, and blobs_[0] is C x M/g x KH x KW
        self.deconv = bool(options.get("deconv", 0))
        self.out_hw = deconv_out_shape(desc) if self.deconv else out_shape(desc)

    def close(self):
        if self._h:
            lib().escoin_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, key, value):
        check(lib().escoin_plan_set_option(self._h, key.encode(), int(value)),
              "escoin_plan_set_option(%s)" % key)

    def weight_align(self, dense_w, stream=None):
        """WeightAlign().  dense_w: numpy (host) or torch CUDA tensor (device), M x C/g x KH x KW;
        float64 input makes a Dtype = double plan (escoin_weight_align_f64)."""
        if isinstance(dense_w, np.ndarray):
            f64 = dense_w.dtype == np.float64
            w = np.ascontiguousarray(dense_w, np.float64 if f64 else np.float32)
            fn = lib().escoin_weight_align_f64 if f64 else lib().escoin_weight_align
            check(fn(self._h, _np_ptr(w), 0, stream), "escoin_weight_align")
        else:
            w = dense_w.contiguous()
            assert w.is_cuda and w.dtype.is_floating_point and w.element_size() in (4, 8)
            fn = lib().escoin_weight_align_f64 if w.element_size() == 8 else lib().escoin_weight_align
            check(fn(self._h, C.c_void_p(w.data_ptr()), 1, stream), "escoin_weight_align")

    # ---- weight updates in place (include/escoin.h "Weight updates") -----------------------------------------------------
    def _update(self, a, dense, stream):
        base = "escoin_update_values" if dense else "escoin_plan_set_values"
        if isinstance(a, np.ndarray):
            f64 = a.dtype == np.float64
            w = np.ascontiguousarray(a, np.float64 if f64 else np.float32)
            check(getattr(lib(), base + ("_f64" if f64 else ""))(self._h, _np_ptr(w), 0, stream), base)
            return
        import torch
        w = a.contiguous()
        assert w.is_cuda and w.dtype in (torch.float32, torch.float64)
        if stream is None:
            stream = C.c_void_p(torch.cuda.current_stream(w.device).cuda_stream)
        check(getattr(lib(), base + ("_f64" if w.element_size() == 8 else ""))(self._h, C.c_void_p(w.data_ptr()), 1, stream), base)

    def update_values(self, dense_w, stream=None):
        """New weights at the old pattern, in place.  dense_w: blobs_[0] as numpy (host) or a torch CUDA tensor (device:
        asynchronous on `stream`, default torch's current stream); read at the plan's CSR positions only."""
        self._update(dense_w, True, stream)

    def set_values(self, values, stream=None):
        """The same from the compact value array (nnz elements in get_csr()'s order), numpy or torch CUDA."""
        self._update(values, False, stream)

    def update_values_cpu(self, dense_w):
        """update_values for a plan aligned by weight_align_cpu (host CSR only); float32 or float64 numpy."""
        f64 = dense_w.dtype == np.float64
        w = np.ascontiguousarray(dense_w, np.float64 if f64 else np.float32)
        fn = lib().escoin_update_values_cpu_f64 if f64 else lib().escoin_update_values_cpu
        check(fn(self._h, _np_ptr(w)), "escoin_update_values_cpu")

    # ---- solver step (include/escoin.h "Solver step") ---------------------------------------------------------------------
    def solver_step(self, diff, history, history2=None, dense_w=None, stream=None, desc=None, **kw):
        """The solver's rule and the in-place update in one launch, on torch CUDA tensors (all updated in place),
        asynchronous on `stream` (default torch's current stream).  diff: values_diff (1-D, nnz elements, get_csr()'s
        order) or, with diff_is_dense=1, a blobs_[0]-shaped weight_diff; history / history2: nnz elements; dense_w:
        blobs_[0], which receives the new values at the pattern.  The rule: a SolverDesc, or its fields as keywords
        (type="sgd" | "nesterov" | "adam", regularization, rate, momentum, momentum2, delta, decay, diff_scale, rate_dev,
        diff_is_dense, clear_diff)."""
        import torch
        d = _solver_desc(desc, kw)
        ptrs, f64 = _solver_arrays([diff, history, history2, dense_w], True)
        n = self.nnz()
        assert diff.numel() == (self.desc.M * int(np.prod(self._grad_shapes())) if d.diff_is_dense else n), "diff: wrong size for its layout"
        assert history.numel() == n and (history2 is None or history2.numel() == n), "history: nnz elements"
        assert dense_w is None or dense_w.numel() == self.desc.M * int(np.prod(self._grad_shapes())), "dense_w: blobs_[0]'s size"
        if stream is None:
            stream = C.c_void_p(torch.cuda.current_stream(diff.device).cuda_stream)
        fn = lib().escoin_solver_step_f64 if f64 else lib().escoin_solver_step
        check(fn(self._h, C.byref(d), *ptrs, stream), "escoin_solver_step")

    def solver_step_cpu(self, diff, history, history2=None, dense_w=None, desc=None, **kw):
        """solver_step for a plan aligned by weight_align_cpu, on numpy arrays (updated in place)."""
        d = _solver_desc(desc, kw)
        ptrs, f64 = _solver_arrays([diff, history, history2, dense_w], False)
        n = self.nnz()
        assert diff.size == (self.desc.M * int(np.prod(self._grad_shapes())) if d.diff_is_dense else n), "diff: wrong size for its layout"
        assert history.size == n and (history2 is None or history2.size == n), "history: nnz elements"
        assert dense_w is None or dense_w.size == self.desc.M * int(np.prod(self._grad_shapes())), "dense_w: blobs_[0]'s size"
        fn = lib().escoin_solver_step_cpu_f64 if f64 else lib().escoin_solver_step_cpu
        check(fn(self._h, C.byref(d), *ptrs), "escoin_solver_step_cpu")

    # ---- pruning (include/escoin.h "Pruning") ------------------------------------------------------------------------------
    def _prune_desc(self, keep, sparsity, threshold):
        if sum(a is not None for a in (keep, sparsity, threshold)) != 1:
            raise EscoinError("prune: give exactly one of keep, sparsity, threshold")
        if sparsity is not None:
            d = self.desc
            keep = int(round((1.0 - float(sparsity)) * d.M * (d.C // d.group) * d.KH * d.KW))
        if keep is not None:
            return PruneDesc(PRUNE_KEEP, int(keep), 0.0, None)
        return PruneDesc(PRUNE_THRESHOLD, 0, float(threshold), None)

    def prune(self, keep=None, sparsity=None, threshold=None, score=None, stream=None):
        """escoin_plan_prune: drops all but the `keep` largest-magnitude entries (or those below `threshold`) of a
        device-aligned plan and re-aligns it on the rest.  sparsity: keep = round((1 - sparsity) * M * Cg * KH * KW).
        score: a torch CUDA tensor of nnz elements of the plan's dtype in get_csr()'s order to rank instead of the
        values.  Returns entry_map, an int32 torch CUDA tensor of the old nnz elements: the entry's new index, or -1.
        Synchronises `stream` (default torch's current stream); not capturable."""
        import torch
        d = self._prune_desc(keep, sparsity, threshold)
        n = self.nnz()
        dev = torch.device("cuda", torch.cuda.current_device()) if score is None else score.device
        if score is not None:
            want = torch.float64 if self.stat("is_f64") == 1 else torch.float32
            assert score.is_cuda and score.is_contiguous() and score.dtype == want and score.numel() == n, "score: nnz elements of the plan's dtype"
            d.score = score.data_ptr()
        entry_map = torch.empty(n, dtype=torch.int32, device=dev)
        if stream is None:
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        new_nnz = C.c_long()
        check(lib().escoin_plan_prune(self._h, C.byref(d), C.c_void_p(entry_map.data_ptr()) if n else None, C.byref(new_nnz), stream),
              "escoin_plan_prune")
        return entry_map

    def prune_cpu(self, keep=None, sparsity=None, threshold=None, score=None):
        """escoin_plan_prune_cpu: the same for a plan aligned by weight_align_cpu; score and the returned entry_map are
        numpy arrays."""
        d = self._prune_desc(keep, sparsity, threshold)
        n = self.nnz()
        s = None
        if score is not None:
            s = np.ascontiguousarray(score, np.float64 if self.stat("is_f64") == 1 else np.float32)
            assert s.size == n, "score: nnz elements"
            d.score = s.ctypes.data
        entry_map = np.empty(n, np.int32)
        new_nnz = C.c_long()
        check(lib().escoin_plan_prune_cpu(self._h, C.byref(d), _np_ptr(entry_map), C.byref(new_nnz)), "escoin_plan_prune_cpu")
        return entry_map

    # ---- rewiring (include/escoin.h "Rewiring") ---------------------------------------------------------------------------
    def _dense_size(self):
        d = self.desc
        return d.M * (d.C // d.group) * d.KH * d.KW

    def _rewire_drop(self, drop_keep, drop_sparsity, drop_threshold, drop_score):
        if drop_keep is None and drop_sparsity is None and drop_threshold is None:
            if drop_score is not None:
                raise EscoinError("rewire: drop_score needs one of drop_keep, drop_sparsity, drop_threshold")
            return None
        return self._prune_desc(drop_keep, drop_sparsity, drop_threshold)

    def rewire(self, grow, score, init=None, drop_keep=None, drop_sparsity=None, drop_threshold=None, drop_score=None, stream=None):
        """escoin_plan_rewire: drops entries by escoin_plan_prune's rule (drop_keep / drop_sparsity / drop_threshold, ranked
        on the values or on drop_score, nnz elements; none given: nothing is dropped), grows the `grow` positions outside
        the pattern where |score| is largest, and re-aligns the device-aligned plan ONCE.  score, init: torch CUDA tensors
        of M * Cg * KH * KW elements of the plan's dtype (score may be None iff grow == 0; init None: grown entries are
        +0.0).  Returns (entry_map, grown): int32 torch CUDA tensors of the old nnz (new index, or -1) and of n_grown
        elements (the new indices of the grown positions, ascending).  Synchronises `stream` (default torch's current
        stream); not capturable."""
        import torch
        want = torch.float64 if self.stat("is_f64") == 1 else torch.float32
        n, D = self.nnz(), self._dense_size()
        dev = torch.device("cuda", torch.cuda.current_device())
        drop = self._rewire_drop(drop_keep, drop_sparsity, drop_threshold, drop_score)
        if drop_score is not None:
            assert drop_score.is_cuda and drop_score.is_contiguous() and drop_score.dtype == want and drop_score.numel() == n, "drop_score: nnz elements of the plan's dtype"
            drop.score = drop_score.data_ptr()
        d = RewireDesc(C.pointer(drop) if drop is not None else None, int(grow), None, None)
        for name, t in (("score", score), ("init", init)):
            if t is not None:
                assert t.is_cuda and t.is_contiguous() and t.dtype == want and t.numel() == D, name + ": M * Cg * KH * KW elements of the plan's dtype"
                setattr(d, name, t.data_ptr())
                dev = t.device
        entry_map = torch.empty(n, dtype=torch.int32, device=dev)
        grown = torch.empty(max(min(int(grow), D - n), 0), dtype=torch.int32, device=dev)      # n_grown = min(grow, D - nnz)
        if stream is None:
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        new_nnz, n_grown = C.c_long(), C.c_long()
        check(lib().escoin_plan_rewire(self._h, C.byref(d), C.c_void_p(entry_map.data_ptr()) if n else None,
                                       C.c_void_p(grown.data_ptr()) if grown.numel() else None, C.byref(new_nnz), C.byref(n_grown), stream),
              "escoin_plan_rewire")
        return entry_map, grown[:n_grown.value]

    def rewire_cpu(self, grow, score, init=None, drop_keep=None, drop_sparsity=None, drop_threshold=None, drop_score=None):
        """escoin_plan_rewire_cpu: the same for a plan aligned by weight_align_cpu; score, init, drop_score and the
        returned (entry_map, grown) are numpy arrays."""
        dt = np.float64 if self.stat("is_f64") == 1 else np.float32
        n, D = self.nnz(), self._dense_size()
        drop = self._rewire_drop(drop_keep, drop_sparsity, drop_threshold, drop_score)
        keep_alive = []
        if drop_score is not None:
            ds = np.ascontiguousarray(drop_score, dt)
            assert ds.size == n, "drop_score: nnz elements"
            keep_alive.append(ds)
            drop.score = ds.ctypes.data
        d = RewireDesc(C.pointer(drop) if drop is not None else None, int(grow), None, None)
        for name, a in (("score", score), ("init", init)):
            if a is not None:
                a = np.ascontiguousarray(a, dt)
                assert a.size == D, name + ": M * Cg * KH * KW elements"
                keep_alive.append(a)
                setattr(d, name, a.ctypes.data)
        entry_map = np.empty(n, np.int32)
        grown = np.empty(max(min(int(grow), D - n), 0), np.int32)      # n_grown = min(grow, D - nnz)
        new_nnz, n_grown = C.c_long(), C.c_long()
        check(lib().escoin_plan_rewire_cpu(self._h, C.byref(d), _np_ptr(entry_map), _np_ptr(grown), C.byref(new_nnz), C.byref(n_grown)),
              "escoin_plan_rewire_cpu")
        return entry_map, grown[:n_grown.value]

    # ---- dense weight gradient (include/escoin.h "Dense weight gradient") -------------------------------------------------
    def dense_wgrad(self, top_diff, bottom, top=None, out=None, accumulate=False, n_images=None, stream=None):
        """escoin_dense_wgrad: the dense M x Cg x KH x KW weight gradient -- every position of blobs_[0], inside and
        outside the pattern -- on torch CUDA tensors, asynchronous on `stream` (default torch's current stream).  top: the
        forward's top blob (fuse_relu plans).  out: the tensor to write (accumulate=True: to add onto); None = a new one.
        n_images: the leading images to reduce over (default all of top_diff's).  The result is what rewire() takes as
        score=."""
        import torch
        d = self.desc
        g = top_diff
        dt = g.dtype
        assert g.is_cuda and dt in (torch.float32, torch.float64) and g.is_contiguous()
        assert tuple(g.shape[1:]) == (d.M,) + tuple(self.out_hw), "top_diff shape mismatch"
        n = g.shape[0] if n_images is None else int(n_images)
        for t in (bottom, top):
            if t is not None:
                assert t.is_cuda and t.dtype == dt and t.is_contiguous() and t.shape[0] >= min(n, g.shape[0])
        shape = (d.M,) + self._grad_shapes()
        if out is None:
            if accumulate:
                raise EscoinError("dense_wgrad: accumulate needs the blob to add onto (out=)")
            out = torch.empty(shape, device=g.device, dtype=dt)
        assert out.is_cuda and out.dtype == dt and out.is_contiguous() and tuple(out.shape) == shape, "out: wrong dtype / shape / layout"

        def _p(t):
            return C.c_void_p(t.data_ptr()) if t is not None else None

        if stream is None:
            stream = C.c_void_p(torch.cuda.current_stream(g.device).cuda_stream)
        fn = lib().escoin_dense_wgrad_f64 if dt == torch.float64 else lib().escoin_dense_wgrad
        check(fn(self._h, _p(bottom), _p(top), _p(g), _p(out), n, int(bool(accumulate)), stream), "escoin_dense_wgrad")
        return out

    def dense_wgrad_cpu(self, top_diff, bottom, top=None, out=None, accumulate=False, n_images=None, n_threads=0):
        """escoin_dense_wgrad_cpu: the same on numpy arrays (float32 or float64, matching the aligned weights), on any plan
        with a host CSR."""
        d = self.desc
        f64 = top_diff.dtype == np.float64
        dt = np.float64 if f64 else np.float32
        g = np.ascontiguousarray(top_diff, dt)
        assert tuple(g.shape[1:]) == (d.M,) + tuple(self.out_hw), "top_diff shape mismatch"
        n = g.shape[0] if n_images is None else int(n_images)
        x = None if bottom is None else np.ascontiguousarray(bottom, dt)
        t = None if top is None else np.ascontiguousarray(top, dt)
        shape = (d.M,) + self._grad_shapes()
        if out is None:
            if accumulate:
                raise EscoinError("dense_wgrad_cpu: accumulate needs the blob to add onto (out=)")
            out = np.empty(shape, dt)
        assert out.dtype == dt and out.flags["C_CONTIGUOUS"] and tuple(out.shape) == shape, "out: wrong dtype / shape / layout"

        def _p(a):
            return _np_ptr(a) if a is not None else None

        fn = lib().escoin_dense_wgrad_cpu_f64 if f64 else lib().escoin_dense_wgrad_cpu
        check(fn(self._h, _p(x), _p(t), _p(g), _p(out), n, int(bool(accumulate)), int(n_threads)), "escoin_dense_wgrad_cpu")
        return out

    # ---- Caffe::CPU mode (no device needed) ----------------------------------------------------
    def weight_align_cpu(self, dense_w):
        """WeightAlign() in CPU mode: host CSR only.  float32 or float64 numpy."""
        f64 = dense_w.dtype == np.float64
        w = np.ascontiguousarray(dense_w, np.float64 if f64 else np.float32)
        fn = lib().escoin_weight_align_cpu_f64 if f64 else lib().escoin_weight_align_cpu
        check(fn(self._h, _np_ptr(w)), "escoin_weight_align_cpu")

    def forward_cpu(self, bottom, bias=None, n_threads=0, out=None):
        """Forward_cpu on numpy arrays (float32 or float64, matching the aligned weights).  `out`: a C-contiguous top
        blob to write into (a Caffe top blob is allocated once at Reshape, not per Forward)."""
        d = self.desc
        f64 = bottom.dtype == np.float64
        dt = np.float64 if f64 else np.float32
        x = np.ascontiguousarray(bottom, dt)
        assert tuple(x.shape[1:]) == (d.C, d.H, d.W), "bottom shape mismatch"
        b = None if bias is None else np.ascontiguousarray(bias, dt)
        shape = (x.shape[0], d.M) + tuple(self.out_hw)
        if out is None:
            top = np.empty(shape, dt)
        else:
            assert out.dtype == dt and tuple(out.shape) == shape and out.flags["C_CONTIGUOUS"], "out: wrong dtype / shape / layout"
            top = out
        fn = lib().escoin_forward_cpu_f64 if f64 else lib().escoin_forward_cpu
        check(fn(self._h, _np_ptr(x), _np_ptr(b) if b is not None else None, _np_ptr(top), x.shape[0],
                 int(n_threads)), "escoin_forward_cpu")
        return top

    def set_csr(self, rowptr, colidx, values, nnz_per_group, stream=None):
        rp = np.ascontiguousarray(rowptr, np.int32)
        ci = np.ascontiguousarray(colidx, np.int32)
        f64 = isinstance(values, np.ndarray) and values.dtype == np.float64
        va = np.ascontiguousarray(values, np.float64 if f64 else np.float32)
        ng = np.ascontiguousarray(nnz_per_group, np.int32)
        fn = lib().escoin_plan_set_csr_f64 if f64 else lib().escoin_plan_set_csr
        check(fn(self._h, _np_ptr(rp), _np_ptr(ci), _np_ptr(va), _np_ptr(ng), stream), "escoin_plan_set_csr")

    def nnz(self, group=-1):
        n = lib().escoin_plan_nnz(self._h, group)
        if n < 0:
            check(int(n), "escoin_plan_nnz")
        return int(n)

    def get_csr(self, stretched=False):
        d = self.desc
        mg = (d.C if self.deconv else d.M) // d.group      # (a "deconv" plan's rows are the bottom's channels)
        nnz = self.nnz()
        f64 = self.stat("is_f64") == 1
        rp = np.zeros(d.group * (mg + 1), np.int32)
        ci = np.zeros(max(nnz, 1), np.int32)
        va = np.zeros(max(nnz, 1), np.float64 if f64 else np.float32)
        fn = lib().escoin_plan_get_csr_f64 if f64 else lib().escoin_plan_get_csr
        check(fn(self._h, _np_ptr(rp), _np_ptr(ci), _np_ptr(va), int(stretched)), "escoin_plan_get_csr")
        ng = np.array([self.nnz(g) for g in range(d.group)], np.int32)
        return rp, ci[:nnz], va[:nnz], ng

    def export_aligned(self):
        """The aligned form (CSR + channel deal + unit table + code object) as a numpy uint8 array."""
        n = C.c_size_t()
        check(lib().escoin_plan_export_aligned(self._h, None, 0, C.byref(n)), "escoin_plan_export_aligned")
        buf = np.zeros(n.value, np.uint8)
        check(lib().escoin_plan_export_aligned(self._h, _np_ptr(buf), buf.size, C.byref(n)),
              "escoin_plan_export_aligned")
        return buf[:n.value]

    def import_aligned(self, blob, stream=None):
        """Restore what export_aligned wrote; True when the persisted code object was loaded as it was.
        blob: numpy uint8 (host), or a torch CUDA uint8 tensor -- the buffer an RCCL broadcast filled -- which is
        handed over as it is (escoin_plan_import_aligned_dev: no .cpu().numpy() round trip)."""
        if not isinstance(blob, np.ndarray) and getattr(blob, "is_cuda", False):
            t = blob.contiguous()
            assert t.element_size() == 1
            check(lib().escoin_plan_import_aligned_dev(self._h, C.c_void_p(t.data_ptr()), t.numel(), stream),
                  "escoin_plan_import_aligned_dev")
            return self.stat("import_fast") == 1
        b = np.ascontiguousarray(blob, np.uint8)
        check(lib().escoin_plan_import_aligned(self._h, _np_ptr(b), b.size, stream), "escoin_plan_import_aligned")
        return self.stat("import_fast") == 1

    def stat(self, key):
        v = lib().escoin_plan_stat(self._h, key.encode())
        if v < 0:
            check(int(v), "escoin_plan_stat(%s)" % key)
        return int(v)

    @property
    def align_ms(self):
        return self.stat("align_us") * 1e-3

    @property
    def workspace_bytes(self):
        return int(lib().escoin_plan_workspace_bytes(self._h))

    @property
    def kernel_name(self):
        return lib().escoin_plan_kernel_name(self._h).decode()

    @property
    def tiling_info(self):
        """How the fast kernel tiles the layer (one line; "" for the generic / dense / lowered kernels)."""
        return lib().escoin_plan_tiling_info(self._h).decode()

    def forward_ptr(self, bottom_ptr, bias_ptr, top_ptr, n_images, stream=None):
        """Raw-pointer Forward_gpu (device pointers as ints)."""
        check(lib().escoin_forward(self._h, C.c_void_p(bottom_ptr),
                                   C.c_void_p(bias_ptr) if bias_ptr else None,
                                   C.c_void_p(top_ptr), int(n_images), stream), "escoin_forward")

    def s2d_pack(self, bottom):
        """The space-to-depth rearrangement of an "s2d" plan alone, into the plan's scratch, on torch's current stream
        (what forward() runs before the inner plan; for measuring it)."""
        import torch
        d = self.desc
        assert bottom.is_cuda and bottom.dtype == torch.float32 and bottom.is_contiguous()
        assert tuple(bottom.shape[1:]) == (d.C, d.H, d.W), "bottom shape mismatch"
        stream = C.c_void_p(torch.cuda.current_stream(bottom.device).cuda_stream)
        check(lib().escoin_plan_s2d_pack(self._h, C.c_void_p(bottom.data_ptr()), int(bottom.shape[0]), stream), "escoin_plan_s2d_pack")

    def s2b_pack(self, bottom):
        """The space-to-batch rearrangement of an "s2b" plan alone, into the plan's X' scratch, on torch's current stream
        (what forward() runs before the inner plan; for measuring it)."""
        import torch
        d = self.desc
        assert bottom.is_cuda and bottom.dtype == torch.float32 and bottom.is_contiguous()
        assert tuple(bottom.shape[1:]) == (d.C, d.H, d.W), "bottom shape mismatch"
        stream = C.c_void_p(torch.cuda.current_stream(bottom.device).cuda_stream)
        check(lib().escoin_plan_s2b_pack(self._h, C.c_void_p(bottom.data_ptr()), int(bottom.shape[0]), stream), "escoin_plan_s2b_pack")

    def s2b_unpack(self, top):
        """The batch-to-space rearrangement of an "s2b" plan alone, from the plan's T' scratch (whatever it holds) into `top`
        (N x M x OH x OW), on torch's current stream (what forward() runs after the inner plan; for measuring it)."""
        import torch
        d = self.desc
        assert top.is_cuda and top.dtype == torch.float32 and top.is_contiguous()
        assert tuple(top.shape[1:]) == (d.M,) + tuple(self.out_hw), "top shape mismatch"
        stream = C.c_void_p(torch.cuda.current_stream(top.device).cuda_stream)
        check(lib().escoin_plan_s2b_unpack(self._h, C.c_void_p(top.data_ptr()), int(top.shape[0]), stream), "escoin_plan_s2b_unpack")

    def d2s_unpack(self, top, bias=None, src=None, n_images=None):
        """The unpack kernel of a "deconv" plan alone, on torch's current stream: the top blob from T' (src: N x M*P x H' x W';
        default: the plan's scratch, as the last forward's inner launch left it), + bias, through ReLU on a fuse_relu plan."""
        import torch
        for t in (top,) + tuple(x for x in (bias, src) if x is not None):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        n = int(top.shape[0]) if n_images is None else int(n_images)
        d = self.desc
        assert top.numel() >= n * d.M * self.out_hw[0] * self.out_hw[1], "top too small"
        stream = C.c_void_p(torch.cuda.current_stream(top.device).cuda_stream)
        check(lib().escoin_plan_d2s_unpack(self._h, None if src is None else C.c_void_p(src.data_ptr()),
                                           None if bias is None else C.c_void_p(bias.data_ptr()), C.c_void_p(top.data_ptr()), n, stream),
              "escoin_plan_d2s_unpack")

    def d2s_pack(self, top_diff, top=None, dst=None, n_images=None):
        """The pack kernel of a "deconv" plan alone: G' (dst: N x M*P x H' x W'; default: the plan's scratch) from top_diff,
        gated by top > 0 on a fuse_relu plan."""
        import torch
        for t in (top_diff,) + tuple(x for x in (top, dst) if x is not None):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        n = int(top_diff.shape[0]) if n_images is None else int(n_images)
        stream = C.c_void_p(torch.cuda.current_stream(top_diff.device).cuda_stream)
        check(lib().escoin_plan_d2s_pack(self._h, C.c_void_p(top_diff.data_ptr()), None if top is None else C.c_void_p(top.data_ptr()),
                                         None if dst is None else C.c_void_p(dst.data_ptr()), n, stream), "escoin_plan_d2s_pack")

    def b2s_pack(self, src, dst, mask=None, top_side=False, n_images=None):
        """One transpose of a "b2s" plan alone, on the caller's tensors and torch's current stream: src (N x CH, CH = M on
        the top side, C on the bottom side; gated by mask > 0 where mask is given) into dst, the ceil(n_images / B) x CH x B
        inner blob (at least that many elements; the rest of dst is left alone)."""
        import torch
        for t in (src, dst) + (() if mask is None else (mask,)):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        n = int(src.shape[0]) if n_images is None else int(n_images)
        ch = self.desc.M if top_side else self.desc.C
        blk = self.stat("b2s_block")
        assert src.numel() >= n * ch and (mask is None or mask.numel() >= n * ch), "src / mask too small"
        assert blk <= 0 or dst.numel() >= -(-n // blk) * ch * blk, "dst too small"
        stream = C.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)
        check(lib().escoin_plan_b2s_pack(self._h, C.c_void_p(src.data_ptr()), None if mask is None else C.c_void_p(mask.data_ptr()),
                                         C.c_void_p(dst.data_ptr()), int(bool(top_side)), n, stream), "escoin_plan_b2s_pack")

    def b2s_unpack(self, src, dst, top_side=False, relu=False, n_images=None):
        """The reverse transpose of a "b2s" plan alone: src, an inner blob as b2s_pack writes it, into the first n_images
        rows of dst (N x CH), through ReLU if asked."""
        import torch
        for t in (src, dst):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        n = int(dst.shape[0]) if n_images is None else int(n_images)
        ch = self.desc.M if top_side else self.desc.C
        blk = self.stat("b2s_block")
        assert dst.numel() >= n * ch, "dst too small"
        assert blk <= 0 or src.numel() >= -(-n // blk) * ch * blk, "src too small"
        stream = C.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)
        check(lib().escoin_plan_b2s_unpack(self._h, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), int(bool(top_side)),
                                           int(bool(relu)), n, stream), "escoin_plan_b2s_unpack")

    def forward(self, bottom, bias=None, top=None):
        """Forward_gpu on torch CUDA tensors (float32, or float64 for a double plan), on torch's current stream."""
        import torch
        d = self.desc
        dt = bottom.dtype
        assert bottom.is_cuda and dt in (torch.float32, torch.float64) and bottom.is_contiguous()
        n = bottom.shape[0]
        assert tuple(bottom.shape[1:]) == (d.C, d.H, d.W), "bottom shape mismatch"
        if top is None:
            top = torch.empty((n, d.M) + tuple(self.out_hw), device=bottom.device, dtype=dt)
        assert top.is_contiguous() and top.dtype == dt and tuple(top.shape) == (n, d.M) + tuple(self.out_hw)
        if bias is not None:
            assert bias.is_cuda and bias.dtype == dt and bias.numel() == d.M
        stream = C.c_void_p(torch.cuda.current_stream(bottom.device).cuda_stream)
        if dt == torch.float64:
            check(lib().escoin_forward_f64(self._h, C.c_void_p(bottom.data_ptr()),
                                           C.c_void_p(bias.data_ptr()) if bias is not None else None,
                                           C.c_void_p(top.data_ptr()), int(n), stream), "escoin_forward_f64")
            return top
        self.forward_ptr(bottom.data_ptr(), bias.data_ptr() if bias is not None else 0,
                         top.data_ptr(), n, stream)
        return top

    # ---- Backward (pattern-preserving; include/escoin.h "Backward") ----------------------------------------------------
    def _grad_shapes(self):
        d = self.desc
        return (d.C // d.group, d.KH, d.KW)

    def _weight_shape(self):
        """blobs_[0]: M x C/g x KH x KW, or C x M/g x KH x KW on a "deconv" plan."""
        d = self.desc
        return (d.C, d.M // d.group, d.KH, d.KW) if self.deconv else (d.M,) + self._grad_shapes()

    def backward(self, top_diff, bottom=None, top=None, bottom_diff=True, weight_diff=None, bias_diff=None,
                 values_diff=None):
        """Backward_gpu on torch CUDA tensors, on torch's current stream.  bottom_diff: True = a new tensor, a tensor =
        written (overwritten) in place, None / False = not computed.  weight_diff / bias_diff: True = a new zeroed tensor,
        a tensor = accumulated into (+=, at the CSR positions only for the weights), None / False = not computed.
        values_diff (instead of weight_diff): the weight gradient in compact form, a 1-D tensor of nnz elements in
        get_csr()'s order -- the order set_values() reads; True / tensor / None as for weight_diff.
        Returns (bottom_diff, weight_diff or values_diff, bias_diff)."""
        import torch
        d = self.desc
        g = top_diff
        dt = g.dtype
        assert g.is_cuda and dt in (torch.float32, torch.float64) and g.is_contiguous()
        n = g.shape[0]
        assert tuple(g.shape[1:]) == (d.M,) + tuple(self.out_hw), "top_diff shape mismatch"

        def _new_or(t, shape, zero):
            if t is None or t is False:
                return None
            if t is True:
                return (torch.zeros if zero else torch.empty)(shape, device=g.device, dtype=dt)
            assert t.is_cuda and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == tuple(shape)
            return t

        compact = values_diff is not None and values_diff is not False
        if compact and weight_diff is not None and weight_diff is not False:
            raise EscoinError("backward: weight_diff and values_diff are two layouts of one gradient: ask for one")
        bd = _new_or(bottom_diff, (n, d.C, d.H, d.W), False)
        wd = _new_or(values_diff, (self.nnz(),), True) if compact else _new_or(weight_diff, self._weight_shape(), True)
        bsd = _new_or(bias_diff, (d.M,), True)
        for t in (bottom, top):
            if t is not None:
                assert t.is_cuda and t.dtype == dt and t.is_contiguous()

        def _p(t):
            return C.c_void_p(t.data_ptr()) if t is not None else None

        stream = C.c_void_p(torch.cuda.current_stream(g.device).cuda_stream)
        fn = getattr(lib(), "escoin_backward" + ("_values" if compact else "") + ("_f64" if dt == torch.float64 else ""))
        check(fn(self._h, _p(bottom), _p(top), _p(g), _p(bd), _p(wd), _p(bsd), int(n), stream), "escoin_backward")
        return bd, wd, bsd

    def backward_cpu(self, top_diff, bottom=None, top=None, bottom_diff=True, weight_diff=None, bias_diff=None,
                     n_threads=0, values_diff=None):
        """Backward_cpu on numpy arrays (float32 or float64, matching the aligned weights); arguments and result as in
        backward()."""
        d = self.desc
        f64 = top_diff.dtype == np.float64
        dt = np.float64 if f64 else np.float32
        g = np.ascontiguousarray(top_diff, dt)
        n = g.shape[0]
        assert tuple(g.shape[1:]) == (d.M,) + tuple(self.out_hw), "top_diff shape mismatch"

        def _new_or(t, shape, zero):
            if t is None or t is False:
                return None
            if t is True:
                return (np.zeros if zero else np.empty)(shape, dt)
            assert t.dtype == dt and t.flags["C_CONTIGUOUS"] and tuple(t.shape) == tuple(shape)
            return t

        compact = values_diff is not None and values_diff is not False
        if compact and weight_diff is not None and weight_diff is not False:
            raise EscoinError("backward_cpu: weight_diff and values_diff are two layouts of one gradient: ask for one")
        bd = _new_or(bottom_diff, (n, d.C, d.H, d.W), False)
        wd = _new_or(values_diff, (self.nnz(),), True) if compact else _new_or(weight_diff, self._weight_shape(), True)
        bsd = _new_or(bias_diff, (d.M,), True)
        x = None if bottom is None else np.ascontiguousarray(bottom, dt)
        t = None if top is None else np.ascontiguousarray(top, dt)

        def _p(a):
            return _np_ptr(a) if a is not None else None

        fn = getattr(lib(), "escoin_backward" + ("_values" if compact else "") + "_cpu" + ("_f64" if f64 else ""))
        check(fn(self._h, _p(x), _p(t), _p(g), _p(bd), _p(wd), _p(bsd), int(n), int(n_threads)), "escoin_backward_cpu")
        return bd, wd, bsd
