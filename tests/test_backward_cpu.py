"""Pattern-preserving Backward in Caffe::CPU mode (escoin_backward_cpu[_f64]), without a GPU: every golden geometry
against torch float64 autograd with the weight gradient masked by the pattern, accumulation and argument rules,
thread-count independence, explicit zeros in a handed-over CSR."""
import numpy as np
import pytest

from conftest import Golden, golden_params, rel_err

torch = pytest.importorskip("torch")
F = torch.nn.functional

from wgrad_common import EDGES, csr_positions, edge_inputs, torch_backward  # noqa: E402


def _seeded(shape, seed, dt):
    return np.random.RandomState(seed).uniform(-1, 1, shape).astype(dt)


def _check(pkg, gd, dt, has_bias, relu, n_threads=3):
    tol = 1e-12 if dt == np.float64 else 1e-4
    x, w = gd.x.astype(dt), gd.w.astype(dt)
    bias = None if (gd.bias is None or not has_bias) else gd.bias.astype(dt)
    desc = gd.desc(pkg, fuse_relu=relu)
    desc.has_bias = int(bias is not None)
    plan = pkg.Plan(desc)
    plan.weight_align_cpu(w)
    top = plan.forward_cpu(x, bias, n_threads=2) if relu else None
    oh, ow = plan.out_hw
    td = _seeded((gd.N, gd.M, oh, ow), 7, dt)
    bd, wd, bsd = plan.backward_cpu(td, bottom=x, top=top, weight_diff=True,
                                    bias_diff=True if bias is not None else None, n_threads=n_threads)
    want_bd, want_wd, want_bsd = torch_backward(x, w, bias, gd, td, top)
    assert bd.dtype == dt and wd.dtype == dt
    assert rel_err(bd, want_bd) <= tol, rel_err(bd, want_bd)
    assert rel_err(wd, want_wd) <= tol, rel_err(wd, want_wd)
    assert np.all(wd[w == 0] == 0)
    if bias is not None:
        assert rel_err(bsd, want_bsd) <= tol
    plan.close()


@pytest.mark.parametrize("path", golden_params())
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["float", "double"])
def test_backward_cpu_goldens_match_torch(pkg, path, dt):
    gd = Golden(path)
    _check(pkg, gd, dt, has_bias=True, relu=False)
    _check(pkg, gd, dt, has_bias=False, relu=True)


def _desc(pkg, N, C, H, W, M, K, pad, stride, dil, group, bias=1, relu=0, KW=None, pad_w=None):
    KW = K if KW is None else KW
    pad_w = pad if pad_w is None else pad_w
    return pkg.ConvDesc(N, C, H, W, M, K, KW, pad, pad_w, stride, stride, dil, dil, group, bias, relu)


def _pruned(shape, seed, keep, dt=np.float32):
    rs = np.random.RandomState(seed)
    w = rs.uniform(-1, 1, shape).astype(dt)
    w[rs.uniform(0, 1, shape) >= keep] = 0
    return w


def test_unpruned_weight_gradient_equals_torch_full_gradient(pkg):
    d = _desc(pkg, 2, 6, 9, 8, 4, 3, 1, 2, 1, 2)
    w = _seeded((4, 3, 3, 3), 1, np.float64) + 2.0      # no zero anywhere
    x = _seeded((2, 6, 9, 8), 2, np.float64)
    plan = pkg.Plan(d)
    plan.weight_align_cpu(w)
    td = _seeded((2, 4) + plan.out_hw, 3, np.float64)
    _, wd, _ = plan.backward_cpu(td, bottom=x, bottom_diff=None, weight_diff=True)
    X = torch.tensor(x)
    Wt = torch.tensor(w, requires_grad=True)
    F.conv2d(X, Wt, None, stride=2, padding=1, groups=2).backward(torch.tensor(td))
    assert rel_err(wd, Wt.grad.numpy()) <= 1e-12


def test_accumulation_nan_prefill_and_null_outputs(pkg):
    d = _desc(pkg, 2, 4, 7, 7, 6, 3, 1, 1, 1, 1)
    w = _pruned((6, 4, 3, 3), 4, 0.4)
    x = _seeded((2, 4, 7, 7), 5, np.float32)
    plan = pkg.Plan(d)
    plan.weight_align_cpu(w)
    td = _seeded((2, 6) + plan.out_hw, 6, np.float32)
    bd0, wd0, bsd0 = plan.backward_cpu(td, bottom=x, weight_diff=True, bias_diff=True)
    # += on weight_diff / bias_diff, only at the CSR positions: pruned positions prefilled with NaN stay NaN
    wd = np.where(w == 0, np.float32(np.nan), np.float32(0.5)).astype(np.float32)
    bsd = np.full(6, 0.25, np.float32)
    bd = np.full((2, 4, 7, 7), np.nan, np.float32)                  # bottom_diff is overwritten
    plan.backward_cpu(td, bottom=x, bottom_diff=bd, weight_diff=wd, bias_diff=bsd)
    assert np.array_equal(bd, bd0)
    assert np.all(np.isnan(wd[w == 0]))
    assert np.array_equal(wd[w != 0], (np.float32(0.5) + wd0[w != 0]).astype(np.float32))
    assert np.array_equal(bsd, (np.float32(0.25) + bsd0).astype(np.float32))
    # NULL outputs are skipped (no bottom needed without the weight gradient)
    bd1, wd1, bsd1 = plan.backward_cpu(td, bottom_diff=None, weight_diff=None, bias_diff=True)
    assert bd1 is None and wd1 is None and np.array_equal(bsd1, bsd0)
    bd2, _, _ = plan.backward_cpu(td)
    assert np.array_equal(bd2, bd0)
    plan.close()


def test_argument_and_state_errors(pkg):
    import ctypes as C
    L = pkg.lib()
    d = _desc(pkg, 2, 4, 7, 7, 6, 3, 1, 1, 1, 1, relu=1)
    plan = pkg.Plan(d)
    buf = np.zeros(4096, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    # before align
    assert L.escoin_backward_cpu(plan._h, p, p, p, p, None, None, 1, 1) == -4
    plan.weight_align_cpu(_pruned((6, 4, 3, 3), 4, 0.4))
    # wrong dtype
    assert L.escoin_backward_cpu_f64(plan._h, p, p, p, p, None, None, 1, 1) == -4
    assert L.escoin_backward_cpu(plan._h, p, p, None, p, None, None, 1, 1) == -1      # no top_diff
    assert L.escoin_backward_cpu(plan._h, p, None, p, p, None, None, 1, 1) == -1      # fuse_relu without top
    assert L.escoin_backward_cpu(plan._h, None, p, p, None, p, None, 1, 1) == -1      # weight_diff without bottom
    assert L.escoin_backward_cpu(plan._h, p, p, p, p, None, None, -1, 1) == -1        # n_images < 0
    assert L.escoin_backward_cpu(plan._h, p, p, p, p, p, p, 0, 1) == 0                # nothing to do
    assert L.escoin_backward_cpu(None, p, p, p, p, None, None, 1, 1) == -1
    plan.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["float", "double"])
def test_thread_count_and_repeated_calls_give_identical_bits(pkg, dt):
    d = _desc(pkg, 3, 8, 11, 10, 12, 3, 2, 1, 2, 2, relu=1)
    w = _pruned((12, 4, 3, 3), 8, 0.3, dt)
    x = _seeded((3, 8, 11, 10), 9, dt)
    b = _seeded((12,), 10, dt)
    plan = pkg.Plan(d)
    plan.weight_align_cpu(w)
    top = plan.forward_cpu(x, b)
    td = _seeded((3, 12) + plan.out_hw, 11, dt)
    runs = [plan.backward_cpu(td, bottom=x, top=top, weight_diff=True, bias_diff=True, n_threads=n) for n in (1, 7, 7, 0)]
    for r in runs[1:]:
        for a, b_ in zip(runs[0], r):
            assert a.tobytes() == b_.tobytes()
    plan.close()


@pytest.mark.gpu
def test_explicit_zeros_handed_to_set_csr_receive_a_gradient(pkg):
    """set_csr keeps explicit zeros: they are positions of the pattern and get their gradient.  (set_csr aligns on the
    device, hence the mark; the backward under test is the host one, on the host CSR a device align keeps.)"""
    d = _desc(pkg, 1, 2, 5, 5, 2, 3, 1, 1, 1, 1, bias=0)
    plan = pkg.Plan(d)
    rowptr = np.array([0, 2, 3], np.int32)
    colidx = np.array([0, 4, 13], np.int32)
    vals = np.array([0.0, 1.5, 0.0], np.float32)       # two explicit zeros
    plan.set_csr(rowptr, colidx, vals, [3])
    x = _seeded((1, 2, 5, 5), 12, np.float32)
    td = _seeded((1, 2, 5, 5), 13, np.float32)
    _, wd, _ = plan.backward_cpu(td, bottom=x, bottom_diff=None, weight_diff=True)
    X = torch.tensor(x.astype(np.float64))
    w = np.zeros((2, 2, 3, 3))
    Wt = torch.tensor(w, requires_grad=True)
    F.conv2d(X, Wt, None, padding=1).backward(torch.tensor(td.astype(np.float64)))
    full = Wt.grad.numpy().reshape(2, -1)
    flat = wd.reshape(2, -1)
    for oc, col in ((0, 0), (0, 4), (1, 13)):
        assert flat[oc, col] != 0 and abs(flat[oc, col] - full[oc, col]) <= 1e-4 * np.abs(full).max()
    mask = np.zeros_like(flat, bool)
    mask[0, 0] = mask[0, 4] = mask[1, 13] = True
    assert np.all(flat[~mask] == 0)
    plan.close()


@pytest.mark.parametrize("name", list(EDGES))
def test_directed_edges_match_torch(pkg, name):
    """The shapes test_backward_gpu.py runs on the device kernels (wgrad_common.EDGES), through backward_cpu: more than
    32767 output channels per group, transposed pads 0 and 4, partial batches with fuse_relu, padding beyond the kernel's
    reach and none, a conv group without a nonzero."""
    synth = pkg.synth
    s, w, x, b = edge_inputs(synth, name)
    relu = name == "relu3x3_n7"
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu))
    plan.weight_align_cpu(w)
    top = plan.forward_cpu(x, b) if relu else None
    td = _seeded((s.N, s.M) + plan.out_hw, 21, np.float32)
    full = None
    for n in ((s.N, 1, 3, 6) if relu else (s.N,)):
        tp = None if top is None else top[:n]
        bd, wd, bsd = plan.backward_cpu(td[:n], bottom=x[:n], top=tp, weight_diff=True, bias_diff=True)
        want = torch_backward(x[:n], w, b, s, td[:n], tp)
        for got, ref in zip((bd, wd, bsd), want):
            assert rel_err(got, ref) <= 1e-4, (name, n, rel_err(got, ref))
        assert np.all(wd[w == 0] == 0)
        full = bd if full is None else full
        assert bd.tobytes() == full[:n].tobytes()
        _, vd, _ = plan.backward_cpu(td[:n], bottom=x[:n], top=tp, bottom_diff=None, values_diff=True)
        assert vd.tobytes() == wd.reshape(-1)[csr_positions(plan)].tobytes()
    plan.close()
