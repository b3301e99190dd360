"""The compact weight gradient in Caffe::CPU mode (escoin_backward_values_cpu[_f64]), without a GPU: values_diff is the
dense weight_diff gathered at the CSR positions bit for bit, accumulates, keeps explicit zeros, and follows
escoin_backward_cpu's argument rules."""
import numpy as np
import pytest

from conftest import Golden, golden_params, rel_err

torch = pytest.importorskip("torch")

from wgrad_common import SHAPES, csr_positions, make_shape, seeded, torch_backward  # noqa: E402


def _both(pkg, desc, w, x, bias, relu, dt):
    plan = pkg.Plan(desc)
    plan.weight_align_cpu(w.astype(dt))
    x = x.astype(dt)
    b = None if bias is None else bias.astype(dt)
    top = plan.forward_cpu(x, b, n_threads=2) if relu else None
    td = seeded((x.shape[0], desc.M) + tuple(plan.out_hw), 7, dt)
    _, wd, bsd = plan.backward_cpu(td, bottom=x, top=top, bottom_diff=None, weight_diff=True, bias_diff=True, n_threads=3)
    _, vd, bsd2 = plan.backward_cpu(td, bottom=x, top=top, bottom_diff=None, values_diff=True, bias_diff=True, n_threads=2)
    pos = csr_positions(plan)
    assert vd.dtype == dt and vd.shape == (plan.nnz(),)
    assert vd.tobytes() == wd.reshape(-1)[pos].tobytes()
    assert bsd.tobytes() == bsd2.tobytes()
    assert np.count_nonzero(wd) <= len(pos)
    # += : a second call doubles
    plan.backward_cpu(td, bottom=x, top=top, bottom_diff=None, values_diff=vd)
    assert vd.tobytes() == (wd.reshape(-1)[pos] * dt(2)).tobytes()
    plan.close()


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["float", "double"])
@pytest.mark.parametrize("path", golden_params())
def test_values_diff_is_weight_diff_gathered_goldens(pkg, path, dt, relu):
    gd = Golden(path)
    _both(pkg, gd.desc(pkg, fuse_relu=relu), gd.w, gd.x, gd.bias, relu, dt)


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["float", "double"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_values_diff_is_weight_diff_gathered_shapes(pkg, synth, name, dt, relu):
    s = make_shape(synth, name)
    _both(pkg, pkg.ConvDesc.from_shape(s, fuse_relu=relu), synth.pruned_weights(s, 11), synth.activations(s, 12),
          synth.bias_vector(s, 13), relu, dt)


def test_both_layouts_together_are_refused(pkg, synth):
    s = make_shape(synth, "pointwise")
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
    plan.weight_align_cpu(synth.pruned_weights(s, 11))
    td = seeded((s.N, s.M) + tuple(plan.out_hw), 7)
    with pytest.raises(pkg.EscoinError):
        plan.backward_cpu(td, bottom=synth.activations(s, 12), weight_diff=True, values_diff=True)
    plan.close()


def test_argument_and_state_errors(pkg):
    import ctypes as C
    L = pkg.lib()
    d = pkg.ConvDesc(2, 4, 7, 7, 6, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1)
    plan = pkg.Plan(d)
    buf = np.zeros(4096, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.escoin_backward_values_cpu(plan._h, p, p, p, p, None, None, 1, 1) == -4      # before align
    w = seeded((6, 4, 3, 3), 4)
    w[seeded((6, 4, 3, 3), 5) > -0.2] = 0
    plan.weight_align_cpu(w)
    assert L.escoin_backward_values_cpu_f64(plan._h, p, p, p, p, None, None, 1, 1) == -4  # wrong Dtype
    assert L.escoin_backward_values_cpu(plan._h, None, p, p, None, p, None, 1, 1) == -1   # values_diff without bottom
    assert L.escoin_backward_values_cpu(plan._h, p, p, None, p, None, None, 1, 1) == -1   # no top_diff
    assert L.escoin_backward_values_cpu(plan._h, p, None, p, p, None, None, 1, 1) == -1   # fuse_relu without top
    assert L.escoin_backward_values_cpu(plan._h, p, p, p, p, None, None, -1, 1) == -1     # n_images < 0
    assert L.escoin_backward_values_cpu(plan._h, p, p, p, p, p, p, 0, 1) == 0             # nothing to do
    plan.close()


def test_explicit_zeros_left_by_a_host_update_receive_a_gradient(pkg, synth):
    """update_values_cpu keeps the pattern, so a weight that became 0 stays an entry (the host-only way to an explicit
    zero): the compact gradient still has nnz elements, and the entries whose weight is 0 get the gradient torch gives."""
    s = make_shape(synth, "straddle3x3")
    w = synth.pruned_weights(s, 11)
    x = synth.activations(s, 12)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
    plan.weight_align_cpu(w)
    nnz = plan.nnz()
    pos = csr_positions(plan)
    w2 = w.copy()
    w2.reshape(-1)[pos[::3]] = 0                       # every third entry becomes an explicit zero
    plan.update_values_cpu(w2)
    assert plan.nnz() == nnz and np.count_nonzero(plan.get_csr()[2] == 0) == len(pos[::3])
    td = seeded((s.N, s.M) + tuple(plan.out_hw), 7)
    _, vd, _ = plan.backward_cpu(td, bottom=x, bottom_diff=None, values_diff=True)
    _, wd, _ = plan.backward_cpu(td, bottom=x, bottom_diff=None, weight_diff=True)
    assert vd.shape == (nnz,) and vd.tobytes() == wd.reshape(-1)[pos].tobytes()
    want = torch_backward(x, w, None, s, td)[1].reshape(-1)[pos]      # (masked by the pattern: w, not w2)
    assert np.all(vd[::3] != 0)
    assert rel_err(vd, want) <= 1e-4
    plan.close()


@pytest.mark.gpu
def test_explicit_zeros_handed_to_set_csr_receive_a_gradient(pkg):
    """set_csr keeps explicit zeros: they are entries of the compact gradient.  (set_csr aligns on the device, hence the
    mark; the backward under test is the host one.)"""
    F = torch.nn.functional
    d = pkg.ConvDesc(1, 2, 5, 5, 2, 3, 3, 1, 1, 1, 1, 1, 1, 1, 0, 0)
    plan = pkg.Plan(d)
    plan.set_csr(np.array([0, 2, 3], np.int32), np.array([0, 4, 13], np.int32), np.array([0.0, 1.5, 0.0], np.float32), [3])
    x = seeded((1, 2, 5, 5), 12)
    td = seeded((1, 2, 5, 5), 13)
    _, vd, _ = plan.backward_cpu(td, bottom=x, bottom_diff=None, values_diff=True)
    Wt = torch.zeros((2, 2, 3, 3), dtype=torch.float64, requires_grad=True)
    F.conv2d(torch.tensor(x.astype(np.float64)), Wt, None, padding=1).backward(torch.tensor(td.astype(np.float64)))
    full = Wt.grad.numpy().reshape(2, -1)
    want = np.array([full[0, 0], full[0, 4], full[1, 13]])
    assert vd.shape == (3,) and np.all(vd != 0)
    assert rel_err(vd, want) <= 1e-4
    plan.close()
