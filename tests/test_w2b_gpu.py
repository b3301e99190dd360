"""Plan option "w2b" on the MI355X.  The three kernels alone against the numpy rule of w2b_common.py, exactly; forward,
escoin_backward and escoin_backward_values of every shape against torch float64 and the per-element bound of errbound.py, the
inner kernel automatic and forced; a 300-wide layer, which the tiled kernels refuse without the option; and one sequence of
align, forward, backward, solver step, captured forward and prune."""
import numpy as np
import pytest

import errbound as eb
from prune_common import masked_dense
from upd_common import values_at
from w2b_common import SHAPES, make, pack, plan_row, unpack, unpack_sum
from wgrad_common import seeded

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
# (bias, relu) a forced inner kernel runs with; AUTO runs all four
COMBOS = {"GENERIC": [(0, 1)], "DENSE": [(1, 0)], "JIT": [(1, 1)], "TILED": [(0, 0)], "AUTO": [(1, 0), (1, 1), (0, 0), (0, 1)]}
_CASES = {}


@pytest.fixture(scope="module")
def dev(pkg):
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        pytest.fail("no HIP device visible (these tests run on the MI355X)")
    return torch.device("cuda:0")


def _case(synth, name, bias=True):
    """(shape, skewed inputs) of a shape: made once, never written."""
    if (name, bias) not in _CASES:
        s = make(synth, name, bias=bool(bias))
        td = seeded((s.N, s.M) + synth.out_hw(s), 21)
        _CASES[(name, bias)] = (s, eb.skew(s, synth.pruned_weights(s, 11), synth.activations(s, 12), synth.bias_vector(s, 13), 95, top_diff=td))
    return _CASES[(name, bias)]


def _up(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def _nan(shape, dev):
    return torch.full(tuple(shape), float("nan"), device=dev)


def _plan(pkg, name, s, w, relu=False, **opts):
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=bool(relu)), w2b=1, w2b_strip=SHAPES[name][10], **opts)
    plan.weight_align(w)
    return plan


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_three_kernels_alone_equal_the_numpy_rule(pkg, synth, dev, name):
    """A copy is exact and a sum of two floats does not depend on the order: array_equal.  With n_images = N - 1 the last
    image's destination keeps its NaN."""
    s, sk = _case(synth, name)
    S, SW, Wi = plan_row(synth, s, SHAPES[name][10])[1:4]
    oh, ow = synth.out_hw(s)
    plan = _plan(pkg, name, s, sk.w)
    assert (plan.stat("w2b"), plan.stat("w2b_strips"), plan.stat("w2b_strip")) == (1, S, SW)
    assert plan.stat("w2b_scratch_bytes") == 4 * (2 * s.N * S * s.C * s.H * Wi + s.N * S * s.M * oh * SW)
    x, td, mask = sk.x, sk.top_diff, seeded(sk.top_diff.shape, 22)
    dx, t = seeded((s.N * S, s.C, s.H, Wi), 23), seeded((s.N * S, s.M, oh, SW), 24)
    for n in (s.N, s.N - 1):
        runs = [  # (the call, its destination, what the first n images' part of it must hold)
            (lambda d: plan.w2b_pack(_up(x, dev), d, n_images=n), dx.shape, pack(x[:n], S, SW, Wi, s.pad_w)),
            (lambda d: plan.w2b_pack(_up(td, dev), d, mask=_up(mask, dev), top_side=True, n_images=n), t.shape, pack(td[:n], S, SW, SW, 0, mask[:n])),
            (lambda d: plan.w2b_pack(_up(td, dev), d, top_side=True, n_images=n), t.shape, pack(td[:n], S, SW, SW, 0)),
            (lambda d: plan.w2b_unpack(_up(t, dev), d, n_images=n), td.shape, unpack(t[:n * S], S, SW, ow)),
            (lambda d: plan.w2b_unpack(_up(t, dev), d, relu=True, n_images=n), td.shape, unpack(t[:n * S], S, SW, ow, relu=True)),
            (lambda d: plan.w2b_unpack_sum(_up(dx, dev), d, n_images=n), x.shape, unpack_sum(dx[:n * S], S, SW, s.W, s.pad_w))]
        for i, (call, shape, want) in enumerate(runs):
            dst = _nan(shape, dev)
            call(dst)
            got = dst.cpu().numpy()
            assert np.array_equal(got[:len(want)], want) and np.all(np.isnan(got[len(want):])), (name, n, i)
            assert len(got) - len(want) == (s.N - n) * shape[0] // s.N
    plan.close()


@pytest.mark.parametrize("kernel", list(COMBOS))
@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_and_backward_within_the_float64_error_bound(pkg, synth, dev, name, kernel):
    for bias, relu in COMBOS[kernel]:
        s, sk = _case(synth, name, bias)
        plan = _plan(pkg, name, s, sk.w, relu, kernel=getattr(pkg, "KERNEL_" + kernel))
        assert plan.stat("w2b") == 1 and plan.kernel_name.startswith("escoin_w2b_pack_kernel + ") and plan.kernel_name.endswith(" + escoin_w2b_unpack_kernel")
        assert kernel == "AUTO" or plan.stat("kernel_choice") == getattr(pkg, "KERNEL_" + kernel), plan.kernel_name     # the inner plan's
        what = (name, kernel, "bias", bias, "relu", relu)
        xd, tdd = _up(sk.x, dev), _up(sk.top_diff, dev)
        want, B = eb.forward_bound(s, sk.w, sk.x, sk.b, relu=bool(relu))
        top = plan.forward(xd, _up(sk.b, dev), _nan(want.shape, dev))
        rf = eb.within(top.cpu().numpy(), want, B, plan.kernel_name, sk.row_exp, what=what)
        wantb, Bs = eb.backward_bound(s, sk.w, sk.x, sk.b, sk.top_diff, top.cpu().numpy() if relu else None)
        t = top if relu else None
        bd, wd, bsd = plan.backward(tdd, bottom=xd, top=t, bottom_diff=_nan(sk.x.shape, dev), weight_diff=True, bias_diff=True if bias else None)
        _, vd, _ = plan.backward(tdd, bottom=xd, top=t, bottom_diff=None, values_diff=True)
        rb = eb.within(bd.cpu().numpy(), wantb[0], Bs[0], "data gradient", sk.chan_exp, what=what)
        rw = eb.within(wd.cpu().numpy(), wantb[1], Bs[1], "weight gradient", what=what)
        assert not bias or eb.within(bsd.cpu().numpy(), wantb[2], Bs[2], "bias gradient", what=what) <= 1
        rv = eb.within(vd.cpu().numpy(), values_at(plan, wantb[1])[2], values_at(plan, Bs[1])[2], "compact gradient", axis=0, what=what)
        print("errbound w2b %-8s %-8s bias=%d relu=%d forward %.3g, data %.3g, weight %.3g, compact %.3g  %s" % (what[:2] + (bias, relu, rf, rb, rw, rv, plan.kernel_name)))
        plan.close()


@pytest.mark.parametrize("kernel", ["JIT", "TILED"])
def test_without_the_option_a_300_wide_layer_refuses_the_tiled_kernels(pkg, synth, dev, kernel):
    """The gap itself; with the option the same forced kernels run it as 2 strips of 152 (the tests above)."""
    s, sk = _case(synth, "real")
    plain = pkg.Plan(pkg.ConvDesc.from_shape(s), kernel=getattr(pkg, "KERNEL_" + kernel))
    with pytest.raises(pkg.EscoinError) as e:
        plain.weight_align(sk.w)
    assert "failed (-1)" in str(e.value)                                    # ESCOIN_EINVAL
    plain.close()
    plan = _plan(pkg, "real", s, sk.w, kernel=getattr(pkg, "KERNEL_" + kernel))
    assert (plan.stat("w2b"), plan.stat("w2b_strips"), plan.stat("w2b_strip")) == (1, 2, 152)
    plan.close()


def test_align_forward_backward_solver_step_captured_forward_prune_forward(pkg, synth, dev):
    s, sk = _case(synth, "k3p1")
    plan = _plan(pkg, "k3p1", s, sk.w)
    xd, bd_, tdd = _up(sk.x, dev), _up(sk.b, dev), _up(sk.top_diff, dev)

    def forward_within(step):
        want, B = eb.forward_bound(s, masked_dense(plan.desc, *plan.get_csr()), sk.x, sk.b)
        y = plan.forward(xd, bd_, _nan(want.shape, dev))
        eb.within(y.cpu().numpy(), want, B, plan.kernel_name, what=("k3p1", step))
        return y

    forward_within("align")
    nnz = plan.nnz()
    _, vd, _ = plan.backward(tdd, bottom=xd, bottom_diff=_nan(sk.x.shape, dev), values_diff=True)
    plan.solver_step(vd, torch.zeros(nnz, device=dev), type="sgd", rate=0.05, momentum=0.9)
    assert plan.stat("update_fast") == 1 and plan.stat("w2b") == 1
    eager = forward_within("solver_step")
    ws, out, g = plan.workspace_bytes, _nan(eager.shape, dev), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.forward(xd, bd_, out)
    for _ in range(2):
        out.fill_(float("nan"))
        g.replay()
        assert out.cpu().numpy().tobytes() == eager.cpu().numpy().tobytes()
    assert plan.workspace_bytes == ws                                       # the forward allocates nothing
    plan.prune(keep=nnz // 2)
    assert plan.nnz() == nnz // 2 and plan.stat("w2b") == 1
    forward_within("prune")
    plan.close()
