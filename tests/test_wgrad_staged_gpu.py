"""The weight gradient on the MI355X under option "wgrad_kernel" (AUTO / ENTRY / STAGED) and in compact form
(escoin_backward_values): small shapes that cross every boundary of the chunked reduction against torch float64 autograd,
compact == dense gathered bit for bit, channel blocking, partial batches, empty rows, determinism, non-finite input,
bias-only calls and a captured training loop on compact tensors."""
import numpy as np
import pytest

from conftest import rel_err

torch = pytest.importorskip("torch")

from wgrad_common import SHAPES, csr_positions, make_shape, seeded, torch_backward  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module")
def dev(pkg):
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        pytest.fail("no HIP device visible (these tests run on the MI355X)")
    return torch.device("cuda:0")


_INPUTS = {}


def _inputs(synth, name):
    """(shape, weights, activations, bias, top_diff) of a named shape: made once, never written."""
    if name not in _INPUTS:
        s = make_shape(synth, name)
        oh, ow = synth.out_hw(s)
        _INPUTS[name] = (s, synth.pruned_weights(s, 11), synth.activations(s, 12), synth.bias_vector(s, 13),
                         seeded((s.N, s.M, oh, ow), 21))
    return _INPUTS[name]


def _plan(pkg, s, w, kernel, relu=False, **opts):
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu), wgrad_kernel=kernel, **opts)
    plan.weight_align(w)
    return plan


def _chunks(s, synth, n=None):
    oh, ow = synth.out_hw(s)
    return ((s.N if n is None else n) * oh * ow + 1023) // 1024


def _bytes(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_wgrad_kernel_matches_torch_and_compact_equals_dense(pkg, dev, synth, name, relu):
    s, w, x, b, td = _inputs(synth, name)
    staged_serves = s.stride_h == 1 and s.stride_w == 1
    xt, tdt = torch.from_numpy(x).to(dev), torch.from_numpy(td).to(dev)
    bt = torch.from_numpy(b).to(dev) if b is not None else None
    want = None
    for kernel in (pkg.WGRAD_AUTO, pkg.WGRAD_ENTRY, pkg.WGRAD_STAGED):
        plan = _plan(pkg, s, w, kernel, relu)
        with pytest.raises(pkg.EscoinError):
            plan.stat("wgrad_kernel")               # nothing has run yet
        top = plan.forward(xt, bt) if relu else None
        if kernel == pkg.WGRAD_STAGED and not staged_serves:
            with pytest.raises(pkg.EscoinError):
                plan.backward(tdt, bottom=xt, top=top, weight_diff=True)
            plan.close()
            continue
        _, wd, bsd = plan.backward(tdt, bottom=xt, top=top, bottom_diff=None, weight_diff=True,
                                   bias_diff=True if b is not None else None)
        _, vd, bsd2 = plan.backward(tdt, bottom=xt, top=top, bottom_diff=None, values_diff=True,
                                    bias_diff=True if b is not None else None)
        torch.cuda.synchronize()
        if want is None:
            want = torch_backward(x, w, b, s, td, None if top is None else top.cpu().numpy())
        wd, vd = wd.cpu().numpy(), vd.cpu().numpy()
        ran = plan.stat("wgrad_kernel")
        what = (name, kernel, ran, relu)
        print(what, "weight_diff rel_err", rel_err(wd, want[1]),
              "bias_diff rel_err", None if b is None else rel_err(bsd.cpu().numpy(), want[2]))
        assert rel_err(wd, want[1]) <= TOL, what
        assert np.all(wd[w == 0] == 0), what
        if b is not None:
            assert rel_err(bsd.cpu().numpy(), want[2]) <= TOL, what
            assert _bytes(bsd) == _bytes(bsd2), what
        assert vd.shape == (plan.nnz(),)
        assert vd.tobytes() == wd.reshape(-1)[csr_positions(plan)].tobytes(), what
        if kernel != pkg.WGRAD_AUTO:
            assert ran == kernel, what
        else:
            # AUTO compares two modelled times (profiles/backward_mi355x.md).  Launches this small fill a fraction of one
            # round of workgroups on either kernel, where the model has the staged kernel ahead: 21.9 against 24.1 us
            # on pointwise, the closest of these shapes, 33 against 91 on dense_rows
            auto = pkg.WGRAD_STAGED if staged_serves else pkg.WGRAD_ENTRY
            assert ran == auto, what
        if not staged_serves:
            assert ran == pkg.WGRAD_ENTRY and plan.stat("wgrad_lds_bytes") == 0
        if ran == pkg.WGRAD_STAGED:
            assert 0 < plan.stat("wgrad_lds_bytes") <= 64 * 1024     # the kernel's budget: two workgroups per CU
        assert plan.stat("bwd_chunks") == _chunks(s, synth), what
        plan.close()


@pytest.mark.parametrize("name", ["straddle3x3", "dense_rows"])
def test_channel_block_does_not_change_the_bits(pkg, dev, synth, name):
    s, w, x, b, td = _inputs(synth, name)
    xt, tdt = torch.from_numpy(x).to(dev), torch.from_numpy(td).to(dev)
    got = []
    for cb in (1, 3, 0):
        plan = _plan(pkg, s, w, pkg.WGRAD_STAGED, wgrad_channel_block=cb)
        _, vd, bsd = plan.backward(tdt, bottom=xt, bottom_diff=None, values_diff=True, bias_diff=True)
        torch.cuda.synchronize()
        assert plan.stat("wgrad_kernel") == pkg.WGRAD_STAGED
        got.append((_bytes(vd), _bytes(bsd), plan.stat("wgrad_lds_bytes")))
        plan.close()
    assert got[0][:2] == got[1][:2] == got[2][:2]
    assert got[0][2] < got[1][2] <= got[2][2]           # the option did change the staging


def test_auto_keeps_the_entry_kernel_on_short_rows_over_many_blocks(pkg, dev, synth):
    """GoogLeNet's inception_4a/1x1_2 at batch 64: 16 output channels, 480 input channels in 32 staged blocks, 24 entries
    per row.  The staged kernel would stage 832 tiles (1.6 rounds of 512 resident workgroups) for 0.75 entries per
    (row, block): modelled 46.9 us against the entry kernel's 32.4, so AUTO keeps the entry kernel.  The staged kernel
    still serves the plan when asked, with the same gradient."""
    s = synth.shape("short_rows", 64, 480, 14, 14, 16, 1, sparsity=0.95)
    w, x = synth.pruned_weights(s, 11), synth.activations(s, 12)
    td = seeded((s.N, s.M, 14, 14), 21)
    xt, tdt = torch.from_numpy(x).to(dev), torch.from_numpy(td).to(dev)
    want = torch_backward(x, w, None, s, td)
    for kernel, runs in ((pkg.WGRAD_AUTO, pkg.WGRAD_ENTRY), (pkg.WGRAD_STAGED, pkg.WGRAD_STAGED)):
        plan = _plan(pkg, s, w, kernel)
        _, wd, _ = plan.backward(tdt, bottom=xt, bottom_diff=None, weight_diff=True)
        torch.cuda.synchronize()
        assert plan.stat("wgrad_kernel") == runs, kernel
        assert rel_err(wd.cpu().numpy(), want[1]) <= TOL, kernel
        plan.close()


def test_partial_batch_is_the_gradient_of_the_first_images(pkg, dev, synth):
    s, w, x, b, td = _inputs(synth, "small7x7g2")
    n = s.N - 1
    xt, tdt = torch.from_numpy(x).to(dev), torch.from_numpy(td).to(dev)
    want = torch_backward(x[:n], w, b, s, td[:n])
    compact = {}
    for kernel in (pkg.WGRAD_ENTRY, pkg.WGRAD_STAGED):
        plan = _plan(pkg, s, w, kernel)
        _, wd, bsd = plan.backward(tdt[:n], bottom=xt[:n], bottom_diff=None, weight_diff=True, bias_diff=True)
        _, vd, _ = plan.backward(tdt[:n], bottom=xt[:n], bottom_diff=None, values_diff=True)
        torch.cuda.synchronize()
        wd, vd = wd.cpu().numpy(), vd.cpu().numpy()
        assert rel_err(wd, want[1]) <= TOL and rel_err(bsd.cpu().numpy(), want[2]) <= TOL, kernel
        pos = csr_positions(plan)
        assert rel_err(vd, want[1].reshape(-1)[pos]) <= TOL, kernel
        assert vd.tobytes() == wd.reshape(-1)[pos].tobytes(), kernel
        assert plan.stat("wgrad_kernel") == kernel and plan.stat("bwd_chunks") == _chunks(s, synth, n)
        compact[kernel] = vd
        plan.close()
    # the two kernels sum 2058 products per entry in different orders: that all 144 fp32 results agree to the last bit
    # would mean the forced kernel did not run
    assert compact[pkg.WGRAD_ENTRY].tobytes() != compact[pkg.WGRAD_STAGED].tobytes()


def test_empty_rows_and_an_empty_input_channel(pkg, dev, synth):
    s, w, x, b, td = _inputs(synth, "straddle3x3")
    w = w.copy()
    w[0] = 0
    w[s.M - 1] = 0
    w[:, 5] = 0
    xt, tdt = torch.from_numpy(x).to(dev), torch.from_numpy(td).to(dev)
    want = torch_backward(x, w, b, s, td)
    for kernel in (pkg.WGRAD_ENTRY, pkg.WGRAD_STAGED):
        for cb in (0, 1):
            plan = _plan(pkg, s, w, kernel, wgrad_channel_block=cb)
            _, wd, bsd = plan.backward(tdt, bottom=xt, bottom_diff=None, weight_diff=True, bias_diff=True)
            _, vd, _ = plan.backward(tdt, bottom=xt, bottom_diff=None, values_diff=True)
            torch.cuda.synchronize()
            wd = wd.cpu().numpy()
            assert rel_err(wd, want[1]) <= TOL and rel_err(bsd.cpu().numpy(), want[2]) <= TOL, (kernel, cb)
            assert np.all(wd[w == 0] == 0)
            assert vd.cpu().numpy().tobytes() == wd.reshape(-1)[csr_positions(plan)].tobytes()
            plan.close()


@pytest.mark.parametrize("name", ["straddle3x3", "pointwise"])
def test_determinism_streams_and_memory(pkg, dev, synth, name):
    s, w, x, b, td = _inputs(synth, name)
    xt, tdt = torch.from_numpy(x).to(dev), torch.from_numpy(td).to(dev)
    plan = _plan(pkg, s, w, pkg.WGRAD_STAGED)
    ws0 = plan.workspace_bytes

    def call():
        return plan.backward(tdt, bottom=xt, bottom_diff=None, values_diff=True, bias_diff=True)
    r1 = call()
    ws1 = plan.workspace_bytes
    assert ws1 > ws0
    assert ws1 == plan.stat("device_bytes") + plan.stat("bwd_device_bytes") + plan.stat("upd_device_bytes")
    r2 = call()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        r3 = call()
    torch.cuda.synchronize()
    assert plan.workspace_bytes == ws1
    for a, c, e in zip(r1[1:], r2[1:], r3[1:]):
        assert _bytes(a) == _bytes(c) == _bytes(e)
    plan.close()


def test_non_finite_bottom_reaches_only_the_entries_whose_tap_reads_it(pkg, dev, synth):
    s, w, x, b, td = _inputs(synth, "straddle3x3")
    c = 7
    x_inf = x.copy()
    x_inf[1, c, 0, 0] = np.inf
    tdt = torch.from_numpy(td).to(dev)
    for kernel in (pkg.WGRAD_ENTRY, pkg.WGRAD_STAGED):
        plan = _plan(pkg, s, w, kernel)
        _, clean, _ = plan.backward(tdt, bottom=torch.from_numpy(x).to(dev), bottom_diff=None, values_diff=True)
        _, dirty, _ = plan.backward(tdt, bottom=torch.from_numpy(x_inf).to(dev), bottom_diff=None, values_diff=True)
        torch.cuda.synchronize()
        clean, dirty = clean.cpu().numpy(), dirty.cpu().numpy()
        # pixel (0, 0) is read by output pixel (pad - kr, pad - kc): inside the image for kr, kc <= pad = 1
        col = plan.get_csr()[1]
        ic, kr, kc = col // 9, (col // 3) % 3, col % 3
        hit = (ic == c) & (kr <= 1) & (kc <= 1)
        assert hit.sum() > 0 and (~hit).sum() > 0
        assert not np.any(np.isfinite(dirty[hit])), kernel
        assert dirty[~hit].tobytes() == clean[~hit].tobytes(), kernel
        plan.close()


@pytest.mark.parametrize("name", ["straddle3x3", "small7x7g2"])
def test_bias_only_call_gives_the_fused_call_s_bits(pkg, dev, synth, name):
    s, w, x, b, td = _inputs(synth, name)
    xt, tdt = torch.from_numpy(x).to(dev), torch.from_numpy(td).to(dev)
    for kernel in (pkg.WGRAD_ENTRY, pkg.WGRAD_STAGED):
        plan = _plan(pkg, s, w, kernel)
        _, _, alone = plan.backward(tdt, bottom_diff=None, bias_diff=True)
        _, _, fused = plan.backward(tdt, bottom=xt, bottom_diff=None, values_diff=True, bias_diff=True)
        torch.cuda.synchronize()
        assert _bytes(alone) == _bytes(fused), kernel
        assert rel_err(alone.cpu().numpy(), td.astype(np.float64).sum(axis=(0, 2, 3))) <= TOL
        plan.close()


@pytest.mark.parametrize("kernel", [1, 2], ids=["entry", "staged"])
def test_captured_training_steps_on_compact_tensors(pkg, dev, synth, kernel):
    """Three steps of forward, backward(values_diff), v -= lr * vd, set_values(v) in one graph, next to a dense-layout
    twin (weight_diff, dense SGD, update_values): after the replays both plans hold the same values, bit for bit."""
    lr = 1e-3
    F = torch.nn.functional
    specs = [(synth.resnet50_3x3(N=2)[3], dict(tiling_batch=256)), (_inputs(synth, "pointwise")[0], {})]
    layers = []
    for i, (s, opts) in enumerate(specs):
        w0 = synth.pruned_weights(s, 70 + i)
        b0 = synth.bias_vector(s, 75 + i)
        pair = []
        for compact in (True, False):
            plan = _plan(pkg, s, w0, kernel, **opts)
            oh, ow = plan.out_hw
            u = dict(x=torch.from_numpy(synth.activations(s, 80 + i)).to(dev),
                     td=torch.from_numpy(seeded((s.N, s.M, oh, ow), 90 + i)).to(dev),
                     y=torch.zeros((s.N, s.M, oh, ow), device=dev),
                     b=torch.from_numpy(b0).to(dev) if b0 is not None else None)
            if compact:
                u["v"] = torch.from_numpy(plan.get_csr()[2].copy()).to(dev)
                u["vd"] = torch.zeros_like(u["v"])
            else:
                u["W"] = torch.from_numpy(w0).to(dev)
                u["wd"] = torch.zeros_like(u["W"])
            pair.append((plan, u))
        layers.append((s, w0, b0, pair))

    def step():
        for s, w0, b0, pair in layers:
            for plan, u in pair:
                plan.forward(u["x"], u["b"], u["y"])
                if "v" in u:
                    u["vd"].zero_()
                    plan.backward(u["td"], bottom=u["x"], bottom_diff=None, values_diff=u["vd"])
                    u["v"].add_(u["vd"], alpha=-lr)
                    plan.set_values(u["v"])
                else:
                    u["wd"].zero_()
                    plan.backward(u["td"], bottom=u["x"], bottom_diff=None, weight_diff=u["wd"])
                    u["W"].add_(u["wd"], alpha=-lr)
                    plan.update_values(u["W"])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                      # warm-up: builds the backward and update states outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for s, w0, b0, pair in layers:
        for plan, u in pair:
            assert plan.stat("wgrad_kernel") == kernel and plan.stat("update_fast") == 1
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(3):
            step()
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    for s, w0, b0, pair in layers:
        (pc, uc), (pd, ud) = pair
        vc, vdn = pc.get_csr()[2], pd.get_csr()[2]
        assert vc.tobytes() == vdn.tobytes(), s.name
        assert vc.tobytes() == uc["v"].cpu().numpy().tobytes()
        W = ud["W"].cpu().numpy()
        assert np.all(W[w0 == 0] == 0) and not np.array_equal(W, w0)
        want = F.conv2d(uc["x"].double().cpu(), torch.from_numpy(W.astype(np.float64)),
                        None if b0 is None else torch.from_numpy(b0.astype(np.float64)), padding=(s.pad_h, s.pad_w)).numpy()
        for plan, u in pair:
            y = plan.forward(u["x"], u["b"]).cpu().numpy()
            assert rel_err(y, want) <= TOL, s.name
            plan.close()
