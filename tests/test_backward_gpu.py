"""Pattern-preserving Backward on the MI355X (escoin_backward[_f64]): goldens and odd geometries through every
backward_kernel against torch float64 autograd, the gather kernel bit for bit against the CPU mode, the BASELINE shapes,
one full-size res2 layer on sampled entries, determinism, memory, re-align and graph capture."""
import numpy as np
import pytest

from conftest import Golden, golden_params, rel_err

torch = pytest.importorskip("torch")
F = torch.nn.functional

from wgrad_common import EDGES, csr_positions, edge_inputs, torch_backward  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module")
def dev(pkg):
    if not torch.cuda.is_available() or pkg.device_count() < 1:
        pytest.fail("no HIP device visible (these tests run on the MI355X)")
    return torch.device("cuda:0")


def _seeded(shape, seed, dt=np.float32):
    return np.random.RandomState(seed).uniform(-1, 1, shape).astype(dt)


def _transposable(s):
    return (s.stride_h == 1 and s.stride_w == 1 and s.pad_h <= s.dil_h * (s.KH - 1) and
            s.pad_w <= s.dil_w * (s.KW - 1))


def _run(pkg, dev, s, desc, w, x, b, kernel=None, dt=np.float32, relu=False, **opts):
    """One GPU backward (all three gradients) + the forward top it needs; returns numpy results and the plan."""
    if kernel is not None:
        opts["backward_kernel"] = kernel
    plan = pkg.Plan(desc, **opts)
    plan.weight_align(w.astype(dt))
    xt = torch.from_numpy(x.astype(dt)).to(dev)
    bt = torch.from_numpy(b.astype(dt)).to(dev) if b is not None else None
    top = plan.forward(xt, bt) if relu else None
    td = _seeded((x.shape[0], desc.M) + tuple(plan.out_hw), 21, dt)
    bd, wd, bsd = plan.backward(torch.from_numpy(td).to(dev), bottom=xt, top=top, weight_diff=True,
                                bias_diff=True if b is not None else None)
    torch.cuda.synchronize()
    return (plan, td, None if top is None else top.cpu().numpy(), bd.cpu().numpy(), wd.cpu().numpy(),
            None if bsd is None else bsd.cpu().numpy())


def _check_against_torch(s, w, x, b, td, top, bd, wd, bsd, tol=TOL, what=""):
    want_bd, want_wd, want_bsd = torch_backward(x, w, b, s, td, top)
    assert rel_err(bd, want_bd) <= tol, (what, "bottom_diff", rel_err(bd, want_bd))
    assert rel_err(wd, want_wd) <= tol, (what, "weight_diff", rel_err(wd, want_wd))
    assert np.all(wd[np.asarray(w) == 0] == 0), what
    if b is not None:
        assert rel_err(bsd, want_bsd) <= tol, (what, "bias_diff")


ODD = [
    # N, C, H, W, M, KH, KW, pad_h, pad_w, stride_h, stride_w, dil_h, dil_w, group
    (2, 6, 11, 9, 8, 3, 3, 2, 2, 1, 1, 2, 2, 2),      # dilation 2, groups (transposed plan: generic kernel)
    (2, 8, 10, 12, 6, 3, 5, 0, 1, 1, 1, 1, 1, 1),     # KH != KW, asymmetric pads
    (3, 16, 14, 14, 24, 1, 1, 0, 0, 2, 2, 1, 1, 1),   # 1x1 stride 2: gather kernel
    (2, 8, 9, 9, 8, 3, 3, 3, 3, 1, 1, 1, 1, 1),       # pad > dil * (K - 1): gather kernel
    (1, 12, 17, 13, 12, 5, 5, 2, 2, 2, 1, 1, 1, 3),   # stride 2 x 1, groups 3
]


def _odd_shape(synth, t, i):
    N, C, H, W, M, KH, KW, ph, pw, sh, sw, dh, dw, g = t
    return synth.shape("odd%d" % i, N, C, H, W, M, KH, pad=ph, stride=sh, dil=dh, group=g, KW=KW, pad_w=pw,
                       stride_w=sw, dil_w=dw, sparsity=0.6)


@pytest.mark.parametrize("path", golden_params())
def test_goldens_match_torch_for_every_backward_kernel(pkg, dev, path):
    gd = Golden(path)
    kernels = [pkg.KERNEL_AUTO, pkg.KERNEL_GENERIC]
    if _transposable(gd):
        kernels += [pkg.KERNEL_TILED, pkg.KERNEL_JIT, pkg.KERNEL_DENSE]
    for relu in (False, True):
        for k in kernels:
            try:
                plan, td, top, bd, wd, bsd = _run(pkg, dev, gd, gd.desc(pkg, fuse_relu=relu), gd.w, gd.x, gd.bias,
                                                  kernel=k, relu=relu)
            except pkg.EscoinError:
                # a forced kernel the transposed geometry does not fit: the forward refuses it the same way
                assert k in (pkg.KERNEL_TILED, pkg.KERNEL_JIT)
                continue
            got_k = plan.stat("bwd_data_kernel")
            if k == pkg.KERNEL_GENERIC or not _transposable(gd):
                assert got_k == pkg.KERNEL_GENERIC
            elif k != pkg.KERNEL_AUTO:
                assert got_k == k, (k, got_k)
            _check_against_torch(gd, gd.w, gd.x, gd.bias, td, top, bd, wd, bsd, what=(gd.name, k, relu))
            plan.close()


@pytest.mark.parametrize("i", range(len(ODD)))
def test_odd_geometries_match_torch(pkg, dev, synth, i):
    s = _odd_shape(synth, ODD[i], i)
    w = synth.pruned_weights(s, 100 + i)
    x = synth.activations(s, 200 + i)
    b = synth.bias_vector(s, 300 + i)
    for k in (pkg.KERNEL_AUTO, pkg.KERNEL_GENERIC):
        for relu in (False, True):
            plan, td, top, bd, wd, bsd = _run(pkg, dev, s, pkg.ConvDesc.from_shape(s, fuse_relu=relu), w, x, b,
                                              kernel=k, relu=relu)
            _check_against_torch(s, w, x, b, td, top, bd, wd, bsd, what=(s.name, k, relu))
            plan.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["float", "double"])
@pytest.mark.parametrize("path", golden_params())
def test_gather_kernel_is_bit_equal_to_the_cpu_mode(pkg, dev, path, dt):
    gd = Golden(path)
    for relu in (False, True):
        desc = gd.desc(pkg, fuse_relu=relu)
        plan, td, top, bd, wd, bsd = _run(pkg, dev, gd, desc, gd.w, gd.x, gd.bias, kernel=pkg.KERNEL_GENERIC, dt=dt,
                                          relu=relu)
        assert plan.stat("bwd_data_kernel") == pkg.KERNEL_GENERIC
        cbd, cwd, cbsd = plan.backward_cpu(td, bottom=gd.x.astype(dt), top=top, weight_diff=True)
        assert bd.tobytes() == cbd.tobytes(), (gd.name, relu)
        tol = 1e-12 if dt == np.float64 else TOL
        assert rel_err(wd, cwd) <= tol
        if dt == np.float64:
            _check_against_torch(gd, gd.w, gd.x, gd.bias, td, top, bd, wd, bsd, tol=1e-12, what=gd.name)
        plan.close()


def _baseline_shapes(synth):
    out = [s for s in synth.resnet50_3x3(N=2)] + synth.alexnet(N=2) + synth.lenet_conv2(N=2)
    g = synth.googlenet_1x1(N=2)
    out += [g[1], g[8], g[-1]]
    return out


_CONFIG_BATCH = {"res": 256, "alex": 128, "lenet": 64}


def test_baseline_shapes_match_torch(pkg, dev, synth):
    for s in _baseline_shapes(synth):
        tb = next((v for k, v in _CONFIG_BATCH.items() if s.name.startswith(k)), 256)
        w = synth.pruned_weights(s, 41)
        x = synth.activations(s, 42)
        b = synth.bias_vector(s, 43)
        plan, td, top, bd, wd, bsd = _run(pkg, dev, s, pkg.ConvDesc.from_shape(s), w, x, b, tiling_batch=tb)
        _check_against_torch(s, w, x, b, td, top, bd, wd, bsd, what=(s.name, plan.stat("bwd_data_kernel")))
        plan.close()


def test_full_size_res2_on_sampled_entries_and_pixels(pkg, dev, synth):
    s = synth.resnet50_3x3(N=256)[0]
    w = synth.pruned_weights(s, 51)
    x = synth.activations(s, 52)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
    plan.weight_align(w)
    xt = torch.from_numpy(x).to(dev)
    td = torch.empty((s.N, s.M, 56, 56), device=dev).uniform_(-1, 1, generator=torch.Generator(dev).manual_seed(5))
    bd, wd, _ = plan.backward(td, bottom=xt, weight_diff=True)
    torch.cuda.synchronize()
    g = td.cpu().numpy().astype(np.float64)
    xd = np.pad(x.astype(np.float64), ((0, 0), (0, 0), (1, 1), (1, 1)))
    wd = wd.cpu().numpy()
    nz = np.argwhere(w != 0)
    rs = np.random.RandomState(3)
    for oc, ic, kr, kc in nz[rs.choice(len(nz), 32, replace=False)]:
        want = float(np.sum(g[:, oc] * xd[:, ic, kr:kr + 56, kc:kc + 56]))
        assert abs(wd[oc, ic, kr, kc] - want) <= 1e-4 * max(1.0, abs(want)) + 1e-5 * np.sqrt(s.N * 56 * 56), (oc, ic, kr, kc)
    gp = np.pad(g, ((0, 0), (0, 0), (1, 1), (1, 1)))
    bdn = bd.cpu().numpy()
    for _ in range(32):
        n, c, h, ww = rs.randint(s.N), rs.randint(s.C), rs.randint(56), rs.randint(56)
        # bottom_diff[n, c, h, w] = sum_oc,kr,kc w[oc, c, kr, kc] * G[n, oc, h + 1 - kr, w + 1 - kc]
        win = gp[n, :, h:h + 3, ww:ww + 3][:, ::-1, ::-1]
        want = float(np.sum(w[:, c].astype(np.float64) * win))
        assert abs(bdn[n, c, h, ww] - want) <= 1e-4 * max(1.0, abs(want)), (n, c, h, ww)
    assert plan.stat("bwd_chunks") == (s.N * 56 * 56 + 1023) // 1024
    plan.close()


def test_determinism_memory_and_realign(pkg, dev, synth):
    for s in (synth.resnet50_3x3(N=4)[2], _odd_shape(synth, ODD[2], 2)):
        w = synth.pruned_weights(s, 61)
        x = synth.activations(s, 62)
        b = synth.bias_vector(s, 63)
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
        plan.weight_align(w)
        ws0 = plan.workspace_bytes
        xt = torch.from_numpy(x).to(dev)
        td = torch.from_numpy(_seeded((s.N, s.M) + tuple(plan.out_hw), 64)).to(dev)
        r1 = plan.backward(td, bottom=xt, weight_diff=True, bias_diff=True if b is not None else None)
        ws1 = plan.workspace_bytes
        assert ws1 > ws0 and plan.stat("bwd_device_bytes") == ws1 - ws0
        r2 = plan.backward(td, bottom=xt, weight_diff=True, bias_diff=True if b is not None else None)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            r3 = plan.backward(td, bottom=xt, weight_diff=True, bias_diff=True if b is not None else None)
        torch.cuda.synchronize()
        assert plan.workspace_bytes == ws1
        for a, c, e in zip(r1, r2, r3):
            if a is not None:
                assert a.cpu().numpy().tobytes() == c.cpu().numpy().tobytes() == e.cpu().numpy().tobytes()
        # re-align with new weights: the state is rebuilt and the gradients are the new weights'
        w2 = synth.pruned_weights(s, 65)
        plan.weight_align(w2)
        assert plan.stat("bwd_device_bytes") == 0 and plan.workspace_bytes == plan.stat("device_bytes")
        bd, wd, _ = plan.backward(td, bottom=xt, weight_diff=True)
        torch.cuda.synchronize()
        want_bd, want_wd, _ = torch_backward(x, w2, None, s, td.cpu().numpy())
        assert rel_err(bd.cpu().numpy(), want_bd) <= TOL and rel_err(wd.cpu().numpy(), want_wd) <= TOL
        plan.close()


def test_argument_and_state_errors_on_the_device(pkg, dev, synth):
    import ctypes as C
    L = pkg.lib()
    s = synth.shape("e", 2, 4, 7, 7, 6, 3, pad=1, sparsity=0.5)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=True))
    buf = torch.zeros(4096, device=dev)
    p = C.c_void_p(buf.data_ptr())
    assert L.escoin_backward(plan._h, p, p, p, p, None, None, 1, None) == -4          # before align
    plan.weight_align(synth.pruned_weights(s, 1))
    assert L.escoin_backward_f64(plan._h, p, p, p, p, None, None, 1, None) == -4      # wrong dtype
    assert L.escoin_backward(plan._h, p, p, None, p, None, None, 1, None) == -1       # no top_diff
    assert L.escoin_backward(plan._h, p, None, p, p, None, None, 1, None) == -1       # fuse_relu without top
    assert L.escoin_backward(plan._h, None, p, p, None, p, None, 1, None) == -1       # weight_diff without bottom
    assert L.escoin_backward(plan._h, p, p, p, p, None, None, 3, None) == -1          # n_images > desc.N
    assert L.escoin_backward(plan._h, p, p, p, p, None, None, -1, None) == -1
    plan.close()
    # a forced transposed-plan kernel on a geometry without a transposed plan
    s2 = synth.shape("e2", 2, 4, 8, 8, 6, 3, pad=1, stride=2, sparsity=0.5)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s2), backward_kernel=pkg.KERNEL_JIT)
    plan.weight_align(synth.pruned_weights(s2, 1))
    with pytest.raises(pkg.EscoinError):
        plan.backward(torch.zeros((2, 6, 4, 4), device=dev))
    plan.close()


def test_explicit_zeros_handed_to_set_csr_receive_a_gradient_on_the_device(pkg, dev):
    d = pkg.ConvDesc(1, 2, 5, 5, 2, 3, 3, 1, 1, 1, 1, 1, 1, 1, 0, 0)
    x = _seeded((1, 2, 5, 5), 12)
    td = _seeded((1, 2, 5, 5), 13)
    Wt = torch.zeros((2, 2, 3, 3), dtype=torch.float64, requires_grad=True)
    F.conv2d(torch.tensor(x.astype(np.float64)), Wt, None, padding=1).backward(torch.tensor(td.astype(np.float64)))
    full = Wt.grad.numpy().reshape(2, -1)
    for k in (pkg.KERNEL_AUTO, pkg.KERNEL_GENERIC):
        plan = pkg.Plan(d, backward_kernel=k)
        plan.set_csr(np.array([0, 2, 3], np.int32), np.array([0, 4, 13], np.int32),
                     np.array([0.0, 1.5, 0.0], np.float32), [3])
        _, wd, _ = plan.backward(torch.from_numpy(td).to(dev), bottom=torch.from_numpy(x).to(dev), bottom_diff=None,
                                 weight_diff=True)
        flat = wd.cpu().numpy().reshape(2, -1)
        mask = np.zeros_like(flat, bool)
        mask[0, 0] = mask[0, 4] = mask[1, 13] = True
        assert np.all(flat[~mask] == 0)
        assert np.all(np.abs(flat[mask] - full[mask]) <= 1e-4 * np.abs(full).max()) and np.all(flat[mask] != 0)
        plan.close()


def test_forward_backward_graph_capture(pkg, dev, synth):
    """After one warm-up call, forward + backward of three layers captured into one graph: a generated-code transposed
    plan, a gather-kernel layer, a fuse_relu layer.  Two replays on new data, each checked against torch."""
    specs = [
        (synth.resnet50_3x3(N=2)[3], pkg.KERNEL_JIT, False),
        (_odd_shape(synth, ODD[2], 2), pkg.KERNEL_AUTO, False),
        (synth.shape("relu3x3", 2, 16, 12, 12, 24, 3, pad=1, sparsity=0.7), pkg.KERNEL_AUTO, True),
    ]
    layers = []
    for i, (s, k, relu) in enumerate(specs):
        w = synth.pruned_weights(s, 70 + i)
        b = synth.bias_vector(s, 80 + i)
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=relu), backward_kernel=k, tiling_batch=256)
        plan.weight_align(w)
        oh, ow = plan.out_hw
        bufs = dict(x=torch.zeros((s.N, s.C, s.H, s.W), device=dev), td=torch.zeros((s.N, s.M, oh, ow), device=dev),
                    y=torch.zeros((s.N, s.M, oh, ow), device=dev), bd=torch.zeros((s.N, s.C, s.H, s.W), device=dev),
                    wd=torch.zeros((s.M, s.C // s.group, s.KH, s.KW), device=dev),
                    bsd=torch.zeros((s.M,), device=dev) if b is not None else None,
                    b=torch.from_numpy(b).to(dev) if b is not None else None)
        layers.append((s, plan, w, b, relu, bufs))

    def step():
        for s, plan, w, b, relu, u in layers:
            plan.forward(u["x"], u["b"], u["y"])
            plan.backward(u["td"], bottom=u["x"], top=u["y"] if relu else None, bottom_diff=u["bd"],
                          weight_diff=u["wd"], bias_diff=u["bsd"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                      # warm-up: builds the backward state outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert layers[0][1].stat("bwd_data_kernel") == pkg.KERNEL_JIT
    assert layers[1][1].stat("bwd_data_kernel") == pkg.KERNEL_GENERIC
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    for rnd in range(2):
        inputs = []
        for k, (s, plan, w, b, relu, u) in enumerate(layers):
            x = synth.activations(s, 900 + 10 * rnd + k)
            td = _seeded(tuple(u["td"].shape), 950 + 10 * rnd + k)
            u["x"].copy_(torch.from_numpy(x))
            u["td"].copy_(torch.from_numpy(td))
            u["bd"].fill_(float("nan"))
            u["wd"].zero_()
            if u["bsd"] is not None:
                u["bsd"].zero_()
            inputs.append((x, td))
        g.replay()
        torch.cuda.synchronize()
        for (s, plan, w, b, relu, u), (x, td) in zip(layers, inputs):
            top = u["y"].cpu().numpy() if relu else None
            _check_against_torch(s, w, x, b, td, top, u["bd"].cpu().numpy(), u["wd"].cpu().numpy(),
                                 None if b is None else u["bsd"].cpu().numpy(), what=(s.name, rnd))
    for s, plan, *_ in layers:
        plan.close()


# ---- directed edges (wgrad_common.EDGES; test_backward_cpu.py runs the same shapes through backward_cpu) -----------------
def test_more_than_32767_output_channels_per_group_take_the_gather_kernel(pkg, dev, synth):
    """ocl fills the upper bits of the gather table's ttap, the entry kernel's grid.y is M."""
    s, w, x, b = edge_inputs(synth, "mg40000")
    for k, wk in ((pkg.KERNEL_AUTO, pkg.WGRAD_AUTO), (pkg.KERNEL_GENERIC, pkg.WGRAD_ENTRY)):
        plan, td, top, bd, wd, bsd = _run(pkg, dev, s, pkg.ConvDesc.from_shape(s), w, x, b, kernel=k, wgrad_kernel=wk)
        assert plan.stat("bwd_data_kernel") == pkg.KERNEL_GENERIC
        if wk == pkg.WGRAD_ENTRY:
            assert plan.stat("wgrad_kernel") == pkg.WGRAD_ENTRY
        _check_against_torch(s, w, x, b, td, top, bd, wd, bsd, what=(s.name, k))
        plan.close()
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s), backward_kernel=pkg.KERNEL_JIT)
    plan.weight_align(w)
    with pytest.raises(pkg.EscoinError, match="no transposed forward plan"):
        plan.backward(torch.zeros((s.N, s.M, 2, 2), device=dev))
    plan.close()


@pytest.mark.parametrize("name", ["lenet5x5_pad0", "5x5_pad4", "3x5_pad2x0", "group_pruned"])
def test_transposed_pads_and_a_fully_pruned_group_on_the_forced_fast_kernels(pkg, dev, synth, name):
    s, w, x, b = edge_inputs(synth, name)
    for k in (pkg.KERNEL_TILED, pkg.KERNEL_JIT):
        plan, td, top, bd, wd, bsd = _run(pkg, dev, s, pkg.ConvDesc.from_shape(s), w, x, b, kernel=k)
        assert plan.stat("bwd_data_kernel") == k
        _check_against_torch(s, w, x, b, td, top, bd, wd, bsd, what=(name, k))
        plan.close()


def test_partial_batches_on_a_fuse_relu_transposed_plan(pkg, dev, synth):
    s, w, x, b = edge_inputs(synth, "relu3x3_n7")
    xt, bt = torch.from_numpy(x).to(dev), torch.from_numpy(b).to(dev)
    td = _seeded((s.N, s.M) + synth.out_hw(s), 21)
    tdt = torch.from_numpy(td).to(dev)
    for k in (pkg.KERNEL_TILED, pkg.KERNEL_JIT):
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s, fuse_relu=True), backward_kernel=k, tiling_batch=256)
        plan.weight_align(w)
        top = plan.forward(xt, bt)
        top_np = top.cpu().numpy()
        full = None
        for n in (0, s.N, 1, 3, 6):      # 0 images first: a no-op that still builds the state
            out = torch.full((s.N, s.C, s.H, s.W), -7.5, device=dev)
            if n == 0:      # (an empty torch tensor has no address: the C entry point with the full blobs' pointers)
                import ctypes as C
                wd, bsd = torch.zeros((s.M, s.C, 3, 3), device=dev), torch.zeros((s.M,), device=dev)
                P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
                assert pkg.lib().escoin_backward(plan._h, P(xt), P(top), P(tdt), P(out), P(wd), P(bsd), 0,
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
            else:
                _, wd, bsd = plan.backward(tdt[:n], bottom=xt[:n], top=top[:n], bottom_diff=out[:n], weight_diff=True,
                                           bias_diff=True)
            torch.cuda.synchronize()
            assert plan.stat("bwd_data_kernel") == k
            got = out.cpu().numpy()
            assert np.all(got[n:] == -7.5), (k, n)
            if n == 0:
                assert not wd.cpu().numpy().any() and not bsd.cpu().numpy().any()
                continue
            _check_against_torch(s, w, x[:n], b, td[:n], top_np[:n], got[:n], wd.cpu().numpy(), bsd.cpu().numpy(), what=(k, n))
            if n == s.N:
                full = got
            assert got[:n].tobytes() == full[:n].tobytes(), (k, n)
        plan.close()


def test_sub_batch_launches_of_the_transposed_plan(pkg, dev, synth):
    s, w, x, b = edge_inputs(synth, "chunked")
    oh, ow = synth.out_hw(s)
    for k in (pkg.KERNEL_TILED, pkg.KERNEL_JIT):
        # three images of the transposed plan's bottom (top_diff) per launch: 11 images in four launches
        plan, td, top, bd, wd, bsd = _run(pkg, dev, s, pkg.ConvDesc.from_shape(s), w, x, b, kernel=k,
                                          max_launch_bytes=3 * s.M * oh * ow * 4 + 100)
        assert plan.stat("bwd_data_kernel") == k
        _check_against_torch(s, w, x, b, td, top, bd, wd, bsd, what=(s.name, k))
        plan.close()
        # No stat counts the launches, and a split cannot change a result.  That the option does reach the transposed
        # plan shows where it must refuse: with less than ONE image of top_diff per launch the transposed plan's launcher
        # says so (the plan's own forward, whose bottom the option also bounds, is never called here).
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s), backward_kernel=k, max_launch_bytes=s.M * oh * ow * 4 - 4)
        plan.weight_align(w)
        with pytest.raises(pkg.EscoinError, match="one image exceeds"):
            plan.backward(torch.from_numpy(td).to(dev))
        plan.close()


def test_a_weight_stream_beyond_the_lds_budget_refuses_forced_tiled_only(pkg, dev, synth):
    """Found by tools/fuzz_backward.py (profiles/backward_fuzz.md): the transposed descriptor passes the geometry
    predicate, but at tiling_batch 256 the stream kernel's weight stream (2 x 630 entries per group, 70 % dense 5 x 5) does
    not fit beside the input planes.  A forced TILED says so; AUTO and JIT compute the gradient."""
    s, w, x, b = edge_inputs(synth, "stream_budget")
    opts = dict(tiling_batch=256, max_launch_bytes=121060)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s), backward_kernel=pkg.KERNEL_TILED, **opts)
    plan.weight_align(w)
    with pytest.raises(pkg.EscoinError, match="weight stream does not fit the LDS budget"):
        plan.backward(torch.zeros((s.N, s.M) + synth.out_hw(s), device=dev))
    plan.close()
    for k in (pkg.KERNEL_AUTO, pkg.KERNEL_JIT):
        plan, td, top, bd, wd, bsd = _run(pkg, dev, s, pkg.ConvDesc.from_shape(s), w, x, b, kernel=k, **opts)
        assert plan.stat("bwd_data_kernel") == pkg.KERNEL_JIT, k
        _check_against_torch(s, w, x, b, td, top, bd, wd, bsd, what=(s.name, k))
        plan.close()


@pytest.mark.parametrize("name", ["overpad3x3", "nopad3x3", "nopad3x3_n4"])
def test_staged_weight_gradient_with_more_padding_than_the_kernel_reaches_and_with_none(pkg, dev, synth, name):
    s, w, x, b = edge_inputs(synth, name)
    for relu in (False, True):
        plan, td, top, bd, wd, bsd = _run(pkg, dev, s, pkg.ConvDesc.from_shape(s, fuse_relu=relu), w, x, b, relu=relu,
                                          wgrad_kernel=pkg.WGRAD_STAGED)
        assert plan.stat("wgrad_kernel") == pkg.WGRAD_STAGED
        _check_against_torch(s, w, x, b, td, top, bd, wd, bsd, what=(name, relu))
        _, vd, _ = plan.backward(torch.from_numpy(td).to(dev), bottom=torch.from_numpy(x).to(dev),
                                 top=None if top is None else torch.from_numpy(top).to(dev), bottom_diff=None, values_diff=True)
        assert vd.cpu().numpy().tobytes() == wd.reshape(-1)[csr_positions(plan)].tobytes(), (name, relu)
        plan.close()
