"""Plan option "deconv" through the op-sequence suite on the _cpu twins (d2s_seq_common.py has the layers, configurations and
backends; seq_common.run_sequence, the Driver and its checks are used as they are).  Needs no GPU: it proves
plan_model.DeconvModel, the skewed inputs and the seeds right before test_d2s_sequence_gpu.py puts a device behind the same
driver.  Also here: the model's own geometry against d2s_common's restatements, and that the driver fails where a deconv
backend goes wrong."""
import numpy as np
import pytest

import d2s_common as dc
import d2s_seq_common as ds
import errbound as eb
import seq_common as sq
import solver_common as sc
from plan_model import same_bits
from wgrad_common import tiled_ok

pytest.importorskip("torch")


# ---- no library ---------------------------------------------------------------------------------------------------------------
def test_the_seeds_are_the_first_that_cover():
    """seq_common.SEEDS' rule, held for every deconv configuration: the first three consecutive seeds from 1 over which every
    op of the vocabulary occurs at least twice; the vocabulary is OPS minus the recorded exclusions."""
    for cfg in ds.CONFIGS + ds.CPU_CONFIGS:
        assert ds.SEEDS[cfg.id] == ds.first_seeds(cfg), (cfg.id, ds.first_seeds(cfg))
        counts, _ = sq.coverage([cfg], ds.SEEDS)
        assert set(counts[cfg.id]) == set(sq.vocabulary(cfg)) and min(counts[cfg.id].values()) >= 2, (cfg.id, counts[cfg.id])
        assert all(op in sq.OPS and why for op, why in cfg.exclude.items())
    for cfg in ds.CONFIGS:
        assert set(sq.OPS) - set(sq.vocabulary(cfg)) == {"prune", "rewire", "dense_wgrad"}
    for cfg in ds.CPU_CONFIGS:
        assert set(sq.OPS) - set(sq.vocabulary(cfg)) == {"prune", "rewire", "dense_wgrad", "import_same", "import_fresh", "flip"}


def test_the_forced_inner_kernels_exist(synth):
    """The layers' inner stride-1 layers are inside the tiled kernels' geometry, so a forced KERNEL_JIT / KERNEL_TILED is not
    refused for its shape; and N = 3 leaves a partial batch of one image with two behind it."""
    for name, s in ds.LAYERS.items():
        assert tiled_ok(dc.inner_shape(synth, s)), name
    s = ds.LAYERS["DK4"]
    assert s.N == 3 and (s.C, s.M) == (24, 20) and dc.inner_dims(s)[0] == 4
    assert dc.inner_dims(ds.LAYERS["DK5G2"])[0] == 9 and ds.LAYERS["DK5G2"].group == 2


@pytest.mark.parametrize("cid", [c.id for c in ds.CPU_CONFIGS])
def test_the_model_speaks_the_layers_own_geometry(synth, cid):
    """DeconvModel against d2s_common: csr() is csr_of's form, dense() the blob, row_scale the per-output-channel exponent
    (shared by the P inner rows of the channel, and what errbound.skew applied), the bounds are d2s_common's."""
    cfg = ds.BY_ID[cid]
    inp = ds.make_inputs(cfg)
    s, m = inp.s, ds.initial_model(synth, cfg, inp)
    assert m.w_shape == inp.w0.shape == (s.C, s.M // s.group, s.KH, s.KW)
    assert np.array_equal(m.dense(), inp.w0) and np.array_equal(m.mask(), inp.w0 != 0)      # (+0 outside the pattern)
    for a, b in zip(m.csr(), dc.csr_of(s, inp.w0)):
        assert same_bits(np.asarray(a), np.asarray(b))
    # the scale: undoing it leaves every row's largest magnitude in (2^-1, 1] ... over output channels, not blob rows
    scale = m.row_scale(inp.row_exp, np.float32)
    assert scale.shape == (s.C, s.M // s.group, 1, 1)
    plain = ds.to_rows(s, inp.w0 / scale)
    assert np.all(np.abs(plain) <= 1) and set(inp.row_exp.tolist()) == set(eb.ROW_EXPONENTS)
    wi, _ = dc.inner_weights(s, scale * np.ones(m.w_shape, np.float32))
    P = dc.inner_dims(s)[0]
    for mm in range(s.M):       # every inner row of channel m carries m's exponent or is empty
        rows = wi[mm * P:(mm + 1) * P].reshape(P, -1)
        assert set(np.unique(rows).tolist()) <= {0.0, float(np.ldexp(1.0, inp.row_exp[mm]))}
    # the skew spans the range it promises
    big = np.abs(inp.w0[inp.w0 != 0])
    assert big.max() / big.min() > 2.0 ** 40
    want, B = m.forward_bound(inp.x, inp.b)
    want2, B2 = dc.forward_bound(eb, synth, s, inp.w0, inp.x, inp.b, cfg.relu)
    assert np.array_equal(want, want2) and np.array_equal(B, B2)
    assert m.wgrad_terms(2, inp.td.shape) == 2 * dc.inner_dims(s)[3] * dc.inner_dims(s)[4]


# ---- the sequences ------------------------------------------------------------------------------------------------------------
def _backend(pkg, synth, cfg):
    inp = ds.make_inputs(cfg)
    model = ds.initial_model(synth, cfg, inp)
    return inp, model, ds.DeconvCpuBackend(pkg, cfg, inp, model.csr())


def _run(pkg, synth, cfg, hyper, ops, what, backend_of=lambda b: b, finish=True):
    inp, model, backend = _backend(pkg, synth, cfg)
    worst = {}
    try:
        drv = sq.run_sequence(backend_of(backend), cfg, inp, hyper, ops, seed=what, worst=worst, model=model, finish=finish)
    finally:
        backend.close()
    for kernel, ratio in sorted(worst.items()):
        print("sequence %-16s %s  %-40s worst err/bound %.3g" % (cfg.id, what, kernel, ratio))
    return drv


CPU_CASES = [(c.id, seed) for c in ds.CPU_CONFIGS for seed in ds.SEEDS[c.id]]


@pytest.mark.parametrize("cid,seed", CPU_CASES, ids=["%s-%d" % c for c in CPU_CASES])
def test_random_sequences_on_the_cpu_twins(pkg, synth, cid, seed):
    cfg = ds.BY_ID[cid]
    hyper, ops = sq.generate(cfg, seed)
    _run(pkg, synth, cfg, hyper, ops, "seed %d" % seed)


@pytest.mark.parametrize("cid", [c.id for c in ds.CPU_CONFIGS])
def test_the_directed_lists_on_the_cpu_twins(pkg, synth, cid):
    """seq_common's directed lists, filtered by the configuration's vocabulary up front (sq.supported): updates from both
    sources around host readers, and the update list's life cycle (the twin reports no destinations: its checks are the
    forwards and backwards between the updates)."""
    cfg = ds.BY_ID[cid]
    hyper = dict(type=sc.ADAM, regularization=sc.REG_NONE, rate=1e-3, momentum=0.9, momentum2=0.999, delta=1e-8)
    _run(pkg, synth, cfg, hyper, sq.supported(cfg, sq.SOURCES_AND_READERS), "sources and readers")
    nothing = lambda drv: None  # noqa: E731
    hyper = dict(type=sc.SGD, regularization=sc.REG_L2, rate=1e-2, momentum=0.9, decay=1e-3)
    _run(pkg, synth, cfg, hyper, sq.supported(cfg, sq.list_lifecycle(nothing, nothing, nothing)), "update list")


# ---- the driver on a deconv backend that is wrong in one way ----------------------------------------------------------------------
class _Wrapper(object):
    def __init__(self, inner):
        self._inner = inner

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def fresh(self, csr):
        return self._inner.fresh(csr)


class DropsOneSetValues(_Wrapper):
    """The second set_values never reaches the plan: a copy of the weights an update missed."""
    calls = 0

    def set_values(self, v, source):
        self.calls += 1
        if self.calls != 2:
            self._inner.set_values(v, source)


class BackwardReadsAStaleCopy(_Wrapper):
    """The data gradient is computed on the values the plan had before its latest update (what an update that misses the
    inner backward state's copy looks like): the forward is right, only the backward shows it."""
    stale = None

    def set_values(self, v, source):
        self.stale = self._inner.plan.get_csr()[2].copy()
        self._inner.set_values(v, source)

    def backward(self, td, x, top, data, wgrad, bias, base=None):
        got = self._inner.backward(td, x, top, data, wgrad, bias, base)
        if self.stale is None or not data:
            return got
        now = self._inner.plan.get_csr()[2].copy()
        self._inner.set_values(self.stale, "host")
        bd = self._inner.backward(td, x, top, True, wgrad, False)[0]
        self._inner.set_values(now, "host")
        return (bd,) + tuple(got[1:])


class PhaseFromTheWrongPlane(_Wrapper):
    """Every top element comes from the plane of phase pw + 1 (mod sw) at its own inner position (i, j): what the unpack kernel
    gives when it reads pw from the wrong plane.  Positions whose neighbour the crop removed keep their own."""

    def forward(self, x, b, prefill=None, full=None):
        top = self._inner.forward(x, b, prefill, full)
        s, n = self._inner.inp.s, x.shape[0]
        ow = np.arange(top.shape[3])
        pw = (ow + s.pad_w) % s.stride_w
        src = np.where(pw < s.stride_w - 1, ow + 1, ow - (s.stride_w - 1))
        src = np.where((src >= 0) & (src < ow.size), src, ow)
        out = top.copy()
        out[:n] = top[:n][:, :, :, src]
        return out


SELF_CHECKS = {
    "drops_a_set_values": (DropsOneSetValues, 2,
                           [("set_values", dict(source="host", seed=1)), sq.BWD, ("set_values", dict(source="device", seed=3)),
                            ("forward", dict(bias=True, partial=False)), ("get_csr", {})]),
    "backward_reads_a_stale_copy": (BackwardReadsAStaleCopy, 2,
                                    [sq.BWD, ("set_values", dict(source="device", seed=2)), sq.BWD, ("get_csr", {})]),
    "phase_from_the_wrong_plane": (PhaseFromTheWrongPlane, 0, [("forward", dict(bias=True, partial=False)), sq.BWD]),
}


@pytest.mark.parametrize("name", sorted(SELF_CHECKS))
def test_the_driver_fails_at_the_step_where_a_deconv_backend_goes_wrong(pkg, synth, name):
    wrapper, at, ops = SELF_CHECKS[name]
    cfg = ds.BY_ID["cpu_deconv_g2"]
    hyper = dict(type=sc.SGD, regularization=sc.REG_NONE, rate=1e-2, momentum=0.9)
    _run(pkg, synth, cfg, hyper, ops, name)          # the honest backend passes the same ops
    with pytest.raises(sq.SequenceError) as e:
        _run(pkg, synth, cfg, hyper, ops, name, backend_of=wrapper)
    assert e.value.index == at, (name, e.value.index, str(e.value.cause))


# ---- the numpy restatement itself: the faults the device tests rely on it to show ------------------------------------------------
@pytest.mark.parametrize("name", list(dc.SHAPES))
def test_pack_selects_and_unpack_reads_its_own_phase(name):
    """d2s_common.pack / unpack are what test_d2s_gpu holds the two kernels to, bit for bit.  Two plausible faults, restated
    in numpy, must differ from them on every shape they can differ on: a pack that multiplies by the mask (a masked NaN
    survives, a masked negative becomes -0.0), and an unpack that reads phase pw from plane ph."""
    s = dc.make(name)
    P, _, _, hi, wi = dc.inner_dims(s)
    rs = np.random.RandomState(11)
    td = rs.uniform(-1, 1, (s.N, s.M) + dc.out_hw(s)).astype(np.float32)
    for value in (0.0, -0.0, -1.0, np.nan):
        top = np.ones(td.shape, np.float32)
        top[0, 0, 0, 0] = value
        tdn = td.copy()
        tdn[0, 0, 0, 0] = np.nan
        g = dc.pack(s, tdn, top)
        assert not np.isnan(g).any() and np.array_equal(g, dc.pack(s, np.where(np.isnan(tdn), 0, tdn), None))
        with np.errstate(invalid="ignore"):
            multiplied = dc.pack(s, tdn * (top > 0).astype(np.float32))
        assert np.isnan(multiplied).sum() == 1, (name, value)
    # unpack(pack(.)) is the identity on the top's positions: pack is a bijection onto the inner positions it fills
    assert np.array_equal(dc.unpack(s, dc.pack(s, td)), td)
    assert int((dc.pack(s, np.ones_like(td)) != 0).sum()) == td.size
    if s.stride_h == s.stride_w and s.stride_h > 1:
        t = rs.uniform(-1, 1, (s.N, s.M * P, hi, wi)).astype(np.float32)
        swapped = t.reshape(s.N, s.M, s.stride_h, s.stride_w, hi, wi).transpose(0, 1, 3, 2, 4, 5).reshape(t.shape)
        oh, ow = dc.out_hw(s)
        if min(oh, ow) > 1:
            assert not np.array_equal(dc.unpack(s, np.ascontiguousarray(swapped)), dc.unpack(s, t)), name
