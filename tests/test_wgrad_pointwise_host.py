"""Plan option "wgrad_pointwise" without a GPU: the option's values and the package constant, and -- through
tests/cpp/wgrad_pointwise_tables_check.cpp, compiled with plain g++ and no ROCm include path (that compile is the proof
that the rule and the tables are host-only) -- the serve predicate, the tiling with the LDS bytes it reports and the tables
derived from the CSR, each against a numpy restatement of csrc/align_rules.h and csrc/csr_tables.h on every shape of
wgrad_pointwise_common.py under the two test options; and bwd_choice with the option off against today's decisions."""
import json
import os
import subprocess

import numpy as np
import pytest

import bwd_choice_common as bc
import d2s_common
import wgrad_pointwise_common as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CU = 256


def test_option_values_and_package_constant(pkg, synth):
    assert pkg.WGRAD_POINTWISE == 4 == pc.WGRAD_POINTWISE
    assert (pkg.WGRAD_AUTO, pkg.WGRAD_ENTRY, pkg.WGRAD_STAGED, pkg.WGRAD_MFMA) == (0, 1, 2, 3)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(pc.make(synth, "pw_onepx")))
    for key, bad in (("wgrad_pointwise", (-1, 2)), ("wgrad_pointwise_tile_entries", (-1,))):
        for v in bad:
            with pytest.raises(pkg.EscoinError) as e:
                plan.set_option(key, v)
            assert "failed (-1)" in str(e.value) and key in str(e.value)      # ESCOIN_EINVAL
    plan.set_option("wgrad_pointwise", 1)
    plan.set_option("wgrad_pointwise", 0)
    plan.set_option("wgrad_pointwise_tile_entries", 64)
    plan.set_option("wgrad_pointwise_tile_entries", 0)
    # it is not a value of "wgrad_kernel"
    with pytest.raises(pkg.EscoinError) as e:
        plan.set_option("wgrad_kernel", 4)
    assert "failed (-1)" in str(e.value) and "wgrad_kernel" in str(e.value)
    # (that the option may be set on a device-aligned plan, as "wgrad_kernel" may, is test_wgrad_pointwise_gpu.py's)
    plan.close()
    plan = pkg.Plan(pkg.ConvDesc.from_shape(pc.make(synth, "pw_onepx")), wgrad_pointwise=1, wgrad_pointwise_tile_entries=300)
    plan.close()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """g++, -Icsrc -Iinclude, nothing of ROCm."""
    tmp = tmp_path_factory.mktemp("pw")
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    out = str(tmp / "wgrad_pointwise_tables_check")
    srcs = [os.path.join(ROOT, "tests", "cpp", "wgrad_pointwise_tables_check.cpp")] + [
        os.path.join(csrc, f) for f in ("align_rules.cpp", "csr_tables.cpp", "stream_builder.cpp", "jit_codegen.cpp")]
    flags = ["g++", "-O1", "-std=c++17", "-Wall", "-I" + csrc, "-I" + os.path.join(ROOT, "include")]
    procs = [subprocess.Popen(flags + ["-c", s, "-o", str(tmp / (os.path.basename(s) + ".o"))]) for s in srcs]
    assert all(p.wait() == 0 for p in procs)
    subprocess.check_call(flags + ["-o", out] + [str(tmp / (os.path.basename(s) + ".o")) for s in srcs] + ["-lpthread"])
    return out


def _run(exe, tmp_path, s, rp=None, ci=None, ng=None, f64=False, block=0, tile_entries=0, n_cu=N_CU, nnz=-1):
    mg = s.M // s.group
    words = [s.N, s.C, s.H, s.W, s.M, s.KH, s.KW, s.pad_h, s.pad_w, s.stride_h, s.stride_w, s.dil_h, s.dil_w, s.group, int(f64),
             block, tile_entries, n_cu, nnz]
    if nnz < 0:
        base = 0
        for grp in range(s.group):
            words += [int(v) for v in rp[grp * (mg + 1):(grp + 1) * (mg + 1)]]
            words += [int(v) for v in ci[base:base + int(ng[grp])]]
            base += int(ng[grp])
    path = str(tmp_path / "case.txt")
    with open(path, "w") as f:
        f.write(" ".join(str(w) for w in words) + "\n")
    out = subprocess.run([exe, "tables", path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    text = out.stdout.decode()
    assert out.returncode == 0, text
    rows = {}
    for line in text.splitlines():
        parts = line.split()
        rows[parts[0]] = np.array([int(v) for v in parts[1:]], np.int64)
    return rows


# ---- the numpy restatement of align_rules.h pw_plan and csr_tables.h pw_tables ---------------------------------------------
def _tiles_of(mask, cblk, cap, height):
    """mask [group][Mg][Cg] bool (None rows: every row full).  (c-block-0 tiles, the others): (grp, row0, rows, c0, chans, items)."""
    first, rest = [], []
    groups, mg, cg = mask.shape
    for grp in range(groups):
        for b, c0 in enumerate(range(0, cg, cblk)):
            chans = min(cblk, cg - c0)
            cnt = mask[grp, :, c0:c0 + chans].sum(axis=1)
            out = first if b == 0 else rest
            cur = None                       # [row0, items, last row with an entry]

            def close(end):
                rows = end - cur[0] if b == 0 else cur[2] - cur[0] + 1
                if rows > 0 and (b == 0 or cur[1] > 0):
                    out.append((grp, cur[0], rows, c0, chans, cur[1]))
            for m in range(mg):
                if cur is not None and (cur[1] + cnt[m] > cap or m - cur[0] >= height):
                    close(m)
                    cur = None
                if cur is None:
                    if b > 0 and cnt[m] == 0:
                        continue
                    cur = [m, 0, m]
                cur[1] += int(cnt[m])
                if cnt[m] > 0:
                    cur[2] = m
            if cur is not None:
                close(mg)
    return first, rest


def _plan_of(s, synth, mask, nnz, block, tile_entries, n_cu):
    oh, ow = synth.out_hw(s)
    chunks = -(-s.N * oh * ow // pc.CHUNK)
    mg, cg = s.M // s.group, s.C // s.group
    cap = min(tile_entries, pc.MAX_TILE_ENTRIES) if tile_entries > 0 else pc.MAX_TILE_ENTRIES
    cblk = min(cg, pc.MAX_CHANNEL_BLOCK, cap)
    if block > 0:
        cblk = min(cblk, block)
    height = min(mg, pc.MAX_SLICE_ROWS, pc.MAX_LDS_ROWS - cblk)
    while True:
        first, rest = _tiles_of(mask, cblk, cap, height)
        if height <= pc.MIN_SLICE_ROWS or nnz * chunks < pc.SPLIT_WORK or chunks * (len(first) + len(rest)) >= 2 * n_cu:
            break
        height = max(pc.MIN_SLICE_ROWS, height // 2)
    tiles = first + rest
    fullest = max(t[5] for t in tiles)
    lane = 1
    while pc.THREADS * lane < fullest:
        lane *= 2
    rows_max, chans_max = max(t[2] for t in tiles), max(t[4] for t in tiles)
    line = [pc.STEP, pc.PITCH, cblk, lane, cap, chunks, rows_max, chans_max, 4 * pc.PITCH * (rows_max + chans_max), pc.LDS_BUDGET,
            len(first), len(tiles)]
    return line, tiles


def _mask(s, rp, ci, ng):
    mg, cg = s.M // s.group, s.C // s.group
    mask = np.zeros((s.group, mg, cg), bool)
    ent = np.full((s.group, mg, cg), -1, np.int64)
    base = 0
    for grp in range(s.group):
        r = rp[grp * (mg + 1):(grp + 1) * (mg + 1)]
        for m in range(mg):
            cols = ci[base + r[m]:base + r[m + 1]]
            mask[grp, m, cols] = True
            ent[grp, m, cols] = np.arange(base + r[m], base + r[m + 1])
        base += int(ng[grp])
    return mask, ent


def _check(exe, tmp_path, synth, s, rp, ci, ng, block, tile_entries, what):
    got = _run(exe, tmp_path, s, rp, ci, ng, block=block, tile_entries=tile_entries)
    assert got["serves"].tolist() == [1], what
    mask, ent_of = _mask(s, rp, ci, ng)
    nnz = int(mask.sum())
    line, tiles = _plan_of(s, synth, mask, nnz, block, tile_entries, N_CU)
    assert got["plan"].tolist() == line, what
    bline, btiles = _plan_of(s, synth, np.ones_like(mask), nnz, block, tile_entries, N_CU)
    assert got["bound"].tolist() == bline, what
    assert got["btiles"].reshape(-1, 6).tolist() == [list(t) for t in btiles], what
    # the invariants: the LDS budget, the cap, the lanes
    step, pitch, cblk, lane, cap, chunks, rows_max, chans_max, lds, budget, bias_tiles, n_tiles = line
    assert 0 < lds <= budget == pc.LDS_BUDGET and lane in (1, 2, 4, 8, 16) and cap <= pc.MAX_TILE_ENTRIES, what
    assert rows_max <= pc.MAX_SLICE_ROWS, what
    tile = got["tile"].reshape(-1, 8)
    assert len(tile) == n_tiles == len(tiles), what
    ent, pk = got["ent"], got["pk"]
    assert len(ent) == len(pk) == max(nnz, 1), what
    seen = np.zeros(max(nnz, 1), np.int64)
    bias_rows = np.zeros((s.group, s.M // s.group), np.int64)
    first = 0
    for k, (t, want) in enumerate(zip(tile, tiles)):
        grp, row0, rows, c0, chans, f0, items, zero = [int(v) for v in t]
        assert (grp, row0, rows, c0, chans, items) == want and f0 == first and zero == 0, (what, k)
        assert items <= cap <= pc.THREADS * pc.MAX_LANE_ENTRIES and items <= pc.THREADS * lane, (what, k)
        assert rows + chans <= pc.MAX_LDS_ROWS and 4 * pitch * (rows + chans) <= lds, (what, k)
        assert (k < bias_tiles) == (c0 == 0), (what, k)
        if c0 == 0:
            bias_rows[grp, row0:row0 + rows] += 1
        # the tile's entries in CSR order, each with its two rows of the LDS image
        sub = ent_of[grp, row0:row0 + rows, c0:c0 + chans]
        r, c = np.nonzero(sub >= 0)
        assert np.array_equal(ent[f0:f0 + items], sub[r, c]), (what, k)
        assert np.array_equal(pk[f0:f0 + items] >> 16, r) and np.array_equal(pk[f0:f0 + items] & 0xffff, rows + c), (what, k)
        assert np.all((pk[f0:f0 + items] >> 16) < rows) and np.all((pk[f0:f0 + items] & 0xffff) < rows + chans), (what, k)
        seen[ent[f0:f0 + items]] += 1
        first += items
    if nnz:
        assert first == nnz and np.all(seen == 1), what        # every entry exactly once
    else:
        assert first == 0 and n_tiles == bias_tiles, what      # an empty pattern: the bias tiles alone
    assert np.all(bias_rows == 1), what                        # the bias: every row of every group once
    return line


def _csr(pkg, synth, name):
    s = pc.make(synth, name)
    w = synth.pruned_weights(s, 11)
    if name == "pw_g3":
        w = pc.emptied(w, s)
    plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
    plan.weight_align_cpu(w)
    rp, ci, _, ng = plan.get_csr()
    plan.close()
    return s, rp, ci, ng


@pytest.mark.parametrize("name", list(pc.CONV) + ["pw_fc_inner", "pw_deconv_inner"])
def test_tiling_and_tables_equal_their_numpy_restatement(pkg, synth, exe, tmp_path, name):
    if name == "pw_fc_inner":
        s = pc.fc_inner(synth)
        outer = pc.make(synth, "pw_fc")
        plan = pkg.Plan(pkg.ConvDesc.from_shape(outer))
        plan.weight_align_cpu(synth.pruned_weights(outer, 11))
        rp, ci, _, ng = plan.get_csr()           # "b2s": the inner plan runs on the outer CSR
        plan.close()
    elif name == "pw_deconv_inner":
        d = pc.DECONV
        s = d2s_common.inner_shape(synth, d)
        assert (s.KH, s.KW, s.pad_h, s.pad_w, s.M) == (1, 1, 0, 0, 28)
        wi, _ = d2s_common.inner_weights(d, d2s_common.weights(d))
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
        plan.weight_align_cpu(wi)
        rp, ci, _, ng = plan.get_csr()
        plan.close()
    else:
        s, rp, ci, ng = _csr(pkg, synth, name)
    lines = {}
    for block in pc.CHANNEL_BLOCKS:
        for te in pc.TILE_ENTRIES:
            lines[(block, te)] = _check(exe, tmp_path, synth, s, rp, ci, ng, block, te, (name, block, te))
    if name == "pw_dense":
        assert lines[(0, 0)][3] == 16 and lines[(0, 0)][11] == 1       # 2800 entries in one tile: E = 16
        assert lines[(0, 64)][11] > 40 and lines[(1, 0)][2] == 1       # the options split it
    # a double plan is not served
    assert _run(exe, tmp_path, s, rp, ci, ng, f64=True)["serves"].tolist() == [0]


def test_an_empty_pattern_is_served_with_the_bias_tiles_alone(pkg, synth, exe, tmp_path):
    s = pc.make(synth, "pw_g3")
    mg = s.M // s.group
    rp, ci, ng = np.zeros(s.group * (mg + 1), np.int64), np.zeros(0, np.int64), np.zeros(s.group, np.int64)
    for block in pc.CHANNEL_BLOCKS:
        _check(exe, tmp_path, synth, s, rp, ci, ng, block, 0, ("empty", block))


def test_predicate(pkg, synth, exe, tmp_path):
    """Served: float, 1x1, pad 0, any stride and group count; N*OH*OW, C*H*W and nnz below 2^31; at most 65535 chunks."""
    def serves(s, **kw):
        return _run(exe, tmp_path, s, nnz=kw.pop("nnz", 1), **kw)["serves"].tolist() == [1]
    for name in list(pc.CONV) + ["pw_fc"]:
        assert serves(pc.make(synth, name)), name
        assert not serves(pc.make(synth, name), f64=True), name
    for name in pc.NOT_PW:
        assert not serves(pc.make(synth, name)), name
    assert not serves(synth.shape("pw_1x3", 2, 4, 5, 5, 4, 1, KW=3, pad_w=1, sparsity=0.0))
    assert serves(synth.shape("pw_s3_g2", 2, 4, 7, 9, 4, 1, stride=3, group=2, sparsity=0.0))
    # nnz: 2^31 - 1 is served, 2^31 is not
    s = pc.make(synth, "pw_straddle")
    assert serves(s, nnz=2 ** 31 - 1) and not serves(s, nnz=2 ** 31)
    # the chunks are grid y: 65535 of them are served, one pixel more is not (long before N*OH*OW reaches 2^31)
    assert serves(synth.shape("pw_chunks", 65535, 1, 32, 32, 1, 1, sparsity=0.0))
    assert not serves(synth.shape("pw_chunks1", 1, 1, 8192, 8192, 1, 1, sparsity=0.0))          # 65536 chunks
    assert not serves(synth.shape("pw_pix31", 1 << 15, 1, 256, 256, 1, 1, sparsity=0.0))        # 2^31 pixels
    # C*H*W: 2^31 is not served whatever the stride makes of the pixels
    assert not serves(synth.shape("pw_chw31", 1, 1 << 15, 256, 256, 1, 1, stride=256, sparsity=0.0))
    assert serves(synth.shape("pw_chw", 1, (1 << 15) - 1, 256, 256, 1, 1, stride=256, sparsity=0.0))


# ---- bwd_choice --------------------------------------------------------------------------------------------------------------
def _choice(exe, tmp_path, cases, option, tile_entries=0):
    lines = []
    for c in cases:
        row = [c["shape"][k] for k in bc.SHAPE_FIELDS] + [c["bwd"], c["wgrad"], c["block"], c["s2d"], c["f64"], c["nnz"], N_CU,
                                                          option, tile_entries]
        lines.append(" ".join(str(int(v)) for v in row))
    manifest = str(tmp_path / "pw_choice_manifest.txt")
    with open(manifest, "w") as f:
        f.write("\n".join(lines) + "\n")
    out = subprocess.run([exe, "choice", manifest], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0, out.stdout.decode()
    return [json.loads(l) for l in out.stdout.decode().splitlines()]


def test_bwd_choice_with_the_option_off_is_todays_and_on_changes_served_auto_plans_only(exe, tmp_path):
    today = bc.run_checker(bc.build_checker(tmp_path), tmp_path, bc.CASES, n_cu=N_CU)
    off = _choice(exe, tmp_path, bc.CASES, 0)
    assert off == today                                           # field for field
    for c, got in zip(bc.CASES, off):
        for k, v in c["expect"].items():
            assert got[k] == v, (c["name"], k)
    on = _choice(exe, tmp_path, bc.CASES, 1)
    changed = []
    for c, a, b in zip(bc.CASES, off, on):
        sh = c["shape"]
        served = (sh["KH"], sh["KW"], sh["pad_h"], sh["pad_w"]) == (1, 1, 0, 0) and not c["f64"] and c["wgrad"] == bc.W_AUTO and a["rc"] == 0
        if served:
            changed.append(c["name"])
            assert b["wgrad_kernel"] == pc.WGRAD_POINTWISE and 0 < b["wgrad_lds_bytes"] <= pc.LDS_BUDGET, c["name"]
            assert dict(b, wgrad_kernel=0, wgrad_lds_bytes=0) == dict(a, wgrad_kernel=0, wgrad_lds_bytes=0), c["name"]
        else:
            assert a == b, c["name"]
    assert sorted(changed) == ["auto_entry", "auto_staged"]
    # a forced kernel wins over the option
    pw = dict(N=3, C=40, H=19, W=19, M=70, KH=1, KW=1, pad_h=0, pad_w=0)
    forced = [bc.case("pw_auto", pw, nnz=560), bc.case("pw_entry", pw, wgrad=bc.W_ENTRY, nnz=560),
              bc.case("pw_staged", pw, wgrad=bc.W_STAGED, nnz=560), bc.case("pw_mfma", pw, wgrad=bc.W_MFMA, nnz=560)]
    got = _choice(exe, tmp_path, forced, 1)
    assert [g["wgrad_kernel"] for g in got] == [pc.WGRAD_POINTWISE, bc.W_ENTRY, bc.W_STAGED, bc.W_MFMA]
    without = _choice(exe, tmp_path, forced, 0)
    assert without[1:] == got[1:] and without[0]["wgrad_kernel"] in (bc.W_ENTRY, bc.W_STAGED)
