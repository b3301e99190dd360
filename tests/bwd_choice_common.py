"""The backward's kernel choice (csrc/align_rules.h bwd_choice) through tests/cpp/bwd_choice_check.cpp: the case table with
its hand-written expectations, and the helpers that build the checker (plain g++, no ROCm include path) and run it.
Shared by tests/test_bwd_choice.py (host) and tests/test_bwd_choice_gpu.py (the same cases on the device)."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

AUTO, GENERIC, TILED, DENSE, JIT, BWD_MFMA = 0, 1, 2, 3, 4, 5          # option "backward_kernel"
W_AUTO, W_ENTRY, W_STAGED, W_MFMA = 0, 1, 2, 3                         # option / stat "wgrad_kernel"
EINVAL = -1
MFMA_LDS = 4 * 2 * 2 * 32 * 65      # both MFMA kernels: 2 buffers x 2 tiles x 32 steps x rows of 65 floats

# the refusals, copied from the ladder as it stood in sconv_backward.hip bwd_build, in its order
E_MG = "backward: more than 65535 output channels per group"
E_GRID = "backward: grid dimension exceeds 65535"
E_FORCED = ("backward_kernel: this plan has no transposed forward plan (needs a float plan, stride 1, "
            "pad <= dilation * (kernel - 1)); only the gather kernel serves it")
E_STAGED = ("wgrad_kernel: the staged weight-gradient kernel needs a float plan with stride 1 whose "
            "chunk tile of one input channel fits the LDS budget; only the entry kernel serves this plan")
E_WGM = ("wgrad_kernel: the MFMA weight-gradient kernel needs a float plan whose pixel, weight and "
         "image indices fit 31 bits; the entry kernel serves this plan")
E_DGM = ("backward_kernel: the MFMA data-gradient kernel needs a float plan whose pixel, top and "
         "matrix indices fit 31 bits; the gather kernel serves this plan")
E_NNZ = "backward: more than 2^31 nonzeros"

SHAPE_FIELDS = ("N", "C", "H", "W", "M", "KH", "KW", "pad_h", "pad_w", "stride_h", "stride_w", "dil_h", "dil_w", "group")
BASE = dict(N=2, C=4, H=6, W=6, M=4, KH=3, KW=3, pad_h=1, pad_w=1, stride_h=1, stride_w=1, dil_h=1, dil_w=1, group=1)
S2 = dict(stride_h=2, stride_w=2)
NNZ = 72      # half of 4 x 4 x 3 x 3


def case(name, shape=None, bwd=AUTO, wgrad=W_AUTO, block=0, s2d=0, f64=0, nnz=NNZ, **expect):
    """expect: rc + error for a refusal; data and / or wgrad_kernel, wgrad_lds_bytes, dgrad_lds_bytes otherwise."""
    return dict(name=name, shape=dict(BASE, **(shape or {})), bwd=bwd, wgrad=wgrad, block=block, s2d=s2d, f64=f64, nnz=nnz,
                expect=dict({"rc": 0, "error": ""}, **expect))


def refused(name, error, **kw):
    return case(name, rc=EINVAL, error=error, data="", wgrad_kernel=0, wgrad_lds_bytes=0, dgrad_lds_bytes=0, **kw)


# All cases: N=2, C=4, H=W=6, M=4, 256 compute units, unless noted.  The expectations are read off the parent's ladder by
# hand.  Where AUTO's weight-gradient rule runs on the 3x3 stride-1 base shape, it takes the staged kernel: one chunk,
# 18 entries per row, so the entry kernel's model gives 21.3 + 0.153 + 0.3 x (3.0 + 1.138 x 18) = 28.5 us and the staged
# kernel's 13.4 + 0.4 x (19.3 + 1.02 + 0.426 x 18) = 24.6 us; its tile is 16 padded rows of 8 floats for 4 channels.
CASES = [
    # 3x3 stride 1 pad 1
    case("s1_auto", data="transposed", wgrad_kernel=W_STAGED, wgrad_lds_bytes=4 * 4 * 16 * 8, dgrad_lds_bytes=0),
    case("s1_generic", bwd=GENERIC, data="gather", dgrad_lds_bytes=0),
    case("s1_bwd_mfma", bwd=BWD_MFMA, data="mfma", dgrad_lds_bytes=MFMA_LDS),
    # 3x3 stride 2
    case("s2_auto", S2, data="gather", wgrad_kernel=W_ENTRY, wgrad_lds_bytes=0, dgrad_lds_bytes=0),
    refused("s2_tiled", E_FORCED, shape=S2, bwd=TILED),
    refused("s2_jit", E_FORCED, shape=S2, bwd=JIT),
    refused("s2_dense", E_FORCED, shape=S2, bwd=DENSE),
    # ... with an S2dState
    case("s2d_auto", S2, s2d=1, data="inner", wgrad_kernel=W_ENTRY, dgrad_lds_bytes=0),
    case("s2d_tiled", S2, s2d=1, bwd=TILED, data="inner"),
    case("s2d_jit", S2, s2d=1, bwd=JIT, data="inner"),
    case("s2d_dense", S2, s2d=1, bwd=DENSE, data="inner"),
    case("s2d_generic", S2, s2d=1, bwd=GENERIC, data="gather"),
    case("s2d_bwd_mfma", S2, s2d=1, bwd=BWD_MFMA, data="mfma", dgrad_lds_bytes=MFMA_LDS),
    # pad beyond dilation * (kernel - 1); the channel limit of a plan
    case("pointwise_pad1", dict(KH=1, KW=1), nnz=8, data="gather"),
    case("mg_32768", dict(M=32768), nnz=32768 * 18, data="gather"),
    # double plans
    case("f64_auto", f64=1, data="gather", wgrad_kernel=W_ENTRY, wgrad_lds_bytes=0, dgrad_lds_bytes=0),
    refused("f64_staged", E_STAGED, f64=1, wgrad=W_STAGED),
    refused("f64_wgrad_mfma", E_WGM, f64=1, wgrad=W_MFMA),
    refused("f64_bwd_mfma", E_DGM, f64=1, bwd=BWD_MFMA),
    # option "wgrad_kernel"
    refused("s2_staged", E_STAGED, shape=S2, wgrad=W_STAGED),
    case("s2_wgrad_mfma", S2, wgrad=W_MFMA, data="gather", wgrad_kernel=W_MFMA, wgrad_lds_bytes=MFMA_LDS, dgrad_lds_bytes=0),
    # AUTO on the geometries of tests/golden/align_cases.json "wgrad_entry" and "wgrad_staged" (5 % of the weights kept)
    case("auto_entry", dict(N=256, C=192, H=28, W=28, M=32, KH=1, KW=1, pad_h=0, pad_w=0), nnz=307,
         data="transposed", wgrad_kernel=W_ENTRY, wgrad_lds_bytes=0),
    case("auto_staged", dict(N=256, C=64, H=56, W=56, M=64, KH=1, KW=1, pad_h=0, pad_w=0), nnz=205,
         data="transposed", wgrad_kernel=W_STAGED),
    # the grid, the nonzero count
    refused("mg_65536", E_MG, shape=dict(M=65536)),
    refused("n_65536", E_GRID, shape=dict(N=65536)),
    refused("nnz_2_31", E_NNZ, nnz=2 ** 31),
    # two violations: the ladder's first
    refused("mg_and_n", E_MG, shape=dict(M=65536, N=65536)),
    refused("s2_tiled_staged", E_FORCED, shape=S2, bwd=TILED, wgrad=W_STAGED),
    refused("f64_staged_bwd_mfma", E_STAGED, f64=1, wgrad=W_STAGED, bwd=BWD_MFMA),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def build_checker(tmp_path):
    """tests/cpp/bwd_choice_check.cpp against the rules and the two builders: g++, -Icsrc -Iinclude, nothing of ROCm."""
    csrc = os.path.join(ROOT, "caffe-escoin_amd", "csrc")
    exe = str(tmp_path / "bwd_choice_check")
    srcs = [os.path.join(ROOT, "tests", "cpp", "bwd_choice_check.cpp")] + [os.path.join(csrc, f) for f in
                                                                         ("align_rules.cpp", "stream_builder.cpp", "jit_codegen.cpp")]
    flags = ["g++", "-O2", "-std=c++17", "-I" + csrc, "-I" + os.path.join(ROOT, "include")]
    procs = [subprocess.Popen(flags + ["-c", s, "-o", str(tmp_path / (os.path.basename(s) + ".o"))]) for s in srcs]
    assert all(p.wait() == 0 for p in procs)
    subprocess.check_call(flags + ["-o", exe] + [str(tmp_path / (os.path.basename(s) + ".o")) for s in srcs] + ["-lpthread"])
    return exe


def run_checker(exe, tmp_path, cases, n_cu=256, nnz=None):
    """What bwd_choice decides for `cases` on a device of n_cu compute units: one dict per case.  nnz: per case name, a
    count that replaces the table's."""
    lines = []
    for c in cases:
        row = [c["shape"][k] for k in SHAPE_FIELDS] + [c["bwd"], c["wgrad"], c["block"], c["s2d"], c["f64"],
                                                      (nnz or {}).get(c["name"], c["nnz"]), n_cu]
        lines.append(" ".join(str(int(v)) for v in row))
    manifest = str(tmp_path / "bwd_choice_manifest.txt")
    with open(manifest, "w") as f:
        f.write("\n".join(lines) + "\n")
    out = subprocess.run([exe, manifest], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = out.stdout.decode()
    assert out.returncode == 0, text
    got = [json.loads(l) for l in text.splitlines()]
    assert len(got) == len(cases), text
    return got
