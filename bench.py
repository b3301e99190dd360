#!/usr/bin/env python3
"""bench.py -- conv-layer forward images/s of the direct-sparse-convolution path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload resnet50|alexnet|googlenet|lenet]
                    [--global-batch B] [--dump-outputs DIR] [--full]

A "step" is one pass of the hot path (escoin_forward, the Forward_gpu drop-in) over one batch
of synthetic input for every conv layer of the workload.  Default workload = BASELINE.json's
configs[2]: the 16 ResNet-50 3x3 branch2b layers at 90 % weight sparsity, batch 256 per GPU,
fp32.  For N > 1 there is one process per GPU: either the caller starts them (`python -m
torch.distributed.run --nproc-per-node N bench.py --gpus N ...`, RANK / WORLD_SIZE in the
environment) or `python bench.py --gpus N` starts them ITSELF -- the way the reference's one
command starts a worker per GPU (tools/caffe.cpp:254-256, parallel.cpp:328-358): the parent
spawns torch.distributed.run as a child process before anything has touched the GPU, never
initialises HIP itself, relays rank 0's JSON line and exits with the children's code.  The batch
dimension is sharded, the sparse weights are broadcast once from rank 0 over RCCL, and no
collective sits in the timed region.  Default = weak scaling (256 images per GPU);
`--global-batch 2048` = BASELINE.json's configs[3] as strong scaling (2048 / N images per GPU).

A plain run does only what its headline figure needs: set-up (WeightAlign, broadcast, inputs), W
warm-up steps, the settle loop (--settle-ms), ONE timed region of exactly K steps (`ms_per_step` =
its wall time / K, `value` = images/s from it), the outputs if --dump-outputs is given, and the
result line.  `--dump-outputs DIR` writes rank 0's top blob of every layer after the last timed step
as DIR/top<layer id>_<layer name>.npy (float32; a fixed, seeded sample where the blob is larger
than its share of 48 MB).  The inputs depend on the arguments only, so two builds can be compared
output for output.

`--full` adds everything else the benchmark measures or checks, after (never inside) the headline
region unless said otherwise: K cold steps before the settle loop (`ms_per_step_cold`), R timed
regions of K steps (--repeats, `value` from the median one) with per-launch events in a sample of
the steps (`roofline`), a throw-away plan that prices the process's first WeightAlign
(`first_load_ms`), every rank's images of every distinct layer shape against the CPU oracle
(`parity_max_rel_err`, the checker only), for N > 1 rank 0's recomputation of two images of every
other rank against that rank's per-image checksums, the other single-GPU configurations and the
sparsity sweep (default ResNet run), and the CPU baselines.

Rank 0 prints ONE JSON line on stdout (everything else goes to stderr).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E peak 8.0 TB/s (spec)
# Default (timed steps, warm-up steps) per workload: about 40 ms of warm-up and 200 ms timed.  With 5
# warm-up steps the chip had not settled (clocks, caches): 20 timed steps of the AlexNet set
# (0.7 ms each) read 12 % slower than 300, of the ResNet set 1 %.
DEFAULT_STEPS = {"resnet50": (100, 20), "alexnet": (300, 60), "googlenet": (150, 30), "lenet": (2000, 500)}
FP32_VECTOR_TFLOPS = 157.3   # MI355X_MICROARCH.md: peak FP32 (vector) = peak FP32 (matrix)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def workload_layers(synth, name, batch, sparsity):
    if name == "resnet50":
        return synth.resnet50_3x3(N=batch or 256, sparsity=0.9 if sparsity is None else sparsity), \
            "ResNet-50 16x 3x3 branch2b conv layers"
    if name == "alexnet":
        return synth.alexnet(N=batch or 128, sparsity=0.8 if sparsity is None else sparsity), \
            "AlexNet conv2-conv5"
    if name == "googlenet":
        return synth.googlenet_1x1(N=batch or 256, sparsity=0.95 if sparsity is None else sparsity), \
            "GoogLeNet-v1 1x1 convs"
    if name == "lenet":
        return synth.lenet_conv2(N=batch or 64, sparsity=0.5 if sparsity is None else sparsity), \
            "LeNet-5 conv2"
    raise SystemExit("unknown workload %s" % name)


# ---------------------------------------------------------------------------------------------
# The device side behind a small interface, so that the sharding / broadcast / checking code
# below is the same code in the 2-rank gloo test (tests/test_bench_gloo.py), where the forward
# is a stub around the CPU oracle, and on the GPU box.
# ---------------------------------------------------------------------------------------------

class HipBackend(object):
    name = "hip"
    dist_backend = "nccl"

    def __init__(self, pkg, local_rank, kernel, stream_stores=False, code_loader=0):
        import torch
        self.torch, self.pkg, self.kernel, self.stream_stores = torch, pkg, kernel, stream_stores
        self.code_loader = code_loader
        if not torch.cuda.is_available() or pkg.device_count() < 1:
            raise SystemExit("bench.py needs a HIP device: the product path has no CPU fallback")
        # (one rank per GPU under the driver; ranks wrap around when a rehearsal runs more ranks than
        # the box has GPUs, e.g. two gloo ranks on one device)
        dev_index = local_rank % max(1, torch.cuda.device_count())
        torch.cuda.set_device(dev_index)
        self.device = torch.device("cuda", dev_index)

    def make_plan(self, shape):
        opts = {"stream_stores": 1} if self.stream_stores else {}
        if self.code_loader:
            opts["code_loader"] = int(self.code_loader)
        return self.pkg.Plan(self.pkg.ConvDesc.from_shape(shape), kernel=self.kernel, **opts)

    def synchronize(self):
        self.torch.cuda.synchronize()

    def event(self):
        return self.torch.cuda.Event(enable_timing=True)


def image_seed(shape_index, global_index):
    """Seed of image `global_index` of the batch of distinct shape `shape_index`: a function of the
    GLOBAL image index, so results do not depend on how many ranks share the batch."""
    return 977 * (shape_index + 1) + 7919 * 65536 + global_index * 104729


def device_images(be, shape, shape_index, g0, n):
    """Images [g0, g0 + n) of the global batch, uniform(-1, 1), generated on the device."""
    torch = be.torch
    x = torch.empty((n, shape.C, shape.H, shape.W), device=be.device, dtype=torch.float32)
    gen = torch.Generator(device=be.device)
    if os.environ.get("ESCOIN_BENCH_BULK_INPUTS") == "1":
        # rocprofv3 --pmc runs only (tools/profile.sh): one generator call per layer instead of
        # four dispatches per image -- the counter-collection tool segfaults inside the ~40 000
        # instrumented dispatches the GoogLeNet set's inputs otherwise take.  The values differ
        # from the per-image seeding (cross-rank identity is not checked in those runs); the
        # kernels under measurement see the same shapes and the same distribution.
        gen.manual_seed(image_seed(shape_index, g0))
        return torch.rand((n, shape.C, shape.H, shape.W), device=be.device, generator=gen) * 2 - 1
    for i in range(n):
        gen.manual_seed(image_seed(shape_index, g0 + i))
        x[i] = torch.rand((shape.C, shape.H, shape.W), device=be.device, generator=gen) * 2 - 1
    return x


# how the nonzeros of the synthetic weights lie (--sparsity-dist; synth.SPARSITY_DISTS): "uniform" = every BASELINE config
WEIGHT_DIST = "uniform"


def layer_weight_seed(lid):
    return 1000 + 31 * lid


def build_layers(be, pkg, synth, shapes, rank, world, args=None, dist_on=None):
    with _unpinned():      # (WeightAlign's and the import's helper threads: see _unpinned)
        return _build_layers(be, pkg, synth, shapes, rank, world, args, dist_on)


def _build_layers(be, pkg, synth, shapes, rank, world, args=None, dist_on=None):
    """WeightAlign on rank 0, broadcast of the CSR (RCCL on the GPU box), set_csr elsewhere.
    Returns [(shape, plan, bias, shape_index, layer_id)] and the one-time costs: seconds in the
    broadcast, per-layer WeightAlign milliseconds (rank 0: dense -> CSR -> tiling, channel deal,
    generated code, code object), per-layer set_csr milliseconds on a receiver (the same minus
    dense -> CSR), generated-code bytes."""
    torch = be.torch
    layers, t_bcast, lid = [], 0.0, 0
    setup = {"align_ms": [], "receive_ms": [], "code_bytes": 0, "device_bytes": 0, "first_load_ms": None}
    if dist_on is None:
        dist_on = world > 1
    # --force-dist on ONE rank: the process group, the broadcast and the receiver's import all run (rank 0 is its own
    # receiver: it imports the blob it broadcast into a second plan, and THAT plan is the one the step times)
    loopback = dist_on and world == 1
    if rank == 0 and hasattr(pkg, "Plan") and not test_be(be) and getattr(args, "full", True):
        # The process's first WeightAlign of a generated-code plan also assembles the code object template (once per
        # process, jit_module.cpp) and loads the process's first HIP module: ~90-120 ms that belong to the process,
        # not to a layer.  A throw-away plan of the first layer's shape pays them here, timed on its own line.
        s0 = shapes[0]
        t0 = time.perf_counter()
        warm = be.make_plan(s0)
        warm.weight_align(synth.pruned_weights(s0, layer_weight_seed(0), WEIGHT_DIST))
        be.synchronize()
        t_first = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        again = be.make_plan(s0)
        again.weight_align(synth.pruned_weights(s0, layer_weight_seed(0), WEIGHT_DIST))
        be.synchronize()
        t_again = (time.perf_counter() - t0) * 1e3
        warm.close()
        again.close()
        setup["first_load_ms"] = max(0.0, t_first - t_again)
    # ---- phase 1: every layer gets a plan; rank 0 aligns it from the dense weights --------------------------------
    entries = []                       # [shape, plan, shape index, layer id]
    for si, s in enumerate(shapes):
        for rep in range(s.count):
            plan = be.make_plan(s)
            if rank == 0:
                w = synth.pruned_weights(s, layer_weight_seed(lid), WEIGHT_DIST)
                t0 = time.perf_counter()
                plan.weight_align(w)
                be.synchronize()
                setup["align_ms"].append((time.perf_counter() - t0) * 1e3)
            entries.append([s, plan, si, lid])
            lid += 1
    # ---- phase 2: the broadcast, layer by layer (one message per layer, like NCCL<Dtype>::Broadcast per blob,
    # parallel.cpp:189-200).  What travels: the ALIGNED form (CSR + channel deal + unit table + code object, one blob:
    # escoin_plan_export_aligned) where the plan has one -- a receiver then loads the code rank 0 generated
    # (import_aligned) instead of generating its own from the CSR (set_csr: 5-125 ms per layer) --, the CSR alone
    # otherwise (--broadcast csr, or a backend without code).  The blob stays on the device the collective filled.
    received = []
    aligned = getattr(args, "broadcast", "aligned") == "aligned" and hasattr(entries[0][1], "export_aligned")
    if dist_on:
        for s, plan, si, lid_ in entries:
            mg = s.M // s.group
            be.synchronize()
            t0 = time.perf_counter()
            if aligned:
                got = pkg.shard.broadcast_blob(plan.export_aligned() if rank == 0 else None, src=0, device=be.device,
                                               keep_on_device=not test_be(be))
            else:
                csr = plan.get_csr() if rank == 0 else None
                got = pkg.shard.broadcast_csr(csr, s.group, s.group * (mg + 1), synth.nnz_of(s), src=0, device=be.device)
            be.synchronize()
            t_bcast += time.perf_counter() - t0
            received.append(got)
    # ---- phase 3: the receivers build their plans from what arrived -- on a few host threads: the C ABI is
    # thread-compatible (one plan per thread at a time) and the code object loads of different plans overlap
    # (tools/dbg/import_threads.py: three 11 MB imports side by side take as long as 1.2 of them)
    if dist_on and (rank != 0 or loopback):
        if loopback:
            for e in entries:
                e[1].close()
                e[1] = be.make_plan(e[0])
        per_layer = [0.0] * len(entries)
        fast = [0] * len(entries)

        def receive(k):
            t1 = time.perf_counter()
            if aligned:
                fast[k] = int(entries[k][1].import_aligned(received[k]))
            else:
                entries[k][1].set_csr(*received[k])
            per_layer[k] = (time.perf_counter() - t1) * 1e3
        n_workers = max(1, min(int(getattr(args, "receive_threads", 1) or 1), len(entries)))
        be.synchronize()
        t0 = time.perf_counter()
        if n_workers > 1 and not test_be(be):
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(max_workers=n_workers) as ex:
                list(ex.map(receive, range(len(entries))))
        else:
            for k in range(len(entries)):
                receive(k)
        be.synchronize()
        setup["receive_wall_ms"] = (time.perf_counter() - t0) * 1e3
        setup["receive_threads"] = n_workers
        setup["receive_ms"] = per_layer
        if aligned:
            setup["import_fast"] = sum(fast)
    del received
    for s, plan, si, lid_ in entries:
        if hasattr(plan, "stat"):
            setup["code_bytes"] += plan.stat("code_bytes")
            setup["device_bytes"] += plan.stat("device_bytes")
            # balance of the channel deal: barrier-weighted slowest / mean wave, and the worst block (x 1000; 0 for
            # a plan restored from a persisted code object)
            try:
                setup.setdefault("deal", []).append((s.name, plan.stat("deal_slowest_over_mean_x1000"), plan.stat("deal_worst_block_x1000"),
                                                     plan.stat("code_bytes")))
            except Exception:       # (an older build of the library under ESCOIN_LIB: tools/ab.sh)
                pass
        bias = synth.bias_vector(s, 2000 + 31 * lid_)
        bias = torch.from_numpy(bias).to(be.device) if bias is not None else None
        layers.append((s, plan, bias, si, lid_))
    return layers, t_bcast, setup


def _group_deal(deal):
    out = {}
    for name, a, b, c in deal:
        out.setdefault(name, []).append((a, b, c))
    return list(out.items())


def last_layer_of_shape(layers):
    """{shape index: index (in `layers`) of the last layer of that shape}"""
    last = {}
    for li, entry in enumerate(layers):
        last[entry[3]] = li
    return last


def parity_check(be, oracle, synth, layers, bottoms, tops, images_per_shape=3):
    """After the timed region: tops[li] holds the output of layer li; the LAST layer of every shape is checked.  Images
    {0, N/2, N-1} of this rank's shard are recomputed by the CPU oracle from the same inputs and
    weights (regenerated from their seeds) -- the checker, never the thing measured."""
    torch = be.torch
    worst = 0.0
    for si, li in sorted(last_layer_of_shape(layers).items()):
        s, plan, bias, _, lid = layers[li]
        n = bottoms[li].shape[0]
        imgs = sorted(set([0, n // 2, n - 1]))[:images_per_shape]
        idx = torch.tensor(imgs, device=be.device)
        x = bottoms[li][idx].cpu().numpy()
        got = tops[li][idx].cpu().numpy()
        g = oracle.geom(s.C, s.H, s.W, s.M, s.KH, s.KW, s.pad_h, s.pad_w, s.stride_h, s.stride_w,
                        s.dil_h, s.dil_w, s.group)
        w = synth.pruned_weights(s, layer_weight_seed(lid), WEIGHT_DIST)
        b = synth.bias_vector(s, 2000 + 31 * lid)
        want = oracle.conv_forward(g, x, w, b, gate=False, threads=min(8, len(imgs)))
        err = float(np.abs(got.astype(np.float64) - want).max() / max(1e-6, float(np.abs(want).max())))
        worst = max(worst, err)
    return worst


def cross_rank_check(be, dist, synth, layers, shapes, tops, rank, world, g0_of_rank, n_of_rank):
    """Per-image checksums of every rank's outputs are gathered; rank 0 recomputes the first and
    last image of every OTHER rank's shard (same global-index seeds, its own plans) and compares.
    Returns the worst relative checksum difference (None for world == 1)."""
    if dist is None:
        return None
    torch = be.torch
    worst = 0.0
    n_max = max(n_of_rank)
    for si, li in sorted(last_layer_of_shape(layers).items()):
        s, plan, bias, _, lid = layers[li]
        sums = torch.zeros(n_max, device=be.device, dtype=torch.float64)
        sums[:tops[li].shape[0]] = tops[li].double().sum(dim=(1, 2, 3))
        gathered = [torch.zeros_like(sums) for _ in range(world)]
        dist.all_gather(gathered, sums)
        if rank != 0:
            continue
        for r in range(1, world):
            if n_of_rank[r] < 1:
                continue
            for local in sorted(set([0, n_of_rank[r] - 1])):
                x = device_images(be, s, si, g0_of_rank[r] + local, 1)
                y = plan.forward(x, bias)
                be.synchronize()
                mine = float(y.double().sum())
                theirs = float(gathered[r][local])
                scale = max(1e-6, float(y.double().abs().sum()))
                worst = max(worst, abs(mine - theirs) / scale)
    t = torch.tensor([worst], device=be.device, dtype=torch.float64)
    dist.broadcast(t, src=0)
    return float(t.item())


# ---------------------------------------------------------------------------------------------
# CPU baseline
# ---------------------------------------------------------------------------------------------

def host_cpu_info():
    """Threads this process may use (affinity mask and cgroup quota), physical cores among them,
    CPU model."""
    try:
        allowed = sorted(os.sched_getaffinity(0))
    except AttributeError:
        allowed = list(range(os.cpu_count() or 1))
    quota = None
    try:
        q, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = max(1, int(float(q) / float(period)))
    except Exception:
        pass
    model, cores = "unknown", set()
    try:
        phys = core = proc = None
        for line in open("/proc/cpuinfo"):
            if line.startswith("processor"):
                proc = int(line.split(":")[1])
            elif line.startswith("model name") and model == "unknown":
                model = line.split(":", 1)[1].strip()
            elif line.startswith("physical id"):
                phys = int(line.split(":")[1])
            elif line.startswith("core id"):
                core = int(line.split(":")[1])
            elif not line.strip():
                if proc in allowed and phys is not None and core is not None:
                    cores.add((phys, core))
                phys = core = proc = None
    except Exception:
        pass
    hw_threads = len(allowed) if quota is None else min(len(allowed), quota)
    physical = min(hw_threads, len(cores)) if cores else hw_threads
    return {"hw_threads": hw_threads, "physical_cores": max(1, physical), "model": model,
            "cgroup_quota": quota}


_HOST_INFO = None
_ALLOWED_CPUS = None      # the affinity mask the process started with (main(), before any OpenMP runtime pinned this thread)


class _unpinned(object):
    """Gives this thread the affinity mask the process started with for the duration of a `with` block.
    bench.py exports OMP_PROC_BIND=close for its reference CPU legs, and the OpenMP runtime torch loads binds the
    INITIAL thread to one core when it loads; every thread the product library starts from this thread -- WeightAlign's
    helpers (channel deal, code generation), the CPU mode's pool -- inherits that one-core mask.  That is this harness's
    doing, not the deployment's: a Caffe process does not pin its main thread.  Without the block WeightAlign of a res5
    layer measured 30 ms here against 17 ms in a plain process (profiles/r06_code_memory.md)."""

    def __enter__(self):
        self.pinned = None
        if _ALLOWED_CPUS:
            try:
                self.pinned = os.sched_getaffinity(0)
                os.sched_setaffinity(0, _ALLOWED_CPUS)
            except (AttributeError, OSError):
                self.pinned = None
        return self

    def __exit__(self, *exc):
        if self.pinned:
            try:
                os.sched_setaffinity(0, self.pinned)
            except OSError:
                pass
        return False


def product_cpu_mode(pkg, synth, shapes, threads, budget_s):
    """The PRODUCT's own Caffe::CPU mode (escoin_forward_cpu, csrc/sconv_cpu*.cpp -- not the oracle, not oracle/_ref)
    on the same shapes and host cores, reported beside the reference CPU numbers: images/s over the whole layer set."""
    per_image, share = 0.0, budget_s / max(1, len(shapes))
    # The library's host threads inherit the affinity of the thread that starts them -- and this thread was pinned to ONE
    # core by the OpenMP runtime (OMP_PROC_BIND=close for the reference legs binds the initial thread when libgomp loads).
    # For this leg it gets back the mask the process started with (main() recorded it before anything loaded OpenMP);
    # without that 16 pool threads shared one core (first r06 run: 230 images/s).  Inside the mask the pool spreads itself
    # (sconv_cpu.cpp, place_on_own_core): no warm-up second is needed for the scheduler to find the other cores.
    with _unpinned():
        return _product_cpu_mode(pkg, synth, shapes, threads, per_image, share)


def _product_cpu_mode(pkg, synth, shapes, threads, per_image, share):
    for k, s in enumerate(shapes):
        plan = pkg.Plan(pkg.ConvDesc.from_shape(s))
        plan.weight_align_cpu(synth.pruned_weights(s, 1000 + k, WEIGHT_DIST))
        b = synth.bias_vector(s, 2000 + k)
        n = min(256, max(16 * threads, 64))      # (whole-batch calls like the reference legs: 16 images per thread)
        x = synth.activations(s, 3000 + k, 0, n)
        top = np.zeros((n, s.M) + tuple(plan.out_hw), np.float32)   # the top blob exists before Forward (Reshape), as in Caffe
        t0 = time.perf_counter()                                  # warm: threads, page faults, padded buffers
        while time.perf_counter() - t0 < (0.5 if k == 0 else 0.2):
            plan.forward_cpu(x, b, n_threads=threads, out=top)
        t0 = time.perf_counter()
        plan.forward_cpu(x, b, n_threads=threads, out=top)
        t1 = time.perf_counter() - t0
        reps = int(max(1, min(50, share / max(t1, 1e-4))))
        t0 = time.perf_counter()
        for _ in range(reps):
            plan.forward_cpu(x, b, n_threads=threads, out=top)
        t1 = (time.perf_counter() - t0) / reps
        per_image += s.count * t1 / n
        log("  cpu %-16s product  %4d threads %6d img in %.4f s -> %.1f img/s/layer" % (s.name, threads, n, t1, n / t1))
        plan.close()
    return {"value": round(1.0 / per_image, 3), "unit": "images/s", "cores": threads, "kernel": pkg.cpu_kernel_name(),
            "what": "escoin_forward_cpu: the product library's Caffe::CPU mode (bit-equal to the reference loop nest), "
                    "timed like the reference legs; NOT the cpu_baseline -- shown beside it"}


def cpu_baseline(oracle, synth, shapes, budget_s):
    """Reference CPU sconv path timed on this box's host cores on a bounded sample.

    kind "reference": oracle/_ref = the reference's own kernels compiled in place.  The layer is
    aligned ONCE per shape (RefPlan: dense -> CSR outside the timed call, as WeightAlign does) and
    the whole-batch forward is timed for thread counts {1, physical cores, all hardware threads}
    (OMP_PROC_BIND=close, OMP_PLACES=cores), OpenMP over the batch the way the reference's ICC
    build parallelises (conv_layer.cpp:41-43; with batch >= threads / 2 its thread grouping,
    cpu_info.cpp:483-605, degenerates to exactly that).  `value` = the best thread count with the
    reference's default loop nest (caffe_cpu_sconv, math_functions.cpp:128-176 -- what `caffe test
    -conv_mode 2` runs under g++); `best_effort` = the same with the register-blocked kernel
    sconv_unit_stride (sconv.hpp:57-589, its ICC-only fast path) where the reference's switchboard
    has an instantiation.  kind "port": the C restatement when oracle/_ref is absent."""
    info = _HOST_INFO or host_cpu_info()
    use_ref = oracle.have_ref() and oracle.have_ref_plan()
    sweep = sorted(set([1, info["physical_cores"], info["hw_threads"]]))
    share = budget_s / max(1, len(shapes)) / (2 * len(sweep))
    per_image = {("default", t): 0.0 for t in sweep}
    per_image.update({("blocked", t): 0.0 for t in sweep})
    blocked_ok = use_ref
    sample = []
    for k, s in enumerate(shapes):
        g = oracle.geom(s.C, s.H, s.W, s.M, s.KH, s.KW, s.pad_h, s.pad_w, s.stride_h, s.stride_w,
                        s.dil_h, s.dil_w, s.group)
        w = synth.pruned_weights(s, 1000 + k, WEIGHT_DIST)
        b = synth.bias_vector(s, 2000 + k)
        plan = oracle.RefPlan(g, w) if use_ref else None
        blocked_ok = blocked_ok and plan is not None and plan.has_blocked
        kinds = ["default"] + (["blocked"] if plan is not None and plan.has_blocked else [])
        n_max = 0
        for kind in kinds:
            for t in sweep:
                if plan is not None:
                    run = lambda x, top, t=t, kind=kind: plan.forward(x, b, threads=t, kernel=kind, top=top)
                else:
                    run = lambda x, top, t=t: oracle.conv_forward(g, x, w, b, threads=t, gate=False)
                n = max(t, 2)
                x = synth.activations(s, 3000 + k, 0, n)
                top = np.zeros((n, s.M) + synth.out_hw(s), np.float32)
                run(x, top)                              # warm: threads, page faults
                t0 = time.perf_counter()
                run(x, top)
                t1 = time.perf_counter() - t0
                reps = int(max(1, min(16, share / max(t1, 1e-4))))
                if reps > 1:
                    n = n * reps
                    x = synth.activations(s, 3000 + k, 0, n)
                    top = np.zeros((n, s.M) + synth.out_hw(s), np.float32)
                    run(x, top)
                    t0 = time.perf_counter()
                    run(x, top)
                    t1 = time.perf_counter() - t0
                per_image[(kind, t)] += s.count * t1 / n
                n_max = max(n_max, n)
                log("  cpu %-16s %-8s %4d threads %6d img in %.3f s -> %.1f img/s/layer" %
                    (s.name, kind, t, n, t1, n / t1))
        sample.append("%s:<=%dimg" % (s.name, n_max))
        if plan is not None:
            plan.close()
    rate = lambda kind: {t: 1.0 / per_image[(kind, t)] for t in sweep if per_image[(kind, t)] > 0}
    d = rate("default")
    best_t = max(d, key=d.get)
    out = {"value": round(d[best_t], 3), "unit": "images/s", "cores": best_t,
           "kind": "reference" if use_ref else "port",
           "cpu_model": info["model"], "physical_cores": info["physical_cores"],
           "hw_threads": info["hw_threads"],
           "thread_sweep": {str(t): round(v, 3) for t, v in sorted(d.items())},
           "single_thread_value": round(d[1], 3),
           "sample": "whole-batch forward of " + ", ".join(sample) + " per distinct layer shape "
                     "and thread count, layer aligned once outside the timed call, OpenMP over "
                     "images; per-image time summed over all %d layers" % sum(s.count for s in shapes)}
    if blocked_ok:
        bl = rate("blocked")
        bt = max(bl, key=bl.get)
        out["best_effort"] = {"value": round(bl[bt], 3), "unit": "images/s", "cores": bt,
                              "kernel": "sconv_unit_stride (sconv.hpp:57-589, -DUSE_ICC under g++ -mavx2)",
                              "thread_sweep": {str(t): round(v, 3) for t, v in sorted(bl.items())}}
    return out


WORKLOAD_DEFAULTS = {"resnet50": (256, 90), "alexnet": (128, 80), "googlenet": (256, 95), "lenet": (64, 50)}


def _traffic_blob(workload, batch, sparsity_pct):
    """The committed PMC summary profiles/traffic_<workload>.json IF it was collected on this very configuration:
    same workload, same per-GPU batch, same weight sparsity.  The file carries `_batch` / `_sparsity_pct`
    (tools/save_profile.py writes them from the bench line of the profiled run); a file from before round 6 has
    neither and was collected on the workload's default configuration (WORKLOAD_DEFAULTS).  Anything else -- a
    --global-batch 2048 line, a sparsity sweep point -- has NO matching entry and gets None: a ratio of one
    configuration's traffic over another's algorithmic bytes is not a measurement (0.211)."""
    path = os.path.join(ROOT, "profiles", "traffic_%s.json" % workload)
    try:
        blob = json.load(open(path))
    except Exception:
        return None, path
    dflt = WORKLOAD_DEFAULTS.get(workload, (None, None))
    have_batch = blob.get("_batch", dflt[0])
    have_sp = blob.get("_sparsity_pct", dflt[1])
    if have_batch is None or have_sp is None or int(have_batch) != int(batch) or int(round(have_sp)) != int(round(sparsity_pct)):
        return None, path
    return blob, path


def traffic_per_layer(workload, batch=None, sparsity_pct=None):
    """{layer name: HBM bytes per launch} from the committed PMC summary of THIS configuration (tools/save_profile.py
    breaks the counters down by dispatch order), or {}."""
    dflt = WORKLOAD_DEFAULTS.get(workload, (None, None))
    blob, _ = _traffic_blob(workload, dflt[0] if batch is None else batch, dflt[1] if sparsity_pct is None else sparsity_pct)
    if not blob:
        return {}
    try:
        return {k: v["hbm_bytes_per_launch"] for k, v in blob.get("_per_layer", {}).items()}
    except Exception:
        return {}


def traffic_with_provenance(workload, kernel_name, batch=None, sparsity_pct=None):
    """HBM bytes per launch of the dominant kernel from the committed PMC summary (FETCH_SIZE x 2
    + WRITE_SIZE, MI355X_MICROARCH.md); collected in a separate rocprofv3 --pmc run
    (tools/profile.sh), so it comes with the file and the commit that file was last written in.
    (None, None) when the file was collected on another batch or sparsity."""
    dflt = WORKLOAD_DEFAULTS.get(workload, (None, None))
    batch = dflt[0] if batch is None else batch
    sparsity_pct = dflt[1] if sparsity_pct is None else sparsity_pct
    blob, path = _traffic_blob(workload, batch, sparsity_pct)
    if not blob:
        return None, None
    value = blob.get(kernel_name)
    if value is None:
        return None, None
    commit = blob.get("_commit")
    how = "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes, 2 x FETCH + WRITE"
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "log", "-1", "--format=%h", "--", path],
                                    stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                                    timeout=10).stdout.decode().strip() or None
        except Exception:
            pass
    return value, {"file": os.path.relpath(path, ROOT), "commit": commit, "saved": blob.get("_saved"),
                   "batch": int(batch), "sparsity_pct": int(round(sparsity_pct)), "how": how}


def measure_config(be, pkg, synth, oracle, workload, sparsity, cache, target_ms=150.0, settle_ms=100.0):
    """One more single-GPU configuration, timed AFTER (never inside) the headline region: the same step (every layer of
    the workload, own bottom / top pair per layer, one stream), the same event accounting and the same parity check
    against the oracle.  Returns a compact sub-record for `other_configs` / `sparsity_sweep`.
      ms_per_step   K steps between two HIP events on the launch stream, K chosen for ~target_ms of device time
      frac          the step's algorithmic bytes / ms_per_step / 8 TB/s  (HBM roofline fraction of the whole step)
      binding_frac  sum over layers of max(bytes / 8 TB/s, flops / 157.3 TF) / ms_per_step
      per_layer     from one extra step with an event between every two launches (after the timed steps)"""
    torch = be.torch
    shapes, wl_name = workload_layers(synth, workload, None, sparsity)
    batch = shapes[0].N
    layers, _, setup = build_layers(be, pkg, synth, shapes, 0, 1, None, False)
    key = (workload, batch)
    if key not in cache:                 # the synthetic batch does not depend on the sparsity: one per workload
        cache.clear()                    # (one workload's inputs at a time: the sweep runs workload by workload)
        cache[key] = [device_images(be, s, si, 0, batch) for si, s in enumerate(shapes)]
    shape_bottoms = cache[key]
    bottoms, tops, used = [], [], set()
    for (s, plan, bias, si, lid) in layers:
        bottoms.append(shape_bottoms[si] if si not in used else shape_bottoms[si].clone())
        used.add(si)
        tops.append(torch.empty((batch, s.M) + tuple(synth.out_hw(s)), device=be.device))

    def step(events=None):
        for li, (s, plan, bias, si, lid) in enumerate(layers):
            plan.forward(bottoms[li], bias, tops[li])
            if events is not None:
                events[li + 1].record()

    def timed(k):
        e0, e1 = be.event(), be.event()
        e0.record()
        for _ in range(k):
            step()
        e1.record()
        be.synchronize()
        return e0.elapsed_time(e1) / k
    be.synchronize()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < settle_ms:
        step()
        be.synchronize()
    est = timed(3)
    k = int(min(400, max(10, target_ms / max(est, 1e-3))))
    runs = sorted(timed(k) for _ in range(3))
    ms = runs[1]                                                   # median of three regions of k steps
    ev = [be.event() for _ in range(len(layers) + 1)]
    ev[0].record()
    step(ev)
    be.synchronize()
    layer_ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(len(layers))]
    scale = ms / max(1e-9, sum(layer_ms))                          # (events between launches cost time: normalised to the plain step)
    parity = parity_check(be, oracle, synth, layers, bottoms, tops)
    per_kernel, per_shape = {}, {}
    for li, (s, plan, bias, si, lid) in enumerate(layers):
        per_kernel[plan.kernel_name] = per_kernel.get(plan.kernel_name, 0.0) + layer_ms[li]
        per_shape.setdefault(si, []).append(layer_ms[li] * scale)
    dom = max(per_kernel.items(), key=lambda kv: kv[1])
    byt = sum(synth.algorithmic_bytes(s, batch) * s.count for s in shapes)
    flo = sum(synth.flops(s, batch) * s.count for s in shapes)
    t_bind = sum(max(synth.algorithmic_bytes(s, batch) / (HBM_PEAK_GBS * 1e9),
                     synth.flops(s, batch) / (FP32_VECTOR_TFLOPS * 1e12)) * s.count for s in shapes)
    per_layer = []
    for si, s in enumerate(shapes):
        m = float(np.mean(per_shape[si]))
        b1, f1 = synth.algorithmic_bytes(s, batch), synth.flops(s, batch)
        per_layer.append({"layer": s.name, "count": s.count, "us": round(m * 1e3, 1),
                          "hbm_frac": round(b1 / (HBM_PEAK_GBS * 1e9) / (m * 1e-3), 4),
                          "binding_frac": round(max(b1 / (HBM_PEAK_GBS * 1e9), f1 / (FP32_VECTOR_TFLOPS * 1e12)) / (m * 1e-3), 4)})
    rec = {"workload": workload,
           "config": "%s @%d%% sparsity, batch %d, fp32" % (wl_name, round(100 * shapes[0].sparsity), batch),
           "sparsity_pct": int(round(100 * shapes[0].sparsity)), "batch": batch,
           "ms_per_step": round(ms, 4), "ms_per_step_regions": [round(v, 4) for v in runs], "steps": k,
           "images_per_s": round(batch / (ms * 1e-3), 1),
           "frac": round(byt / (HBM_PEAK_GBS * 1e9) / (ms * 1e-3), 4),
           "binding_frac": round(t_bind / (ms * 1e-3), 4),
           "alg_GBps": round(byt / (ms * 1e-3) / 1e9, 1), "sparse_TFLOPs": round(flo / (ms * 1e-3) / 1e12, 2),
           "parity_max_rel_err": float("%.3g" % parity),
           "dominant_kernel": dom[0], "dominant_kernel_share": round(dom[1] / max(1e-9, sum(layer_ms)), 3),
           "layers_per_step": len(layers), "weight_align_ms": round(sum(setup["align_ms"]), 1),
           "per_layer": per_layer}
    if parity > 1e-4:
        rec["parity_failed"] = True
    for (s, plan, bias, si, lid) in layers:
        plan.close()
    del bottoms, tops
    return rec


def measure_extras(be, pkg, synth, oracle, budget_s):
    """every 1-GPU config of BASELINE.json and north_star's 60-95 % sweep in the driver-run line.
    other_configs: AlexNet conv2-5 @80 % N=128 (configs[1]), GoogLeNet 1x1 @95 % N=256 (configs[4]), LeNet conv2
    (configs[0]'s layer on the GPU).  sparsity_sweep: the ResNet-50 and AlexNet sets at 60 / 70 / 80 / 95 % (ResNet @90 %
    is the headline itself, AlexNet @80 % is other_configs.alexnet -- both are repeated in the sweep table by reference).
    Stops starting new configurations when the budget is spent (what was skipped is listed)."""
    t0 = time.perf_counter()
    cache, other, sweep, skipped = {}, {}, [], []
    plan_list = [("alexnet", None, other), ("alexnet", 0.6, sweep), ("alexnet", 0.7, sweep), ("alexnet", 0.95, sweep),
                 ("lenet", None, other),
                 ("googlenet", None, other),
                 ("resnet50", 0.6, sweep), ("resnet50", 0.7, sweep), ("resnet50", 0.8, sweep), ("resnet50", 0.95, sweep)]
    for workload, sparsity, dest in plan_list:
        if time.perf_counter() - t0 > budget_s:
            skipped.append("%s@%s" % (workload, "default" if sparsity is None else int(sparsity * 100)))
            continue
        t1 = time.perf_counter()
        rec = measure_config(be, pkg, synth, oracle, workload, sparsity, cache)
        rec["wall_s"] = round(time.perf_counter() - t1, 2)
        log("  extra %-10s @%2d%%  %8.4f ms/step  %10.1f img/s  frac %.3f  binding %.3f  parity %.2g  (%s, %.1f s)" %
            (workload, rec["sparsity_pct"], rec["ms_per_step"], rec["images_per_s"], rec["frac"], rec["binding_frac"],
             rec["parity_max_rel_err"], rec["dominant_kernel"], rec["wall_s"]))
        if dest is other:
            other[workload] = rec
        else:
            sweep.append(rec)
    cache.clear()
    return other, sweep, skipped, round(time.perf_counter() - t0, 1)


DUMP_BUDGET_BYTES = 48 << 20      # --dump-outputs: all files together, headers aside (the option promises <= 64 MB)


def dump_outputs(be, layers, tops, out_dir):
    """--dump-outputs: what a caller of the timed path receives -- the top blob of every layer after the last timed
    step -- as <out_dir>/top<layer id>_<layer name>.npy, float32.  A blob larger than its share of DUMP_BUDGET_BYTES is
    written as a fixed sample: that many flat indices drawn without replacement by a generator seeded with the layer
    id, in ascending order -- the same elements in every run with the same arguments.  Returns the file names."""
    torch = be.torch
    os.makedirs(out_dir, exist_ok=True)
    share = DUMP_BUDGET_BYTES // 4 // max(1, len(layers))
    names = []
    for li, (s, plan, bias, si, lid) in enumerate(layers):
        top = tops[li]
        if top.numel() > share:
            idx = np.sort(np.random.default_rng(4099 + lid).choice(top.numel(), share, replace=False))
            top = top.reshape(-1)[torch.from_numpy(idx).to(top.device)]
        name = "top%02d_%s.npy" % (lid, s.name)
        np.save(os.path.join(out_dir, name), top.float().cpu().numpy())
        names.append(name)
    return names


def test_be(be):
    return be.name != "hip"


def run(args, be, pkg, synth, oracle_loader, dist=None):
    torch = be.torch
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    strong = args.global_batch is not None
    if strong:
        spans = [pkg.shard.shard_range(args.global_batch, r, world) for r in range(world)]
        per_rank = [e - b for b, e in spans]
        g0_of_rank = [b for b, e in spans]
        batch = per_rank[rank]
        if min(per_rank) < 1:
            raise SystemExit("--global-batch %d leaves a rank without images" % args.global_batch)
        plan_batch = max(per_rank)
    else:
        batch = args.batch
        plan_batch = None
    shapes, wl_name = workload_layers(synth, args.workload, plan_batch if strong else batch, args.sparsity)
    per_gpu_batch = batch if strong else shapes[0].N
    if not strong:
        per_rank = [per_gpu_batch] * world
        g0_of_rank = [r * per_gpu_batch for r in range(world)]
    global_batch = sum(per_rank)

    dist_on = dist is not None          # world > 1, or one rank under --force-dist
    layers, t_bcast, setup = build_layers(be, pkg, synth, shapes, rank, world, args, dist_on)

    # ---- synthetic activations resident in HBM (image k seeded by its GLOBAL index) -----------
    # Every LAYER has its own bottom / top pair (layers of one shape get copies of the same
    # synthetic batch): consecutive launches of one shape must not find their input in the 256 MB
    # Infinity Cache because the previous launch read the same buffer (res4's six launches read
    # 51 MB each).  A step touches 2.8 GB on the ResNet set, so every launch reads from HBM.
    shape_bottoms = []
    for si, s in enumerate(shapes):
        shape_bottoms.append(device_images(be, s, si, g0_of_rank[rank], per_gpu_batch))
    bottoms, tops, used = [], [], set()
    for (s, plan, bias, si, lid) in layers:
        bottoms.append(shape_bottoms[si] if si not in used else shape_bottoms[si].clone())
        used.add(si)
        oh, ow = synth.out_hw(s)
        tops.append(torch.empty((per_gpu_batch, s.M, oh, ow), device=be.device))
    be.synchronize()

    # --streams S > 1 (not the default; the reference runs everything on one stream): the step's layers are
    # independent (own bottom / top pairs, like the parallel 1x1 branches of an inception module) and go out round
    # robin on S HIP streams -- a layer's launch, start-up and drain then overlap its neighbours' streaming phase
    # (tools/two_streams.py; GoogLeNet set -9 %, ResNet / AlexNet +-0).  What a net-level scheduler could get out of
    # the layer-level drop-in; the per-launch accounting below needs launches that do not overlap and is skipped.
    n_streams = max(1, int(getattr(args, "streams", 1) or 1)) if not test_be(be) else 1
    side_streams = [torch.cuda.Stream(device=be.device) for _ in range(n_streams)] if n_streams > 1 else None

    def step(events=None):
        # (sampled steps only) one event between consecutive launches: the end of launch i is the start
        # of launch i + 1, so a launch's duration includes its dispatch gap, which the step pays for it
        if side_streams is not None:
            main = torch.cuda.current_stream(be.device)
            for st in side_streams:
                st.wait_stream(main)
            for li, (s, plan, bias, si, lid) in enumerate(layers):
                with torch.cuda.stream(side_streams[li % n_streams]):
                    plan.forward(bottoms[li], bias, tops[li])
            for st in side_streams:
                main.wait_stream(st)
            return
        for li, (s, plan, bias, si, lid) in enumerate(layers):
            plan.forward(bottoms[li], bias, tops[li])
            if events is not None:
                events[li + 1].record()

    # Order of the run: W warm-up steps, then (--full only) K steps timed COLD (`ms_per_step_cold`: what a caller gets who
    # does exactly what the command line says -- W untimed steps, K timed ones, nothing else), then the settle loop, then
    # the timed region(s) `value` is computed from.  The chip's clocks take tens of milliseconds of load to settle (the
    # first 100 launches of a layer run 10-15 % slower than the next hundred): with `--warmup 5` the cold region is over
    # before that.  The settle loop runs the same step untimed for a fixed wall-clock time, outside the W + K steps the
    # command asks for and declared in the JSON line (`settle_ms`); under --full both numbers are printed.
    full = bool(getattr(args, "full", True))
    for _ in range(args.warmup):
        step()
    cold_ms = None
    if full and not test_be(be):
        e0, e1 = be.event(), be.event()
        be.synchronize()
        e0.record()
        for _ in range(args.steps):
            step()
        e1.record()
        be.synchronize()
        cold_ms = e0.elapsed_time(e1) / args.steps
    if args.settle_ms > 0:
        be.synchronize()
        t_settle = time.perf_counter()
        while (time.perf_counter() - t_settle) * 1e3 < args.settle_ms:
            step()
            be.synchronize()
    # Events inside the timed region: ONE per step boundary in every step, and one between every two
    # launches in a SAMPLE of the steps (10 of the default 100, 2 of a run of 20).  An event
    # between two kernels is not free -- 1.5 us per launch on the ResNet set, 2.9 us on GoogLeNet's 39
    # short launches (8 % of that step, tools/gap_probe.py) -- and a caller of the path records none,
    # so most steps run as a caller's would.  What an event costs is measured here, as the difference
    # between the sampled and the other steps, and taken off the per-launch durations.
    n_sampled = min(10, max(2, args.steps // 10)) if args.steps >= 4 else 1
    stride = max(1, args.steps // n_sampled)
    sampled = [k for k in range(args.steps) if k % stride == 0][:n_sampled]
    if side_streams is not None or not full:
        sampled = []          # (overlapping launches have no per-launch duration; a plain run records no events)
    # R timed regions (--full: --repeats, SURVEY 8d: median of >= 5 repeats; a plain run: one), each EXACTLY K steps
    # bracketed by a barrier + device synchronisation on both sides and reduced with MAX over the ranks; `value` is
    # computed from the median region, under --full the line also carries the fastest and the slowest one.
    regions = []          # (elapsed seconds, step events, per-launch events of the sampled steps)
    for rep in range(max(1, args.repeats) if full else 1):
        step_ev = [be.event() for _ in range(args.steps + 1)] if full else None
        ev = {k: [step_ev[k]] + [be.event() for _ in range(len(layers))] for k in sampled}
        if dist_on:
            dist.barrier()
        be.synchronize()
        t0 = time.perf_counter()
        for k in range(args.steps):
            if step_ev is not None:
                step_ev[k].record()
            step(ev.get(k))
        if step_ev is not None:
            step_ev[args.steps].record()
        be.synchronize()
        elapsed = time.perf_counter() - t0
        if dist_on:
            dist.barrier()
            t = torch.tensor([elapsed], device=be.device, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        regions.append((elapsed, step_ev, ev))
    order = sorted(range(len(regions)), key=lambda i: regions[i][0])
    median_region = order[(len(order) - 1) // 2]     # (lower median for an even count: a region that was run)
    elapsed, step_ev, ev = regions[median_region]
    region_ms = [r[0] / args.steps * 1e3 for r in regions]

    # ---- what the last timed step computed, for a comparison of two builds output for output ----
    dumped = None
    if getattr(args, "dump_outputs", None) and rank == 0:
        dumped = dump_outputs(be, layers, tops, args.dump_outputs)
        log("bench.py: %d output files in %s" % (len(dumped), args.dump_outputs))

    # ---- self-check of what was just computed (--full; outside the timed region) -------------
    oracle, parity, cross = None, None, None
    if full:
        oracle = oracle_loader()
        parity = parity_check(be, oracle, synth, layers, bottoms, tops)
        if dist_on:
            t = torch.tensor([parity], device=be.device, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            parity = float(t.item())
        cross = cross_rank_check(be, dist, synth, layers, shapes, tops, rank, world, g0_of_rank, per_rank)
    receive = None
    if dist_on:
        # the slowest receiver's set_csr total and its slowest layer (rank 0 has none: it aligned -- unless it is its
        # own receiver, --force-dist on one rank)
        t = torch.tensor([setup.get("receive_wall_ms", 0.0), max(setup["receive_ms"] or [0.0]), -float(setup.get("import_fast", 0)) if (rank or world == 1) else -1e9,
                          sum(setup["receive_ms"])],
                         device=be.device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        # total = wall time of the slowest receiver from "every layer's message is here" to "every plan is ready"
        # (its layers are imported on `threads` host threads); sum_per_layer = the same work added up layer by layer
        receive = {"total": round(float(t[0].item()), 2), "max_per_layer": round(float(t[1].item()), 2),
                   "sum_per_layer": round(float(t[3].item()), 2), "threads": setup.get("receive_threads", 1),
                   "what": getattr(args, "broadcast", "aligned"),
                   # layers whose persisted code object every receiver loaded as it was (the fewest over the receivers)
                   "code_objects_loaded_as_sent": int(-t[2].item()) if t[2].item() > -1e8 else 0}
    if rank != 0:
        return None

    # ---- per-kernel accounting from the events recorded inside the timed region (--full) --------
    sparsity_pct = round(100 * shapes[0].sparsity)
    roofline = None
    if full:
        per_kernel, layer_ms = {}, []
        step_ms = [step_ev[k].elapsed_time(step_ev[k + 1]) for k in range(args.steps)]
        plain = [step_ms[k] for k in range(args.steps) if k not in ev]
        ms_plain = float(np.mean(plain)) if plain else float(np.mean(step_ms))
        ms_sampled = float(np.mean([step_ms[k] for k in sampled])) if sampled else ms_plain
        # what one event between two launches costs the launches of a sampled step: their durations, event to
        # event, add up to this much more than a step without them takes (so the corrected ones add up to it)
        ms_launches = float(np.mean([ev[k][0].elapsed_time(ev[k][len(layers)]) for k in sampled])) if sampled else ms_plain
        event_ms = max(0.0, (ms_launches - ms_plain) / len(layers)) if plain and sampled else 0.0
        # (several streams: launches overlap -- every launch is booked at its algorithmic-byte share of the step, which
        #  keeps the step's totals right and says nothing about single layers: per_layer is dropped below)
        total_alg = float(sum(synth.algorithmic_bytes(l[0], per_gpu_batch) for l in layers))
        layer_ms_raw = []
        for li, (s, plan, bias, si, lid) in enumerate(layers):
            ms = [ev[k][li].elapsed_time(ev[k][li + 1]) for k in sampled] if sampled else \
                 [ms_plain * synth.algorithmic_bytes(s, per_gpu_batch) / total_alg]
            layer_ms_raw.append(float(np.mean(ms)))
            m = max(float(np.mean(ms)) - event_ms, 1e-6)
            layer_ms.append(m)
            # the tiled kernel has a second instantiation for layers whose plane DMA can be issued from
            # inside the stream walk (escoin_sconv_tiled_dma_kernel<3, 1>): one kernel family, two rows
            # in a rocprofv3 summary -- "instantiations" below has each row's launches and average
            fam = plan.kernel_name.replace("_tiled_dma_kernel", "_tiled_kernel")
            d = per_kernel.setdefault(fam, {"ms": 0.0, "bytes": 0, "flops": 0, "launches": 0, "inst": {}})
            d["ms"] += m
            d["bytes"] += synth.algorithmic_bytes(s, per_gpu_batch)
            d["flops"] += synth.flops(s, per_gpu_batch)
            d["launches"] += 1
            i = d["inst"].setdefault(plan.kernel_name, {"ms": 0.0, "launches": 0})
            i["ms"] += m
            i["launches"] += 1
        per_layer, seen = [], {}
        layer_traffic = traffic_per_layer(args.workload, per_gpu_batch, sparsity_pct)
        seen_raw = {}
        for li, (s, plan, bias, si, lid) in enumerate(layers):
            seen.setdefault(si, []).append(layer_ms[li])
            seen_raw.setdefault(si, []).append(layer_ms_raw[li])
        for si, s in enumerate(shapes):
            m = float(np.mean(seen[si]))
            name = layers[last_layer_of_shape(layers)[si]][1].kernel_name
            byt, flo = synth.algorithmic_bytes(s, per_gpu_batch), synth.flops(s, per_gpu_batch)
            t_hbm, t_fma = byt / (HBM_PEAK_GBS * 1e9), flo / (FP32_VECTOR_TFLOPS * 1e12)
            per_layer.append({"layer": s.name, "count": s.count, "us": round(m * 1e3, 1),
                              # event to event, nothing taken off (one event between two launches costs `event_us`)
                              "us_raw": round(float(np.mean(seen_raw[si])) * 1e3, 1),
                              "alg_GBps": round(byt / m / 1e6, 1), "sparse_TFLOPs": round(flo / m / 1e9, 2),
                              "hbm_frac": round(t_hbm / (m * 1e-3), 4), "fma_frac": round(t_fma / (m * 1e-3), 4),
                              "binding_frac": round(max(t_hbm, t_fma) / (m * 1e-3), 4),
                              "alg_bytes": int(byt),
                              # PMC (separate run, profiles/traffic_<workload>.json): HBM bytes of this layer's launch
                              "hbm_traffic": layer_traffic.get(s.name),
                              "traffic_over_alg": round(layer_traffic[s.name] / byt, 3) if s.name in layer_traffic else None})
            log("  gpu %-16s %-44s %8.1f us  %7.1f GB/s alg  %6.2f TFLOP/s  binding %.3f  x%d" %
                (s.name, name, m * 1e3, byt / m / 1e6, flo / m / 1e9, per_layer[-1]["binding_frac"], s.count))
        dom_name, dom = max(per_kernel.items(), key=lambda kv: kv[1]["ms"])
        achieved = dom["bytes"] / (dom["ms"] * 1e-3) / 1e9
        # HBM traffic per launch: the instantiations' PMC figures weighted by their launches
        traffic, provenance, tw = None, None, 0
        for iname, iv in dom["inst"].items():
            tv, pv = traffic_with_provenance(args.workload, iname, per_gpu_batch, sparsity_pct)
            if tv is None:
                traffic = None
                break
            traffic = (traffic or 0) + tv * iv["launches"]
            tw += iv["launches"]
            provenance = pv
        if traffic is not None and tw:
            traffic = int(traffic / tw)
        t_bind = sum(max(synth.algorithmic_bytes(s, per_gpu_batch) / (HBM_PEAK_GBS * 1e9),
                         synth.flops(s, per_gpu_batch) / (FP32_VECTOR_TFLOPS * 1e12)) * s.count for s in shapes)
        # (one name per rocprofv3 row: the family's instantiations, most launches first)
        dom_label = " + ".join(sorted(dom["inst"], key=lambda k: -dom["inst"][k]["launches"]))
        roofline = {"bound": "hbm", "kernel": dom_label, "achieved": round(achieved, 1),
                    "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                    "traffic": traffic, "traffic_provenance": provenance,
                    # PMC bytes (FETCH_SIZE x 2 + WRITE_SIZE, the fabric side of the L2s: Infinity-Cache hits included) over
                    # the algorithmic bytes, per launch of the dominant kernel over the step: > 1 = re-reads (halo, several
                    # workgroup columns, XCD grouping) and generated code; profiles/r05_mall_share.md says which of it is HBM
                    "traffic_over_alg": round(traffic / (dom["bytes"] / dom["launches"]), 3) if traffic else None,
                    "avg_launch_us": round(dom["ms"] / dom["launches"] * 1e3, 2),
                    "launches_per_step": dom["launches"],
                    # per-launch events in `sampled_steps` of the timed steps; one event costs `event_us`
                    # (sampled minus other steps, per launch), already taken off every duration here
                    # (the corrected per-launch durations must add up to a step without events: a check of the
                    #  correction, not a tunable -- bench lines seen so far sit within 2 % of 1)
                    "launch_sum_over_step": round(sum(layer_ms) / max(1e-9, ms_plain), 4),
                    "events": {"sampled_steps": len(sampled), "of": args.steps, "event_us": round(event_ms * 1e3, 2),
                               "ms_per_step_sampled": round(ms_sampled, 4), "ms_per_step_other": round(ms_plain, 4)},
                    "instantiations": {k: {"launches_per_step": v["launches"],
                                           "avg_launch_us": round(v["ms"] / v["launches"] * 1e3, 2)}
                                       for k, v in dom["inst"].items()},
                    "algorithmic_bytes_per_launch": int(dom["bytes"] / dom["launches"]),
                    "sparse_tflops": round(dom["flops"] / (dom["ms"] * 1e-3) / 1e12, 2),
                    # max(bytes / 8 TB/s, flops / 157.3 TF) summed over the step / measured step time:
                    # the fraction of whichever roofline binds each layer
                    "binding_frac": round(t_bind / (sum(layer_ms) * 1e-3), 4),
                    "per_layer": per_layer if sampled else None,
                    "streams": n_streams}

    ms_per_step = elapsed / args.steps * 1e3
    value = global_batch / (ms_per_step * 1e-3)
    out = {
        "metric": "conv-layer fwd images/sec", "value": round(value, 1), "unit": "images/s",
        "n_gpus": world, "n_ranks_seen": dist.get_world_size() if dist is not None else 1,
        "steps": args.steps, "warmup": args.warmup, "settle_ms": args.settle_ms,
        "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "full": full,
        "scaling": "strong" if strong else "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "%s @%d%% sparsity, batch %d/GPU, fp32" %
                               (wl_name, round(100 * shapes[0].sparsity), per_gpu_batch),
                   "global_batch": global_batch, "per_gpu_batch": per_gpu_batch, "sparsity_pct": sparsity_pct,
                   "workload_key": args.workload, "layers_per_step": len(layers),
                   "sparsity_dist": getattr(args, "sparsity_dist", "uniform"),
                   "kernel": args.kernel, "stream_stores": bool(getattr(args, "stream_stores", False)),
                   "streams": n_streams,
                   "parallelism": "batch-sharded x%d" % world,
                   "weight_broadcast_ms": round(t_bcast * 1e3, 3) if dist_on else None},
        "weight_broadcast_ms": round(t_bcast * 1e3, 3) if dist_on else None,
        # one-time costs outside the timed region (the reference's WeightAlign runs once per weight load,
        # net.cpp:819): rank 0's WeightAlign per layer -- it now generates and assembles code --, the
        # generated code's size, and (N > 1) what a RECEIVER spends in set_csr after the broadcast
        # (`first_load_ms`: what the process's FIRST generated-code WeightAlign costs on top of a second one of the same
        #  layer -- the code object template assembled once per process and the first HIP module load -- paid by a
        #  throw-away plan before the layers are aligned, so the per-layer figures are the layers' own)
        "weight_align_ms": {"total": round(sum(setup["align_ms"]), 2),
                            "max_per_layer": round(max(setup["align_ms"]), 2) if setup["align_ms"] else None,
                            "per_layer": [round(v, 2) for v in setup["align_ms"]],
                            "first_load_ms": None if setup.get("first_load_ms") is None else round(setup["first_load_ms"], 2),
                            "layers": len(setup["align_ms"])},
        "generated_code_bytes": setup["code_bytes"], "plan_device_bytes": setup["device_bytes"],
        # per distinct layer shape: how evenly WeightAlign's channel deal loads the waves that meet at a block's barrier
        # (slowest wave / mean wave, weighted over all blocks; the worst single block), and the largest code object
        "channel_deal": [{"layer": n, "slowest_over_mean": max(v[0] for v in vs) / 1000.0, "worst_block": max(v[1] for v in vs) / 1000.0,
                          "max_code_bytes": max(v[2] for v in vs)}
                         for n, vs in _group_deal(setup.get("deal", []))],
        "weight_receive_ms": receive,
        "backend": be.name, "dist_backend": (be.dist_backend if test_be(be) else args.dist_backend) if dist_on else None,
        "buffers": "one bottom/top pair per layer (no launch re-reads the previous launch's input)",
        "outputs_dumped": None if dumped is None else {"dir": args.dump_outputs, "files": len(dumped)},
    }
    if not full:
        return out
    out.update({
        # the K steps right after the W warm-up steps, BEFORE the settle loop (clocks not yet settled)
        "ms_per_step_cold": None if cold_ms is None else round(cold_ms, 4),
        # R timed regions of K steps each; value / ms_per_step are the MEDIAN region's
        "repeats": len(regions), "ms_per_step_min": round(min(region_ms), 4),
        "ms_per_step_max": round(max(region_ms), 4),
        "ms_per_step_regions": [round(v, 4) for v in region_ms],
        "parity_max_rel_err": float("%.3g" % parity),
        "cross_rank_checksum_rel_diff": None if cross is None else float("%.3g" % cross),
        "roofline": roofline,
    })
    if parity > 1e-4 or (cross is not None and cross > 1e-5):
        out["parity_failed"] = True
        log("PARITY FAILURE: parity_max_rel_err=%g cross_rank=%r" % (parity, cross))
    if world == 1 and not dist_on and not test_be(be) and not args.no_extras and args.workload == "resnet50" and \
            args.sparsity is None and args.batch is None and not strong and args.kernel == "auto" and n_streams == 1:
        # the other single-GPU configurations and the sparsity sweep, AFTER the headline region (its buffers freed first)
        del bottoms, tops, shape_bottoms
        for (s_, plan_, *_rest) in layers:
            plan_.close()
        torch.cuda.empty_cache()
        log("other configs + sparsity sweep (after the timed region, budget %.0f s):" % args.extras_budget)
        other, sweep, skipped, took = measure_extras(be, pkg, synth, oracle, args.extras_budget)
        headline = {"workload": "resnet50", "sparsity_pct": sparsity_pct, "batch": per_gpu_batch,
                    "ms_per_step": out["ms_per_step"], "images_per_s": out["value"],
                    "frac": round(total_alg / (HBM_PEAK_GBS * 1e9) / (ms_per_step * 1e-3), 4),
                    "binding_frac": round(t_bind / (ms_per_step * 1e-3), 4),
                    "parity_max_rel_err": out["parity_max_rel_err"], "dominant_kernel": dom_label, "same_as": "the headline line"}
        out["other_configs"] = other
        table = list(sweep) + [headline]
        if "alexnet" in other:
            table.append(dict({k: v for k, v in other["alexnet"].items() if k != "per_layer"}, same_as="other_configs.alexnet"))
        out["sparsity_sweep"] = sorted(table, key=lambda r: (r["workload"], r["sparsity_pct"]))
        out["extras"] = {"wall_s": took, "skipped": skipped,
                         "note": "timed after the headline region, never inside it; K steps between two HIP events on the "
                                 "launch stream, median of 3 regions; same synthetic data rules, parity vs the oracle per config"}
        if any(r.get("parity_failed") for r in list(other.values()) + sweep):
            out["parity_failed"] = True
    if world == 1 and not args.no_cpu:
        log("cpu_baseline (bounded sample, %.0f s budget):" % args.cpu_budget)
        out["cpu_baseline"] = cpu_baseline(oracle, synth, shapes, args.cpu_budget)
        if hasattr(pkg, "cpu_kernel_name") and not test_be(be):
            info = _HOST_INFO or host_cpu_info()
            out["cpu_baseline"]["product_cpu_mode"] = product_cpu_mode(pkg, synth, shapes, info["hw_threads"], 4.0)
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default: per workload, see DEFAULT_STEPS)")
    ap.add_argument("--warmup", type=int, default=None, help="untimed warm-up steps (default: per workload)")
    ap.add_argument("--repeats", type=int, default=5,
                    help="--full: timed regions of --steps steps each; value = the median region (SURVEY 8d).  A plain "
                         "run times one region")
    ap.add_argument("--settle-ms", type=float, default=300.0,
                    help="run the step untimed for this long after the warm-up steps, before the timed region (clock settling; "
                         "0: not at all)")
    ap.add_argument("--workload", default="resnet50")
    ap.add_argument("--batch", type=int, default=None, help="images per GPU (weak scaling)")
    ap.add_argument("--global-batch", type=int, default=None,
                    help="total images over all GPUs (strong scaling; BASELINE configs[3]: 2048)")
    ap.add_argument("--sparsity", type=float, default=None)
    ap.add_argument("--sparsity-dist", default="uniform",
                    choices=["uniform", "channel", "zero_inputs", "filters_tail", "i", "ii", "iii"],
                    help="how the nonzeros lie at the same total count: uniform (the BASELINE configs); i = channel: "
                         "per-output-channel density ~U(0, 2d); ii = zero_inputs: 20 %% of the input channels all zero; "
                         "iii = filters_tail: 10 %% of the filters all zero and 5 %% of the rows at 4d -- what a pruned "
                         "model looks like (the reference's nets are SkimCaffe-pruned, run.sh:14)")
    ap.add_argument("--kernel", default="auto", choices=["auto", "generic", "tiled", "jit"],
                    help="auto = generated code (jit) where available; tiled = the LDS-staged stream kernel")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline figure: cold steps, --repeats regions "
                         "with per-launch events (roofline), parity against the CPU oracle, the cross-rank check, the other "
                         "configurations and the sparsity sweep, the CPU baselines")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the top blob of every layer as DIR/<name>.npy (float32; a fixed, "
                         "seeded sample of a larger blob; at most 48 MB in all)")
    ap.add_argument("--cpu-budget", type=float, default=20.0, help="--full: seconds for the cpu_baseline leg")
    ap.add_argument("--no-cpu", action="store_true", help="--full: no cpu_baseline leg")
    ap.add_argument("--no-extras", action="store_true",
                    help="--full: skip the other single-GPU configurations and the sparsity sweep that the default 1-GPU ResNet run "
                         "times after its headline region (profiling runs: the kernel averages then are the headline's)")
    ap.add_argument("--extras-budget", type=float, default=55.0, help="--full: seconds for other_configs + sparsity_sweep")
    ap.add_argument("--stream-stores", action="store_true",
                    help="plan option stream_stores = 1: pointwise layers write their top blob with non-temporal "
                         "stores (the layers of a step have no consumer here; a net's next layer reads the blob, "
                         "and the default keeps it cached -- tools/producer_consumer.py)")
    ap.add_argument("--code-loader", type=int, default=0, choices=[0, 1],
                    help="plan option code_loader: 0 = generated code into executable device memory the library fills itself "
                         "(default), 1 = through the HIP module loader (the fallback; for comparisons)")
    ap.add_argument("--broadcast", default="aligned", choices=["aligned", "csr"],
                    help="N > 1: what rank 0 broadcasts per layer -- the aligned form incl. the generated code (receivers "
                         "load it as it is), or the CSR alone (receivers run their own WeightAlign tail)")
    ap.add_argument("--receive-threads", type=int, default=1,
                    help="N > 1: host threads a receiver imports its layers on (the code object loads of different plans "
                         "can overlap: tools/dbg/import_threads.py; in the bench's own flow 4 threads measured SLOWER than 1 -- "
                         "66 against 48 ms for the 16 ResNet layers, profiles/r06_receive_threads.md -- so the default is layer by layer)")
    ap.add_argument("--streams", type=int, default=1,
                    help="issue the step's (independent) layers round robin on this many HIP streams; 1 = one stream, as "
                         "the reference launches its layers (the default and the judged line)")
    ap.add_argument("--force-dist", action="store_true",
                    help="run the distributed code path whatever --gpus says: with --gpus 1, ONE rank under "
                         "torch.distributed.run goes through init_process_group (RCCL), the weight broadcast, export / "
                         "import of the aligned form (rank 0 is its own receiver), the barriers, the MAX reduction and the "
                         "cross-rank check -- the RCCL path on the hardware a one-GPU box has")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="nccl = RCCL (the driver's runs); gloo lets two ranks share one GPU for a rehearsal")
    args = ap.parse_args(argv)
    args.sparsity_dist = {"i": "channel", "ii": "zero_inputs", "iii": "filters_tail"}.get(args.sparsity_dist, args.sparsity_dist)
    global WEIGHT_DIST
    WEIGHT_DIST = args.sparsity_dist
    k, w = DEFAULT_STEPS.get(args.workload, (100, 20))
    if args.steps is None:
        args.steps = k
    if args.warmup is None:
        args.warmup = w
    return args


def _free_port():
    import socket
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    return port


def launch_ranks(n_ranks, argv, script=None):
    """`python bench.py --gpus N` with no RANK / WORLD_SIZE in the environment: start the N ranks.

    The reference's one command starts a worker per GPU itself (tools/caffe.cpp:254-256 ->
    P2PSync::Run, parallel.cpp:328-358).  Here the workers are processes: this parent starts
    `python -m torch.distributed.run --nproc-per-node N bench.py <same arguments>` as a CHILD, before
    torch or HIP has been imported here -- it never touches the GPU and replaces no process --,
    forwards the children's stderr, relays the one JSON line of rank 0 and returns the worst exit
    code (no JSON line from a run that claims success is a failure too)."""
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: what RCCL needs on this host
    env.setdefault("MASTER_ADDR", "127.0.0.1")
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", str(n_ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), script or os.path.abspath(__file__)] + list(argv)
    log("bench.py: starting %d ranks: %s" % (n_ranks, " ".join(cmd)))
    child = subprocess.Popen(cmd, stdout=subprocess.PIPE, env=env, cwd=ROOT)
    line = None
    for raw in child.stdout:
        text = raw.decode("utf-8", "replace").rstrip("\n")
        if text.startswith("{") and '"metric"' in text:
            try:
                json.loads(text)
                line = text
                continue
            except ValueError:
                pass
        log(text)
    rc = child.wait()
    if line is not None:
        print(line, flush=True)
    elif rc == 0:
        log("bench.py: the ranks exited 0 without a JSON line")
        rc = 1
    return rc if rc >= 0 else 128 - rc


def main(backend_factory=None, script=None):
    """backend_factory / script: the CPU test-suite's entry (tests/bench_stub_main.py) passes a stub
    backend and its own path, so that launcher, rendezvous and reporting run on a box without a GPU;
    `python bench.py` itself knows one backend, the HIP library."""
    args = parse_args()
    world_env = os.environ.get("WORLD_SIZE")
    if (args.gpus > 1 or args.force_dist) and world_env is None:
        sys.exit(launch_ranks(args.gpus, sys.argv[1:], script))      # nothing below runs in the launcher
    # the host's CPU share is read BEFORE any OpenMP runtime exists: with OMP_PROC_BIND set, the
    # runtime torch loads pins this thread to one core and the affinity mask then reads "2 threads"
    global _HOST_INFO, _ALLOWED_CPUS
    _HOST_INFO = host_cpu_info()
    try:
        _ALLOWED_CPUS = set(os.sched_getaffinity(0))
    except AttributeError:
        _ALLOWED_CPUS = None
    # OpenMP placement for the cpu_baseline leg must be in the environment before libgomp loads
    os.environ.setdefault("OMP_PROC_BIND", "close")
    os.environ.setdefault("OMP_PLACES", "cores")
    import torch.distributed as dist

    pkg = ge.load_package()
    synth = pkg.synth
    rank = int(os.environ.get("RANK", "0"))
    world = int(world_env or "1")
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus (%d) != WORLD_SIZE (%d)" % (args.gpus, world))
    kernel = {"auto": pkg.KERNEL_AUTO, "generic": pkg.KERNEL_GENERIC, "tiled": pkg.KERNEL_TILED,
              "jit": pkg.KERNEL_JIT}[args.kernel]
    if backend_factory is not None:
        be = backend_factory(local_rank)
        args.dist_backend = be.dist_backend
    else:
        be = HipBackend(pkg, local_rank, kernel, stream_stores=args.stream_stores, code_loader=args.code_loader)
    dist_on = world > 1 or args.force_dist
    if dist_on:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=be.device)
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)
    out = run(args, be, pkg, synth, ge.load_oracle, dist if dist_on else None)
    if out is not None:
        if backend_factory is not None:
            out["test_backend"] = True
        print(json.dumps(out), flush=True)
    if dist_on:
        dist.barrier()
        dist.destroy_process_group()
    # wrong results are not a throughput: the line above carries "parity_failed", the exit code says it too
    failed = bool(out.get("parity_failed")) if out is not None else False
    if failed:
        sys.exit(1)


if __name__ == "__main__":
    main()
