// dense_wgrad.hip -- the DENSE weight gradient on the fp32 matrix cores (escoin_dense_wgrad, include/escoin.h "Dense
// weight gradient"): every one of the D = M * Kd positions of blobs_[0], inside and outside the plan's pattern -- the score
// escoin_plan_rewire grows by.  Per conv group
//     dW[Mg x Kd] = G[Mg x P] * im2col(bottom)[P x Kd],   Kd = Cg*KH*KW,  P = the flattened (n, oh, ow) pixels,
// G = top_diff (x [top > 0] on fuse_relu plans): the reference's weight_gpu_gemm result.
//   escoin_dense_wgrad_mfma_kernel   grid (split, group * mtiles, ktiles), 256 threads = four waves as 2 x 2 blocks of
//       32 x 32.  The pixel axis is cut into `splits` spans of `span` whole chunks (align_rules.h dwg_plan); a workgroup
//       walks every live step of its span with ONE accumulator set -- the step loop of wgrad_mfma_step.h, which the
//       sparse-position kernel (wgrad_mfma.hip) runs over one chunk -- and writes its whole 64 x 64 tile to
//       part[split][(grp * Mg + m) * Kd + k], guarded by m < Mg, k < Kd.  No entry lookup, no early exit.  Spans without a
//       live pixel are not launched: grid.x = ceil(chunks(n_images) / span).
//   escoin_dense_wgrad_sum_kernel    one lane per position: sums part[0 .. live splits) ascending (16 partials are loaded
//       before they are added, so the loads overlap; the adds keep their order), then out = (accumulate ? out : 0) + sum.
//       Plain stores, one writer per element.
// Contract:
//   - the order of an element's sum -- the spans ascending, inside a span the steps of 32 pixels ascending, inside a step
//     the matrix instruction's own order over its two pixels -- is a function of the geometry, n_images, the device's CU
//     count and option "dense_wgrad_splits" only: the result is the same bits on every call and every stream;
//   - no atomics, and no workgroup waits for another one;
//   - zeros are staged by select, never as 0 x a loaded value: a non-finite bottom element reaches only the columns whose
//     tap reads it, a non-finite G only its own row;
//   - the bank conflicts of the [pixel][65] LDS layout have not been measured, as in the sparse-position kernel.
// The state (DenseWgradState: the column decode table and the partial slab) depends on the descriptor alone; the first
// call builds it (allocations, one synchronisation), later calls allocate and synchronise nothing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "align_rules.h"
#include "escoin_plan.h"
#include "wgrad_mfma_step.h"

namespace escoin {

struct DwgArgs {
  WgmIn in;
  float *__restrict__ part;             // [splits][D]
  long positions;                       // D
  int span_pixels;                      // span * kBwdChunkPixels
  int Kd, mtiles;
};

template <bool RELU>
__global__ void __launch_bounds__(kWgmThreads)
escoin_dense_wgrad_mfma_kernel(DwgArgs a) {
  __shared__ float sG[2][kWgmTileFloats];
  __shared__ float sX[2][kWgmTileFloats];
  const int tid = threadIdx.x;
  const int split = blockIdx.x;
  const int grp = blockIdx.y / a.mtiles, mt = blockIdx.y - grp * a.mtiles, kt = blockIdx.z;
  const int m0 = mt * kWgmTileM, k0 = kt * kWgmTileK;
  const long q0 = (long)split * a.span_pixels;
  const int live = (int)min((long)a.span_pixels, a.in.total - q0);      // > 0: the grid holds live spans only
  const wgm_f32x16 acc = wgm_tile_sum<RELU>(a.in, sG, sX, grp, m0, k0, q0, live);

  const int k = k0 + wgm_out_col(tid);
  if (k >= a.Kd) return;
  float *__restrict__ out = a.part + (size_t)split * (size_t)a.positions;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int m = m0 + wgm_out_row(tid, reg);
    if (m < a.in.Mg) out[((size_t)grp * a.in.Mg + m) * a.Kd + k] = acc[reg];
  }
}

constexpr int kDwgSumThreads = 64;     // one wave: a layer of a few thousand positions still spreads over the CUs
constexpr int kDwgSumBatch = 16;       // partials loaded before they are added: the loads overlap, the order of the adds stays

__global__ void __launch_bounds__(kDwgSumThreads)
escoin_dense_wgrad_sum_kernel(const float *__restrict__ part, float *__restrict__ out, long positions, int live_splits,
                              int accumulate) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= positions) return;
  const float *__restrict__ src = part + p;
  float s = 0.f;
  int i = 0;
  for (; i + kDwgSumBatch <= live_splits; i += kDwgSumBatch) {
    float v[kDwgSumBatch];
#pragma unroll
    for (int j = 0; j < kDwgSumBatch; ++j) v[j] = src[(size_t)(i + j) * (size_t)positions];
#pragma unroll
    for (int j = 0; j < kDwgSumBatch; ++j) s += v[j];
  }
  for (; i < live_splits; ++i) s += src[(size_t)i * (size_t)positions];
  out[p] = (accumulate ? out[p] : 0.f) + s;
}

static const char *const kNoDouble = "dense_wgrad: no double kernel: use escoin_dense_wgrad_cpu_f64";

static int dwg_build(escoin_plan *p, hipStream_t stream) {
  DwgPlan dp;
  if (!dwg_plan(p->g, p->is_f64, tiled_device_cus(), p->dense_wgrad_splits, &dp))
    return fail(ESCOIN_EINVAL, "dense_wgrad: the MFMA kernel needs a float plan whose pixel, weight and image indices fit 31 "
                               "bits; escoin_dense_wgrad_cpu serves this plan");
  p->dwg.reset(new DenseWgradState());
  DenseWgradState *w = p->dwg.get();
  w->device = p->device;
  w->mtiles = dp.tile.mtiles;
  w->ktiles = dp.tile.ktiles;
  w->span = dp.span;
  w->splits = dp.splits;
  w->positions = dp.positions;
  w->lds_bytes = dp.tile.lds_bytes;
  const std::vector<int> ktab = im2col_ktab(p->g, dp.tile.tile_k);
  ESCOIN_HIP_TRY(w->ktab.upload(ktab, stream));
  ESCOIN_HIP_TRY(w->part.alloc(dp.slab_bytes));
  ESCOIN_HIP_TRY(hipStreamSynchronize(stream));   // the host vector dies at scope exit
  return ESCOIN_OK;
}

static int dense_wgrad_gpu(escoin_plan *p, const float *bottom, const float *top, const float *top_diff, float *dense_diff,
                           int n_images, int accumulate, void *stream_v) {
  if (!p) return fail(ESCOIN_EINVAL, "null plan");
  if (const int rc = refuse_deconv(p, "escoin_dense_wgrad")) return rc;
  if (!p->aligned) return fail(ESCOIN_ESTATE, "dense_wgrad called before weight_align / set_csr");
  if (p->is_f64) return fail(ESCOIN_EINVAL, kNoDouble);
  if (const int rc = check_plan_device(p, "dense_wgrad")) return rc;
  const Geometry &g = p->g;
  const escoin_conv_desc &d = g.d;
  if (!top_diff) return fail(ESCOIN_EINVAL, "dense_wgrad: top_diff is required");
  if (!bottom) return fail(ESCOIN_EINVAL, "dense_wgrad: bottom is required");
  if (!dense_diff) return fail(ESCOIN_EINVAL, "dense_wgrad: dense_diff is required");
  if (d.fuse_relu && !top) return fail(ESCOIN_EINVAL, "dense_wgrad: a fuse_relu plan needs the forward's top");
  if (const int rc = check_n_images(p, n_images)) return rc;
  hipStream_t stream = (hipStream_t)stream_v;
  // option "b2s": the inner plan's own dense weight gradient on (X', G') -- M x Cg on both plans; the padding positions are
  // +0 in both operands and add exact zeros.  The state and "dwg_count" are the inner plan's and this plan's.
  if (B2sState *bs = p->b2s_state.get()) {
    ++p->dwg_count;
    const int n_inner = (n_images + bs->bp.B - 1) / bs->bp.B;
    int rc = g_b2s_hooks.pack(p, bottom, nullptr, bs->x.get<float>(), false, n_images, stream);
    if (rc == ESCOIN_OK) rc = g_b2s_hooks.pack(p, top_diff, d.fuse_relu ? top : nullptr, bs->t.get<float>(), true, n_images, stream);
    if (rc != ESCOIN_OK) return rc;
    return escoin_dense_wgrad(bs->inner.plan.get(), bs->x.get<const float>(), nullptr, bs->t.get<const float>(), dense_diff, n_inner,
                              accumulate, stream_v);
  }
  if (!p->dwg || p->dwg->device != p->device) {
    const int rc = dwg_build(p, stream);
    if (rc != ESCOIN_OK) {
      p->dwg.reset();
      return rc;
    }
  }
  const DenseWgradState *w = p->dwg.get();
  ++p->dwg_count;
  if (n_images == 0 && accumulate) return ESCOIN_OK;
  const long total = (long)n_images * g.OH * g.OW;
  const long chunks = (total + kBwdChunkPixels - 1) / kBwdChunkPixels;
  const int live_splits = (int)((chunks + w->span - 1) / w->span);     // <= w->splits: n_images <= N
  if (live_splits > 0) {
    DwgArgs a;
    a.in.bottom = bottom; a.in.top_diff = top_diff; a.in.top = top; a.in.ktab = w->ktab.get<const int4>();
    a.in.total = total;
    a.in.C = d.C; a.in.H = d.H; a.in.W = d.W; a.in.M = d.M; a.in.OH = g.OH; a.in.OW = g.OW;
    a.in.pad_h = d.pad_h; a.in.pad_w = d.pad_w; a.in.stride_h = d.stride_h; a.in.stride_w = d.stride_w;
    a.in.Cg = g.Cg; a.in.Mg = g.Mg;
    a.part = w->part.get<float>();
    a.positions = w->positions;
    a.span_pixels = (int)std::min<long>((long)w->span * kBwdChunkPixels, 0x7fffffffL);   // (never below a span's live pixels)
    a.Kd = g.kdim; a.mtiles = w->mtiles;
    const dim3 grid((unsigned)live_splits, (unsigned)(d.group * w->mtiles), (unsigned)w->ktiles), block(kWgmThreads);
    if (d.fuse_relu) hipLaunchKernelGGL(escoin_dense_wgrad_mfma_kernel<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(escoin_dense_wgrad_mfma_kernel<false>, grid, block, 0, stream, a);
    ESCOIN_HIP_TRY(hipGetLastError());
  }
  const unsigned blocks = (unsigned)((w->positions + kDwgSumThreads - 1) / kDwgSumThreads);
  hipLaunchKernelGGL(escoin_dense_wgrad_sum_kernel, dim3(blocks), dim3(kDwgSumThreads), 0, stream, w->part.get<const float>(), dense_diff,
                     w->positions, live_splits, accumulate ? 1 : 0);
  ESCOIN_HIP_TRY(hipGetLastError());
  return ESCOIN_OK;
}

}  // namespace escoin

using namespace escoin;

extern "C" {

int escoin_dense_wgrad(escoin_plan *plan, const float *bottom_dev, const float *top_dev, const float *top_diff_dev,
                       float *dense_diff_dev, int n_images, int accumulate, void *stream) {
  return guarded([&]() -> int {
    return dense_wgrad_gpu(plan, bottom_dev, top_dev, top_diff_dev, dense_diff_dev, n_images, accumulate, stream);
  });
}

int escoin_dense_wgrad_f64(escoin_plan *plan, const double *, const double *, const double *, double *, int, int, void *) {
  if (!plan) return fail(ESCOIN_EINVAL, "null plan");
  return fail(ESCOIN_EINVAL, kNoDouble);
}

}  // extern "C"
