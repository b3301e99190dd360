// wgrad_bf16.hip -- the bf16 math mode of the MFMA weight-gradient kernels (plan option "wgrad_math" = ESCOIN_MATH_BF16;
// include/escoin.h "bf16 weight gradient"): per conv group
//     dW[Mg x Kd] = bf16(G)[Mg x P] * bf16(im2col(bottom))[P x Kd],   fp32 sums,
// G = top_diff (x [top > 0] on fuse_relu plans, masked BEFORE the rounding), on v_mfma_f32_32x32x16_bf16.  Two thin bodies
// around the step loop of wgrad_bf16_step.h (steps of 64 pixels, quads of 4 pixels staged by 16-byte loads where the
// geometry and the pointers allow, k-contiguous swizzled bf16 tiles, 4 matrix instructions per wave and step):
//   escoin_sconv_wgrad_bf16_kernel   the twin of escoin_sconv_wgrad_mfma_kernel (wgrad_mfma.hip): its arguments, tables and
//       grid (chunk, group * mtiles, ktiles); the tile's CSR entries go to slab_w[chunk][entry] for the same stage 2;
//   escoin_dense_wgrad_bf16_kernel   the twin of escoin_dense_wgrad_mfma_kernel (dense_wgrad.hip): its arguments and grid
//       (split, group * mtiles, ktiles); the whole tile goes to part[split] for the same sum kernel.
// The option holds no state: the launches below are handed the fp32 launches' filled argument blocks.  The blobs stay fp32;
// the bias gradient does not pass here.  No atomics, one writer per slab element; every staging variant gives the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "align_rules.h"
#include "escoin_plan.h"
#include "wgrad_bf16_step.h"

namespace escoin {

template <bool RELU, bool GV, bool XV>
__global__ void __launch_bounds__(kWgmThreads)
escoin_sconv_wgrad_bf16_kernel(WgmArgs a) {
  __shared__ __attribute__((aligned(16))) wgb_bf16x8 sG[2][kWgbTileChunks];
  __shared__ __attribute__((aligned(16))) wgb_bf16x8 sX[2][kWgbTileChunks];
  const int tid = threadIdx.x;
  const int chunk = blockIdx.x;
  const int grp = blockIdx.y / a.mtiles, mt = blockIdx.y - grp * a.mtiles, kt = blockIdx.z;
  if (a.tile_cnt[((size_t)grp * a.mtiles + mt) * a.ktiles + kt] == 0) return;   // (the whole workgroup: before any barrier)
  const int m0 = mt * kWgmTileM, k0 = kt * kWgmTileK;
  const long q0 = (long)chunk * kBwdChunkPixels;
  const int live = (int)min((long)kBwdChunkPixels, a.in.total - q0);
  const wgm_f32x16 acc = wgb_tile_sum<RELU, GV, XV>(a.in, sG, sX, grp, m0, k0, q0, live);

  const int k = k0 + wgm_out_col(tid);
  if (k >= a.Kd) return;
  float *__restrict__ out = a.slab_w + (size_t)chunk * a.nnz;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int m = m0 + wgm_out_row(tid, reg);
    if (m >= a.in.Mg) continue;
    const int e = a.ent[((size_t)grp * a.in.Mg + m) * a.Kd + k];
    if (e >= 0) out[e] = acc[reg];
  }
}

template <bool RELU, bool GV, bool XV>
__global__ void __launch_bounds__(kWgmThreads)
escoin_dense_wgrad_bf16_kernel(DwgArgs a) {
  __shared__ __attribute__((aligned(16))) wgb_bf16x8 sG[2][kWgbTileChunks];
  __shared__ __attribute__((aligned(16))) wgb_bf16x8 sX[2][kWgbTileChunks];
  const int tid = threadIdx.x;
  const int split = blockIdx.x;
  const int grp = blockIdx.y / a.mtiles, mt = blockIdx.y - grp * a.mtiles, kt = blockIdx.z;
  const int m0 = mt * kWgmTileM, k0 = kt * kWgmTileK;
  const long q0 = (long)split * a.span_pixels;
  const int live = (int)min((long)a.span_pixels, a.in.total - q0);      // > 0: the grid holds live spans only
  const wgm_f32x16 acc = wgb_tile_sum<RELU, GV, XV>(a.in, sG, sX, grp, m0, k0, q0, live);

  const int k = k0 + wgm_out_col(tid);
  if (k >= a.Kd) return;
  float *__restrict__ out = a.part + (size_t)split * (size_t)a.positions;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int m = m0 + wgm_out_row(tid, reg);
    if (m < a.in.Mg) out[((size_t)grp * a.in.Mg + m) * a.Kd + k] = acc[reg];
  }
}

// The staging variant of a call: what the geometry allows (align_rules.h wgb_plan) and the call's pointers are aligned for.
// A blob passed as a window into a larger buffer takes the 4-byte path.
static int wgb_variant(const Geometry &g, const WgmIn &in, bool relu) {
  WgbPlan bp;
  if (!wgb_plan(g, false, &bp)) return 0;
  auto aligned = [](const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  const bool gv = bp.vec_g && aligned(in.top_diff) && (!relu || aligned(in.top));
  const bool xv = bp.vec_x && aligned(in.bottom);
  return (gv ? 1 : 0) + (xv ? 2 : 0);
}

// kernel<RELU, GV, XV> by the run-time triple
#define ESCOIN_WGB_LAUNCH(KERNEL, relu, variant, grid, stream, a)                                                     \
  do {                                                                                                                \
    const dim3 block_(kWgmThreads);                                                                                   \
    switch ((relu ? 4 : 0) + (variant)) {                                                                             \
      case 0: hipLaunchKernelGGL((KERNEL<false, false, false>), grid, block_, 0, stream, a); break;                   \
      case 1: hipLaunchKernelGGL((KERNEL<false, true, false>), grid, block_, 0, stream, a); break;                    \
      case 2: hipLaunchKernelGGL((KERNEL<false, false, true>), grid, block_, 0, stream, a); break;                    \
      case 3: hipLaunchKernelGGL((KERNEL<false, true, true>), grid, block_, 0, stream, a); break;                     \
      case 4: hipLaunchKernelGGL((KERNEL<true, false, false>), grid, block_, 0, stream, a); break;                    \
      case 5: hipLaunchKernelGGL((KERNEL<true, true, false>), grid, block_, 0, stream, a); break;                     \
      case 6: hipLaunchKernelGGL((KERNEL<true, false, true>), grid, block_, 0, stream, a); break;                     \
      default: hipLaunchKernelGGL((KERNEL<true, true, true>), grid, block_, 0, stream, a); break;                     \
    }                                                                                                                 \
  } while (0)

// No allocation, no synchronisation (capturable into a graph), as the fp32 launches.
static int launch_sparse_bf16(const Geometry &g, const WgmArgs &a, dim3 grid, hipStream_t stream, int *variant) {
  *variant = wgb_variant(g, a.in, g.d.fuse_relu != 0);
  ESCOIN_WGB_LAUNCH(escoin_sconv_wgrad_bf16_kernel, g.d.fuse_relu != 0, *variant, grid, stream, a);
  ESCOIN_HIP_TRY(hipGetLastError());
  return ESCOIN_OK;
}

static int launch_dense_wgrad_bf16(const Geometry &g, const DwgArgs &a, dim3 grid, hipStream_t stream, int *variant) {
  *variant = wgb_variant(g, a.in, g.d.fuse_relu != 0);
  ESCOIN_WGB_LAUNCH(escoin_dense_wgrad_bf16_kernel, g.d.fuse_relu != 0, *variant, grid, stream, a);
  ESCOIN_HIP_TRY(hipGetLastError());
  return ESCOIN_OK;
}

// (launch_wgrad_mfma and escoin_dense_wgrad reach these through g_wgb_hooks, wgrad_mfma_step.h: a program that links the
// core's objects alone still links, and refuses the option there)
namespace {
__attribute__((used)) const bool g_registered = (g_wgb_hooks = WgbHooks{launch_sparse_bf16, launch_dense_wgrad_bf16}, true);
}  // namespace

}  // namespace escoin
