// wgrad_mfma_step.h -- the step loop of the fp32-MFMA weight-gradient kernels, shared by the sparse-position kernel
// (wgrad_mfma.hip: one chunk per workgroup, the tile's CSR entries to the backward's slab) and the dense one
// (dense_wgrad.hip: a span of chunks per workgroup, the whole tile to its own slab), in the way radix_select.h serves
// prune and rewire.  Device code only; the tile constants are align_rules.h's.
//   wgm_tile_sum<RELU>(in, sG, sX, grp, m0, k0, q0, live) = the 64 x 64 tile (rows m0.. of conv group grp, columns k0..)
//   of G[Mg x P] * im2col(bottom)[P x Kd] summed over the `live` pixels from flattened (n, oh, ow) pixel q0 on, as the
//   calling wave's 32 x 32 block in the matrix instruction's C/D layout.  Called by all 256 threads of the workgroup with
//   the same arguments (it holds the loop's barriers).
//   steps     kWgmStepPixels = 32 pixels at a time: thread t stages pixel t % 32 of the step for rows / columns
//             t / 32 + 8 j (j < 8) of both tiles -- G[m][p] from top_diff, X[p][k] gathered from the bottom by the
//             column's decode (ktab: offset inside the image, dy, dx; any stride, pad, dilation) -- into registers, then
//             into LDS as [pixel][65]: the odd row length spreads a wave's stores (consecutive pixels) and the fragment
//             reads (consecutive rows / columns) over the banks (bank conflicts have not been measured).  Two LDS
//             buffers: the loads of step s + 1 are in flight while step s is multiplied, one barrier per step;
//   multiply  wave (wm, wk) owns the 32 x 32 block (rows 32 wm.., columns 32 wk..): per step 16 v_mfma_f32_32x32x2_f32
//             (exact fp32 products, fp32 sums), lane (i, h) feeding G[32 wm + i][2 u + h] and X[2 u + h][32 wk + i];
//   zeros     pixels at or past q0 + live, taps outside the image, rows past Mg and columns past Kd are staged as zeros
//             by select (never 0 x a loaded value), so a non-finite bottom element reaches only the columns whose tap
//             reads it and a non-finite G only its own row; steps wholly past the last live pixel are not run.
// The order of an element's sum: steps ascending from q0, within a step the MFMA's own fixed order over its two pixels.
#ifndef ESCOIN_WGRAD_MFMA_STEP_H_
#define ESCOIN_WGRAD_MFMA_STEP_H_

#include <hip/hip_runtime.h>

#include "align_rules.h"

namespace escoin {

typedef float wgm_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kWgmThreads = 256;
constexpr int kWgmSlots = kWgmThreads / kWgmStepPixels;        // 8: rows / columns a pass of the workgroup stages
constexpr int kWgmPerThread = kWgmTileM / kWgmSlots;           // 8 elements of each tile per thread and step
constexpr int kWgmTileFloats = kWgmStepPixels * kWgmLdsRow;
static_assert(kWgmTileM == 64 && kWgmTileK == 64 && kWgmStepPixels == 32, "the wave layout below is 2 x 2 blocks of 32 x 32");
static_assert(sizeof(float) * 4 * kWgmTileFloats == kWgmLdsBytes, "align_rules.h reports these kernels' LDS");
static_assert(kBwdChunkPixels % kWgmStepPixels == 0, "a chunk is whole steps");

// What the step loop reads: the blobs, the column decode and the geometry.
struct WgmIn {
  const float *__restrict__ bottom;
  const float *__restrict__ top_diff;
  const float *__restrict__ top;        // fuse_relu only
  const int4 *__restrict__ ktab;        // [ktiles * 64]: {offset, dy, dx, valid}
  long total;                           // n_images * OH * OW
  int C, H, W, M, OH, OW;
  int pad_h, pad_w, stride_h, stride_w;
  int Cg, Mg;
};

template <bool RELU>
__device__ __forceinline__ wgm_f32x16 wgm_tile_sum(const WgmIn &a, float (*sG)[kWgmTileFloats], float (*sX)[kWgmTileFloats],
                                                   int grp, int m0, int k0, long q0, int live) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int opix = a.OH * a.OW;
  const size_t plane = (size_t)a.H * a.W;
  const int nsteps = (live + kWgmStepPixels - 1) / kWgmStepPixels;

  // staging role: pixel sp of the step, rows m0 + sr + 8 j of G, columns k0 + sr + 8 j of X
  const int sp = tid & (kWgmStepPixels - 1), sr = tid / kWgmStepPixels;
  int xoff[kWgmPerThread], xdy[kWgmPerThread], xdx[kWgmPerThread];
  unsigned kvalid = 0;
#pragma unroll
  for (int j = 0; j < kWgmPerThread; ++j) {
    const int4 t = a.ktab[k0 + sr + kWgmSlots * j];     // (the table covers whole tiles)
    xoff[j] = t.x; xdy[j] = t.y; xdx[j] = t.z;
    kvalid |= t.w ? (1u << j) : 0u;
  }
  float gv[kWgmPerThread], xv[kWgmPerThread];
  auto load = [&](int s) {
    const int ql = s * kWgmStepPixels + sp;
    const bool plive = ql < live;
    const int q = plive ? (int)(q0 + ql) : 0;           // (N*OH*OW < 2^31: wgm_plan)
    const int n = q / opix, r = q - n * opix;
    const int oh = r / a.OW, ow = r - oh * a.OW;
    const int ih0 = oh * a.stride_h - a.pad_h, iw0 = ow * a.stride_w - a.pad_w;
    const size_t gi = ((size_t)n * a.M + (size_t)grp * a.Mg + m0 + sr) * opix + r;
#pragma unroll
    for (int j = 0; j < kWgmPerThread; ++j) {
      float g = 0.f;
      if (plive && m0 + sr + kWgmSlots * j < a.Mg) {
        const size_t at = gi + (size_t)(kWgmSlots * j) * opix;
        g = a.top_diff[at];
        if (RELU && !(a.top[at] > 0.f)) g = 0.f;
      }
      gv[j] = g;
    }
    const float *__restrict__ xb = a.bottom + ((size_t)n * a.C + (size_t)grp * a.Cg) * plane;
    const long xorg = (long)ih0 * a.W + iw0;
#pragma unroll
    for (int j = 0; j < kWgmPerThread; ++j) {
      const int ih = ih0 + xdy[j], iw = iw0 + xdx[j];
      float x = 0.f;
      if (plive && ((kvalid >> j) & 1u) && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W)
        x = xb[xorg + xoff[j]];
      xv[j] = x;
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int j = 0; j < kWgmPerThread; ++j) {
      sG[buf][sp * kWgmLdsRow + sr + kWgmSlots * j] = gv[j];
      sX[buf][sp * kWgmLdsRow + sr + kWgmSlots * j] = xv[j];
    }
  };

  const int wm = wave >> 1, wk = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  wgm_f32x16 acc = {0};
  load(0);
  for (int s = 0; s < nsteps; ++s) {
    const int buf = s & 1;
    store(buf);
    // everyone's part of step s is in buf -- and everyone is past the multiply of step s - 1, which read the other buffer
    __syncthreads();
    if (s + 1 < nsteps) load(s + 1);
    const float *ga = &sG[buf][lh * kWgmLdsRow + wm * 32 + li];
    const float *xa = &sX[buf][lh * kWgmLdsRow + wk * 32 + li];
#pragma unroll
    for (int u = 0; u < kWgmStepPixels / 2; ++u)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[2 * u * kWgmLdsRow], xa[2 * u * kWgmLdsRow], acc, 0, 0, 0);
  }
  return acc;
}

// C/D layout of a wave's 32 x 32 block: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); these give
// the block's place in the tile.
__device__ __forceinline__ int wgm_out_col(int tid) { return ((tid >> 6) & 1) * 32 + (tid & 31); }
__device__ __forceinline__ int wgm_out_row(int tid, int reg) {
  return (tid >> 7) * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * ((tid & 63) >> 5);
}

}  // namespace escoin
#endif  // ESCOIN_WGRAD_MFMA_STEP_H_
