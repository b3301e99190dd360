// wgrad_mfma.hip -- stage 1 of the weight gradient on the fp32 matrix cores (option "wgrad_kernel" = MFMA), for the
// layers the forward keeps dense: per conv group
//     dW[Mg x Kd] = G[Mg x P] * im2col(bottom)[P x Kd],   Kd = Cg*KH*KW,  P = the flattened (n, oh, ow) pixels,
// G = top_diff (x [top > 0] on fuse_relu plans).  The reduction axis is the pixel axis, cut into the backward's chunks of
// kBwdChunkPixels: one workgroup of four waves per (chunk, tile of 64 output channels of a group, tile of 64 columns)
// computes the tile's partial over its chunk and writes the elements that are CSR entries to slab_w[chunk][entry];
// stage 2 (sconv_backward.hip) sums the chunk axis.  Nothing else is written, and a tile without entries leaves at once.
//   steps     the chunk's live pixels, kWgmStepPixels = 32 at a time: thread t stages pixel t % 32 of the step for rows /
//             columns t / 32 + 8 j (j < 8) of both tiles -- G[m][p] from top_diff, X[p][k] gathered from the bottom by the
//             column's decode (ktab: offset inside the image, dy, dx; any stride, pad, dilation) -- into registers, then
//             into LDS as [pixel][65]: the odd row length spreads a wave's stores (consecutive pixels) and the fragment
//             reads below (consecutive rows / columns) over the banks (bank conflicts have not been measured).  Two
//             LDS buffers: the loads of step s + 1 are in flight while step s is multiplied, one barrier per step;
//   multiply  wave (wm, wk) owns the 32 x 32 block (rows 32 wm.., columns 32 wk..): per step 16 v_mfma_f32_32x32x2_f32
//             (exact fp32 products, fp32 sums), lane (i, h) feeding G[32 wm + i][2 u + h] and X[2 u + h][32 wk + i];
//   zeros     pixels at or past n_images*OH*OW, taps outside the image, rows past Mg and columns past Kd are staged as
//             zeros by select (never 0 x a loaded value), so a non-finite bottom element reaches only the columns whose
//             tap reads it and a non-finite G only its own row; steps wholly past the last live pixel are not run.
// The order of an element's sum -- steps ascending, within a step the MFMA's own fixed order over its two pixels -- is
// a function of the geometry and n_images only: no atomics, no inter-workgroup traffic, one writer per slab element.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "align_rules.h"
#include "escoin_plan.h"

namespace escoin {

typedef float wgm_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kWgmThreads = 256;
constexpr int kWgmSlots = kWgmThreads / kWgmStepPixels;        // 8: rows / columns a pass of the workgroup stages
constexpr int kWgmPerThread = kWgmTileM / kWgmSlots;           // 8 elements of each tile per thread and step
constexpr int kWgmTileFloats = kWgmStepPixels * kWgmLdsRow;
static_assert(kWgmTileM == 64 && kWgmTileK == 64 && kWgmStepPixels == 32, "the wave layout below is 2 x 2 blocks of 32 x 32");
static_assert(sizeof(float) * 4 * kWgmTileFloats == kWgmLdsBytes, "align_rules.h reports this kernel's LDS");
static_assert(kBwdChunkPixels % kWgmStepPixels == 0, "a chunk is whole steps");

struct WgmArgs {
  const float *__restrict__ bottom;
  const float *__restrict__ top_diff;
  const float *__restrict__ top;        // fuse_relu only
  const int *__restrict__ ent;          // [M][Kd]: CSR entry or -1
  const int *__restrict__ tile_cnt;     // [group][mtiles][ktiles]
  const int4 *__restrict__ ktab;        // [ktiles * 64]: {offset, dy, dx, valid}
  float *__restrict__ slab_w;           // [chunks][nnz]
  long total;                           // n_images * OH * OW
  int nnz;
  int C, H, W, M, OH, OW;
  int pad_h, pad_w, stride_h, stride_w;
  int Cg, Mg, Kd, mtiles, ktiles;
};

template <bool RELU>
__global__ void __launch_bounds__(kWgmThreads)
escoin_sconv_wgrad_mfma_kernel(WgmArgs a) {
  __shared__ float sG[2][kWgmTileFloats];
  __shared__ float sX[2][kWgmTileFloats];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int chunk = blockIdx.x;
  const int grp = blockIdx.y / a.mtiles, mt = blockIdx.y - grp * a.mtiles, kt = blockIdx.z;
  if (a.tile_cnt[((size_t)grp * a.mtiles + mt) * a.ktiles + kt] == 0) return;   // (the whole workgroup: before any barrier)
  const int m0 = mt * kWgmTileM, k0 = kt * kWgmTileK;
  const int opix = a.OH * a.OW;
  const size_t plane = (size_t)a.H * a.W;
  const long q0 = (long)chunk * kBwdChunkPixels;
  const int live = (int)min((long)kBwdChunkPixels, a.total - q0);
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

  // C/D layout of the 32 x 32 block: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
  const int k = k0 + wk * 32 + li;
  if (k >= a.Kd) return;
  float *__restrict__ out = a.slab_w + (size_t)chunk * a.nnz;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int m = m0 + wm * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
    if (m >= a.Mg) continue;
    const int e = a.ent[((size_t)grp * a.Mg + m) * a.Kd + k];
    if (e >= 0) out[e] = acc[reg];
  }
}

int wgm_build(escoin_plan *p, BwdState *s, hipStream_t stream) {
  WgmPlan wp;
  if (!wgm_plan(p->g, p->is_f64, &wp)) return fail(ESCOIN_EINVAL, "wgrad_kernel: the MFMA weight-gradient kernel does not serve this plan");
  const WgmTables t = wgrad_mfma_tables(csr_view(p), wp.tile_m, wp.tile_k);
  s->wgm_mtiles = wp.mtiles;
  s->wgm_ktiles = wp.ktiles;
  s->wgm_lds_bytes = wp.lds_bytes;
  ESCOIN_HIP_TRY(s->wgm_ent.upload(t.ent, stream));
  ESCOIN_HIP_TRY(s->wgm_cnt.upload(t.tile_cnt, stream));
  ESCOIN_HIP_TRY(s->wgm_ktab.upload(t.ktab, stream));
  ESCOIN_HIP_TRY(hipStreamSynchronize(stream));   // host vectors die at scope exit
  return ESCOIN_OK;
}

int launch_wgrad_mfma(const escoin_plan *p, const BwdState *s, const float *bottom, const float *top,
                      const float *top_diff, float *slab_w, int n_images, int chunks, hipStream_t stream) {
  const Geometry &g = p->g;
  const escoin_conv_desc &d = g.d;
  if (s->nnz == 0 || chunks == 0) return ESCOIN_OK;       // nothing to produce: no launch
  if (!s->wgm_ent.get<void>() || !s->wgm_cnt.get<void>() || !s->wgm_ktab.get<void>())
    return fail(ESCOIN_ESTATE, "MFMA weight-gradient kernel: the backward state has no tables for it");
  WgmArgs a;
  a.bottom = bottom; a.top_diff = top_diff; a.top = top;
  a.ent = s->wgm_ent.get<const int>(); a.tile_cnt = s->wgm_cnt.get<const int>(); a.ktab = s->wgm_ktab.get<const int4>();
  a.slab_w = slab_w;
  a.total = (long)n_images * g.OH * g.OW;
  a.nnz = (int)s->nnz;
  a.C = d.C; a.H = d.H; a.W = d.W; a.M = d.M; a.OH = g.OH; a.OW = g.OW;
  a.pad_h = d.pad_h; a.pad_w = d.pad_w; a.stride_h = d.stride_h; a.stride_w = d.stride_w;
  a.Cg = g.Cg; a.Mg = g.Mg; a.Kd = g.kdim; a.mtiles = s->wgm_mtiles; a.ktiles = s->wgm_ktiles;
  const dim3 grid((unsigned)chunks, (unsigned)(d.group * s->wgm_mtiles), (unsigned)s->wgm_ktiles), block(kWgmThreads);
  if (d.fuse_relu) hipLaunchKernelGGL(escoin_sconv_wgrad_mfma_kernel<true>, grid, block, 0, stream, a);
  else hipLaunchKernelGGL(escoin_sconv_wgrad_mfma_kernel<false>, grid, block, 0, stream, a);
  ESCOIN_HIP_TRY(hipGetLastError());
  return ESCOIN_OK;
}

}  // namespace escoin
