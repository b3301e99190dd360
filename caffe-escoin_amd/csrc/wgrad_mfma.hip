// wgrad_mfma.hip -- stage 1 of the weight gradient on the fp32 matrix cores (option "wgrad_kernel" = MFMA), for the
// layers the forward keeps dense: per conv group
//     dW[Mg x Kd] = G[Mg x P] * im2col(bottom)[P x Kd],   Kd = Cg*KH*KW,  P = the flattened (n, oh, ow) pixels,
// G = top_diff (x [top > 0] on fuse_relu plans).  The reduction axis is the pixel axis, cut into the backward's chunks of
// kBwdChunkPixels: one workgroup of four waves per (chunk, tile of 64 output channels of a group, tile of 64 columns)
// computes the tile's partial over its chunk and writes the elements that are CSR entries to slab_w[chunk][entry];
// stage 2 (sconv_backward.hip) sums the chunk axis.  Nothing else is written, and a tile without entries leaves at once.
// The step loop -- staging, double buffering, the 16-MFMA multiply and the zero-by-select rules -- is wgrad_mfma_step.h,
// which the dense weight gradient (dense_wgrad.hip) shares.
// The order of an element's sum -- steps ascending, within a step the MFMA's own fixed order over its two pixels -- is
// a function of the geometry and n_images only: no atomics, no inter-workgroup traffic, one writer per slab element.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "align_rules.h"
#include "escoin_plan.h"
#include "wgrad_mfma_step.h"

namespace escoin {

struct WgmArgs {
  WgmIn in;                             // the blobs, the column decode, the geometry (wgrad_mfma_step.h)
  const int *__restrict__ ent;          // [M][Kd]: CSR entry or -1
  const int *__restrict__ tile_cnt;     // [group][mtiles][ktiles]
  float *__restrict__ slab_w;           // [chunks][nnz]
  int nnz;
  int Kd, mtiles, ktiles;
};

template <bool RELU>
__global__ void __launch_bounds__(kWgmThreads)
escoin_sconv_wgrad_mfma_kernel(WgmArgs a) {
  __shared__ float sG[2][kWgmTileFloats];
  __shared__ float sX[2][kWgmTileFloats];
  const int tid = threadIdx.x;
  const int chunk = blockIdx.x;
  const int grp = blockIdx.y / a.mtiles, mt = blockIdx.y - grp * a.mtiles, kt = blockIdx.z;
  if (a.tile_cnt[((size_t)grp * a.mtiles + mt) * a.ktiles + kt] == 0) return;   // (the whole workgroup: before any barrier)
  const int m0 = mt * kWgmTileM, k0 = kt * kWgmTileK;
  const long q0 = (long)chunk * kBwdChunkPixels;
  const int live = (int)min((long)kBwdChunkPixels, a.in.total - q0);
  const wgm_f32x16 acc = wgm_tile_sum<RELU>(a.in, sG, sX, grp, m0, k0, q0, live);

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

int wgm_build(const escoin_plan *p, const WgmPlan &wp, WgmState *w, hipStream_t stream) {
  const WgmTables t = wgrad_mfma_tables(csr_view(p), wp.tile_m, wp.tile_k);
  w->mtiles = wp.mtiles;
  w->ktiles = wp.ktiles;
  w->lds_bytes = wp.lds_bytes;
  ESCOIN_HIP_TRY(w->ent.upload(t.ent, stream));
  ESCOIN_HIP_TRY(w->cnt.upload(t.tile_cnt, stream));
  ESCOIN_HIP_TRY(w->ktab.upload(t.ktab, stream));
  ESCOIN_HIP_TRY(hipStreamSynchronize(stream));   // host vectors die at scope exit
  return ESCOIN_OK;
}

int launch_wgrad_mfma(const escoin_plan *p, const WgmState &w, long nnz, const float *bottom, const float *top,
                      const float *top_diff, float *slab_w, int n_images, int chunks, hipStream_t stream) {
  const Geometry &g = p->g;
  const escoin_conv_desc &d = g.d;
  if (nnz == 0 || chunks == 0) return ESCOIN_OK;       // nothing to produce: no launch
  if (!w.ent.get<void>() || !w.cnt.get<void>() || !w.ktab.get<void>())
    return fail(ESCOIN_ESTATE, "MFMA weight-gradient kernel: the backward state has no tables for it");
  WgmArgs a;
  a.in.bottom = bottom; a.in.top_diff = top_diff; a.in.top = top; a.in.ktab = w.ktab.get<const int4>();
  a.ent = w.ent.get<const int>(); a.tile_cnt = w.cnt.get<const int>();
  a.slab_w = slab_w;
  a.in.total = (long)n_images * g.OH * g.OW;
  a.nnz = (int)nnz;
  a.in.C = d.C; a.in.H = d.H; a.in.W = d.W; a.in.M = d.M; a.in.OH = g.OH; a.in.OW = g.OW;
  a.in.pad_h = d.pad_h; a.in.pad_w = d.pad_w; a.in.stride_h = d.stride_h; a.in.stride_w = d.stride_w;
  a.in.Cg = g.Cg; a.in.Mg = g.Mg; a.Kd = g.kdim; a.mtiles = w.mtiles; a.ktiles = w.ktiles;
  const dim3 grid((unsigned)chunks, (unsigned)(d.group * w.mtiles), (unsigned)w.ktiles), block(kWgmThreads);
  if (d.fuse_relu) hipLaunchKernelGGL(escoin_sconv_wgrad_mfma_kernel<true>, grid, block, 0, stream, a);
  else hipLaunchKernelGGL(escoin_sconv_wgrad_mfma_kernel<false>, grid, block, 0, stream, a);
  ESCOIN_HIP_TRY(hipGetLastError());
  return ESCOIN_OK;
}

}  // namespace escoin
