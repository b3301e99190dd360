// wgrad_pointwise.hip -- stage 1 of the weight / bias gradient for pointwise layers (plan option "wgrad_pointwise"): the
// sampled product
//     dW[m][c] = sum over the pixels q of G[m][q] * X[c][q]        for the CSR's (m, c) pairs only,
// G = top_diff (x [top > 0] on fuse_relu plans), X = the bottom at the pixel's strided position, on float plans with
// KH = KW = 1 and pad 0 (align_rules.h pw_plan: the predicate and the tiling).  It fills the backward's slab -- same chunks
// of kBwdChunkPixels flattened (n, oh, ow) pixels, same slab_w[chunk][entry] and slab_b[chunk][m] -- and stage 2 is
// escoin_sconv_wgrad_tree_sum_kernel (sconv_backward.hip).
//
// One workgroup of kPwThreads lanes per (tile, chunk); a tile is an m-slice of a conv group crossed with a block of its
// input channels (csr_tables.h pw_tables).  The chunk is walked kPwStepPixels pixels at a time:
//   staging   the tile's G rows and bottom rows of the step into LDS, one row of kPwPitch floats each (16-byte aligned,
//             consecutive rows four banks apart).  Lane t stages pixel t % 32 of rows t / 32, t / 32 + 8, ...: one pixel
//             decode per lane and step, shared by all rows, and eight rows' loads in flight per round.  The ReLU mask and
//             the stride gather are applied here; a pixel at or past the call's last one is +0 in every row and reads no
//             memory;
//   walk      a lane owns up to E entries of the tile (E = 1, 2, 4, 8, 16: template instantiations); per entry and step
//             eight pairs of 16-byte LDS reads (G row, bottom row) and 32 FMAs into the entry's accumulator register, pixels
//             ascending.  An entry's two row offsets sit packed in one register;
//   bias      summed by the tiles of c-block 0, one lane per G row, pixels ascending; a bias-only call launches those tiles
//             alone, stages no bottom and walks no entry.
// The accumulators live across the chunk's steps and are stored once.  Steps past the call's last pixel are not walked.
// slab_w[chunk][e] is therefore ONE lane's fma chain from +0 over the chunk's live pixels in ascending order (then over the
// +0 products of the last step's dead pixels), slab_b[chunk][m] one lane's chain of additions: their bits are a function of
// the geometry, the pattern's positions and n_images, whatever the tiling.  No atomics, one writer per slab element, nothing
// read or written outside the pattern; a non-finite bottom element reaches the entries of its channel only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "align_rules.h"
#include "csr_tables.h"
#include "escoin_plan.h"

namespace escoin {

struct PwArgs {
  const float *__restrict__ bottom;
  const float *__restrict__ top_diff;
  const float *__restrict__ top;      // fuse_relu only
  const int *__restrict__ tile;       // [tiles][kPwTileWords]
  const int *__restrict__ ent;        // per item
  const int *__restrict__ pk;         // per item
  float *__restrict__ slab_w;         // [chunks][nnz]
  float *__restrict__ slab_b;         // [chunks][M]
  unsigned total;                     // n_images * OH * OW
  int nnz;
  int C, M, W, OW, opix, plane;       // opix = OH * OW, plane = H * W
  int stride_h, stride_w;
  int Cg, Mg;
  int want_w, want_b;
};

constexpr int kPwStageBatch = 8;      // rows a lane loads per staging round

template <int E, bool RELU>
__global__ void __launch_bounds__(kPwThreads)
escoin_sconv_wgrad_pointwise_kernel(PwArgs a) {
  extern __shared__ float4 pw_lds4[];
  float *lds = reinterpret_cast<float *>(pw_lds4);
  const int tid = threadIdx.x;
  const int *__restrict__ td = a.tile + (size_t)blockIdx.x * kPwTileWords;
  const int grp = td[0], row0 = td[1], rows = td[2], c0 = td[3], chans = td[4], first = td[5];
  const int items = a.want_w ? td[6] : 0;
  const bool bias_here = a.want_b && c0 == 0;
  if (items == 0 && !bias_here) return;    // (the whole workgroup: before any barrier)
  const unsigned q0 = blockIdx.y * (unsigned)kBwdChunkPixels;
  const int live = (int)min((unsigned)kBwdChunkPixels, a.total - q0);
  const int steps = (live + kPwStepPixels - 1) / kPwStepPixels;

  // the lane's entries: ent < 0 = none (its offsets name row 0, which exists: the reads stay inside the tile)
  int ent[E];
  unsigned po[E];    // (float offset of the G row << 16) | float offset of the bottom row
  float acc[E];
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const int i = k * kPwThreads + tid;
    const bool has = i < items;
    ent[k] = has ? a.ent[first + i] : -1;
    const unsigned pk = has ? (unsigned)a.pk[first + i] : 0u;
    po[k] = (((pk >> 16) * kPwPitch) << 16) | ((pk & 0xffffu) * kPwPitch);
    acc[k] = 0.f;
  }
  float bsum = 0.f;
  const bool bias_lane = bias_here && tid < rows;

  const int px = tid & (kPwStepPixels - 1), r8 = tid >> 5;
  constexpr int kRowsPerPass = kPwThreads / kPwStepPixels;
  const float *__restrict__ gsrc = a.top_diff + (size_t)(grp * a.Mg + row0) * a.opix;
  const float *__restrict__ tsrc = RELU ? a.top + (size_t)(grp * a.Mg + row0) * a.opix : nullptr;
  const float *__restrict__ xsrc = a.bottom + (size_t)(grp * a.Cg + c0) * a.plane;
  float *xrows = lds + rows * kPwPitch;
  for (int s = 0; s < steps; ++s) {
    const unsigned q = q0 + (unsigned)(s * kPwStepPixels + px);
    const bool alive = q < a.total;
    const unsigned n = alive ? q / (unsigned)a.opix : 0u;
    const unsigned r = alive ? q - n * (unsigned)a.opix : 0u;
    const unsigned oh = r / (unsigned)a.OW, ow = r - oh * (unsigned)a.OW;
    const size_t gi = (size_t)n * a.M * a.opix + r;
    // kPwStageBatch rows per round: their loads are issued together, under one test of the pixel (a row index past the
    // tile's last is clamped to it for the load and not stored)
    for (int m0 = r8; m0 < rows; m0 += kRowsPerPass * kPwStageBatch) {
      float v[kPwStageBatch], t[kPwStageBatch];
#pragma unroll
      for (int u = 0; u < kPwStageBatch; ++u) v[u] = 0.f, t[u] = 1.f;
      if (alive) {
#pragma unroll
        for (int u = 0; u < kPwStageBatch; ++u) {
          const size_t at = gi + (size_t)min(m0 + u * kRowsPerPass, rows - 1) * a.opix;
          v[u] = gsrc[at];
          if (RELU) t[u] = tsrc[at];
        }
      }
#pragma unroll
      for (int u = 0; u < kPwStageBatch; ++u) {
        const int m = m0 + u * kRowsPerPass;
        if (m < rows) lds[m * kPwPitch + px] = RELU && !(t[u] > 0.f) ? 0.f : v[u];
      }
    }
    if (items > 0) {
      const size_t xi = (size_t)n * a.C * a.plane + (size_t)(oh * a.stride_h) * a.W + ow * a.stride_w;
      for (int c0r = r8; c0r < chans; c0r += kRowsPerPass * kPwStageBatch) {
        float v[kPwStageBatch];
#pragma unroll
        for (int u = 0; u < kPwStageBatch; ++u) v[u] = 0.f;
        if (alive) {
#pragma unroll
          for (int u = 0; u < kPwStageBatch; ++u) v[u] = xsrc[xi + (size_t)min(c0r + u * kRowsPerPass, chans - 1) * a.plane];
        }
#pragma unroll
        for (int u = 0; u < kPwStageBatch; ++u) {
          const int c = c0r + u * kRowsPerPass;
          if (c < chans) xrows[c * kPwPitch + px] = v[u];
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < E; ++k) {
      if (ent[k] < 0) continue;
      const float4 *__restrict__ gr = reinterpret_cast<const float4 *>(lds + (po[k] >> 16));
      const float4 *__restrict__ xr = reinterpret_cast<const float4 *>(lds + (po[k] & 0xffffu));
      float t = acc[k];
#pragma unroll
      for (int j = 0; j < kPwStepPixels / 4; ++j) {
        const float4 gv = gr[j], xv = xr[j];
        t = fmaf(gv.x, xv.x, t);
        t = fmaf(gv.y, xv.y, t);
        t = fmaf(gv.z, xv.z, t);
        t = fmaf(gv.w, xv.w, t);
      }
      acc[k] = t;
    }
    if (bias_lane) {
      const float4 *__restrict__ gr = reinterpret_cast<const float4 *>(lds + tid * kPwPitch);
#pragma unroll
      for (int j = 0; j < kPwStepPixels / 4; ++j) {
        const float4 gv = gr[j];
        bsum += gv.x;
        bsum += gv.y;
        bsum += gv.z;
        bsum += gv.w;
      }
    }
    __syncthreads();
  }
  float *__restrict__ out = a.slab_w + (size_t)blockIdx.y * a.nnz;
#pragma unroll
  for (int k = 0; k < E; ++k)
    if (ent[k] >= 0) out[ent[k]] = acc[k];
  if (bias_lane) a.slab_b[(size_t)blockIdx.y * a.M + grp * a.Mg + row0 + tid] = bsum;
}

int pw_build(const escoin_plan *p, const BwdOptions &o, PwWgrad *w, hipStream_t stream) {
  PwPlan pp;
  const long nnz = plan_nnz(p);
  if (!pw_plan(p->g, p->is_f64, nnz, &p->rowptr, &p->colidx, o.wgrad_channel_block, o.pw_tile_entries, tiled_device_cus(), &pp))
    return fail(ESCOIN_ESTATE, "pointwise weight-gradient kernel: the rule does not serve this plan");
  if (pp.lds_bytes > kPwLdsBudget || pp.lane_entries > kPwMaxLaneEntries)
    return fail(ESCOIN_ESTATE, "pointwise weight-gradient kernel: the tiling exceeds the kernel's limits");
  const PwTables t = pw_tables(csr_view(p), pp);
  w->tiles = (int)pp.tiles.size();
  w->bias_tiles = pp.bias_tiles;
  w->lane_entries = pp.lane_entries;
  w->lds_bytes = pp.lds_bytes;
  ESCOIN_HIP_TRY(w->tile.upload(t.tile, stream));
  ESCOIN_HIP_TRY(w->ent.upload(t.ent, stream));
  ESCOIN_HIP_TRY(w->pk.upload(t.pk, stream));
  ESCOIN_HIP_TRY(hipStreamSynchronize(stream));   // host vectors die at scope exit
  return ESCOIN_OK;
}

template <int E>
static void pw_launch(bool relu, dim3 grid, size_t lds, hipStream_t stream, const PwArgs &a) {
  if (relu) hipLaunchKernelGGL((escoin_sconv_wgrad_pointwise_kernel<E, true>), grid, dim3(kPwThreads), lds, stream, a);
  else hipLaunchKernelGGL((escoin_sconv_wgrad_pointwise_kernel<E, false>), grid, dim3(kPwThreads), lds, stream, a);
}

int launch_wgrad_pointwise(const escoin_plan *p, const PwWgrad &w, long nnz, const float *bottom, const float *top,
                           const float *top_diff, float *slab_w, float *slab_b, int n_images, int chunks, hipStream_t stream) {
  const Geometry &g = p->g;
  const escoin_conv_desc &d = g.d;
  const bool want_w = slab_w != nullptr && nnz > 0, want_b = slab_b != nullptr;
  // the bias alone: the tiles of c-block 0; weights: every tile
  const int tiles = want_w ? w.tiles : want_b ? w.bias_tiles : 0;
  if (tiles == 0 || chunks == 0) return ESCOIN_OK;     // nothing to produce: no launch
  if (!w.tile.get<void>() || !w.ent.get<void>() || !w.pk.get<void>())
    return fail(ESCOIN_ESTATE, "pointwise weight-gradient kernel: the backward state has no tables for it");
  PwArgs a;
  a.bottom = bottom; a.top_diff = top_diff; a.top = top;
  a.tile = w.tile.get<const int>(); a.ent = w.ent.get<const int>(); a.pk = w.pk.get<const int>();
  a.slab_w = slab_w; a.slab_b = slab_b;
  a.total = (unsigned)((long)n_images * g.OH * g.OW);
  a.nnz = (int)nnz;
  a.C = d.C; a.M = d.M; a.W = d.W; a.OW = g.OW; a.opix = g.OH * g.OW; a.plane = d.H * d.W;
  a.stride_h = d.stride_h; a.stride_w = d.stride_w; a.Cg = g.Cg; a.Mg = g.Mg;
  a.want_w = want_w; a.want_b = want_b;
  const dim3 grid((unsigned)tiles, (unsigned)chunks);
  const bool relu = d.fuse_relu != 0;
  switch (w.lane_entries) {
    case 1: pw_launch<1>(relu, grid, w.lds_bytes, stream, a); break;
    case 2: pw_launch<2>(relu, grid, w.lds_bytes, stream, a); break;
    case 4: pw_launch<4>(relu, grid, w.lds_bytes, stream, a); break;
    case 8: pw_launch<8>(relu, grid, w.lds_bytes, stream, a); break;
    default: pw_launch<16>(relu, grid, w.lds_bytes, stream, a); break;
  }
  ESCOIN_HIP_TRY(hipGetLastError());
  return ESCOIN_OK;
}

}  // namespace escoin
