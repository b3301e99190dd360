// dgrad_mfma.hip -- the data gradient on the fp32 matrix cores (option "backward_kernel" = ESCOIN_BWD_MFMA), for the
// layers that have no transposed forward plan (stride > 1, pad > dil x (K - 1)) and are kept dense.  With G = top_diff
// (x [top > 0] on fuse_relu plans), per conv group
//     bottom_diff[n][c][h][w] = sum over (ocl, kr, kc) of W[ocl][c][kr][kc] * G[n][ocl][oh][ow],
//     oh = (h + pad_h - kr*dil_h) / stride_h exact and inside the top, ow likewise.
// The bottom pixels split into stride_h x stride_w phases ((h + pad_h) % stride_h, (w + pad_w) % stride_w).  Inside a phase
// the contributing taps are the same for every pixel and tap t of phase pixel (hh, ww) reads (hh + dh[t], ww + dw[t]): a
// phase is the stride-1 implicit GEMM
//     dX_phase[Cg x P] = Wt_phase[Cg x Kp] * gather(G)[Kp x P],  Kp = Mg * taps(phase),  P = the phase's (n, hh, ww) pixels
// of the images below n_images.  Every bottom pixel belongs to one phase: bottom_diff is overwritten once per element.  A
// phase without taps (three of the four of a 1x1 stride-2 layer) writes zeros.
// One workgroup of four waves per (phase, tile of 64 phase pixels, (conv group, tile of 64 input channels)) runs the whole
// K reduction: no split-K, no atomics, no second stage.  The tile geometry, the fragment layout and the zero-by-select
// rule are wgrad_mfma.hip's.
//   steps     the (group, phase, channel tile)'s LIVE steps of 32 columns, ascending (the host's list: the steps whose
//             64 x 32 weight block holds a CSR entry; an empty list is the zero-fill case).  Thread t stages pixel / channel
//             t % 64 for columns t / 64 + 4 j (j < 8): the weight block from the phase matrix (csr_tables.h: a step's
//             block is [column][64 channels], so a wave loads 256 contiguous bytes), the G block gathered by the column's
//             decode {G offset of ocl, dh, dw, valid} (wave-uniform), the lanes along consecutive pixels -- into
//             registers, then into LDS as [column][65].  Two LDS buffers: the loads of the next live step are in flight
//             while this one is multiplied, one barrier per step.  The fuse_relu mask is applied while staging.
//   multiply  wave (wc, wp) owns the 32 x 32 block (channels 32 wc.., pixels 32 wp..): per step 16 v_mfma_f32_32x32x2_f32
//             (exact fp32 products, fp32 sums), lane (i, h) feeding Wt[32 wc + i][2 u + h] and G[2 u + h][32 wp + i];
//   zeros     pixels past the phase's count, taps whose (oh, ow) falls outside the top, channels past Cg, columns past
//             Kp and elements masked by ReLU are staged as zeros by select, never as 0 x a loaded value (the matrix's
//             padding -- channels past Cg, columns past Kp -- is stored zeros, and is not read / meets a selected zero);
//   epilogue  the accumulators go to bottom_diff[n][c][stride_h*hh + h0][stride_w*ww + w0] with plain vector stores; images
//             at or past n_images are not touched.
// The order of an element's sum -- live steps ascending, within a step the MFMA's own fixed order over its columns -- is a
// function of the geometry and the pattern only: not of n_images, not of the image's place in the batch.
// The work is the dense problem restricted to live blocks: a pruned position inside a live block contributes 0 x G.  A
// non-finite G there gives NaN where the gather kernel (which never reads it for that channel) gives a finite value; the
// forward's DENSE kernel has the same property.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "align_rules.h"
#include "escoin_plan.h"

namespace escoin {

typedef float dgm_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kDgmThreads = 256;
constexpr int kDgmSlots = kDgmThreads / kDgmTileP;             // 4: columns a pass of the workgroup stages
constexpr int kDgmPerThread = kDgmStepK / kDgmSlots;           // 8 elements of each block per thread and step
constexpr int kDgmTileFloats = kDgmStepK * kDgmLdsRow;
static_assert(kDgmTileC == 64 && kDgmTileP == 64 && kDgmStepK == 32, "the wave layout below is 2 x 2 blocks of 32 x 32");
static_assert(sizeof(float) * 4 * kDgmTileFloats == kDgmLdsBytes, "align_rules.h reports this kernel's LDS");

struct DgmArgs {
  const float *__restrict__ top_diff;
  const float *__restrict__ top;        // fuse_relu only
  float *__restrict__ bottom_diff;
  const float *__restrict__ mat;        // the phase matrices
  const int4 *__restrict__ col;         // [cols_total]: {G offset of ocl, dh, dw, valid}
  const int *__restrict__ phase;        // [phases][8]: {h0, w0, rows, cols, kp, ksteps, col0, ntaps}
  const int *__restrict__ live_ptr;     // [group * phases * ctiles + 1]
  const int *__restrict__ live;
  int n_images;
  int C, H, W, M, OH, OW;
  int stride_h, stride_w;
  int Cg, Mg, ctiles, phases, cols_total;
};

template <bool RELU>
__global__ void __launch_bounds__(kDgmThreads)
escoin_sconv_dgrad_mfma_kernel(DgmArgs a) {
  __shared__ float sW[2][kDgmTileFloats];
  __shared__ float sG[2][kDgmTileFloats];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ph = blockIdx.y;
  const int grp = blockIdx.z / a.ctiles, ct = blockIdx.z - grp * a.ctiles;
  const int *__restrict__ pt = a.phase + 8 * ph;
  const int h0 = pt[0], w0 = pt[1], cols = pt[3], col0 = pt[6];
  const int ppix = pt[2] * cols;                            // the phase's pixels per image
  const long total = (long)a.n_images * ppix;               // (N*H*W < 2^31: dgm_plan)
  const long p0 = (long)blockIdx.x * kDgmTileP;
  if (p0 >= total) return;                                  // (the whole workgroup: before any barrier)
  const int list = (grp * a.phases + ph) * a.ctiles + ct;
  const int lb = a.live_ptr[list], nlive = a.live_ptr[list + 1] - lb;
  const int c0 = ct * kDgmTileC;
  const int opix = a.OH * a.OW;

  // staging role: pixel / channel `lane` of the tile, columns wave + 4 j of the step
  const long p = p0 + lane;
  const bool plive = p < total;
  const int n = plive ? (int)(p / ppix) : 0, r = plive ? (int)(p - (long)n * ppix) : 0;
  const int hh = r / cols, ww = r - hh * cols;
  const float *__restrict__ gimg = a.top_diff + ((size_t)n * a.M + (size_t)grp * a.Mg) * opix;
  const float *__restrict__ timg = RELU ? a.top + ((size_t)n * a.M + (size_t)grp * a.Mg) * opix : nullptr;
  const bool clive = c0 + lane < a.Cg;
  const float *__restrict__ wblk = a.mat + (((size_t)grp * a.ctiles + ct) * a.cols_total + col0) * kDgmTileC + lane;
  float wv[kDgmPerThread], gv[kDgmPerThread];
  auto load = [&](int s) {
    const int kb = s * kDgmStepK + wave;
#pragma unroll
    for (int j = 0; j < kDgmPerThread; ++j) {
      const int k = kb + kDgmSlots * j;
      const int4 t = a.col[col0 + k];                       // (the table covers whole steps)
      const int oh = hh + t.y, ow = ww + t.z;
      float g = 0.f;
      if (plive && t.w && (unsigned)oh < (unsigned)a.OH && (unsigned)ow < (unsigned)a.OW) {
        const int at = t.x + oh * a.OW + ow;                // (Mg*OH*OW < 2^31: dgm_plan)
        g = gimg[at];
        if (RELU && !(timg[at] > 0.f)) g = 0.f;
      }
      gv[j] = g;
      wv[j] = clive ? wblk[(size_t)k * kDgmTileC] : 0.f;
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int j = 0; j < kDgmPerThread; ++j) {
      sW[buf][(wave + kDgmSlots * j) * kDgmLdsRow + lane] = wv[j];
      sG[buf][(wave + kDgmSlots * j) * kDgmLdsRow + lane] = gv[j];
    }
  };

  const int wc = wave >> 1, wp = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  dgm_f32x16 acc = {0};
  if (nlive > 0) load(a.live[lb]);
  for (int i = 0; i < nlive; ++i) {
    const int buf = i & 1;
    store(buf);
    // everyone's part of step i is in buf -- and everyone is past the multiply of step i - 1, which read the other buffer
    __syncthreads();
    if (i + 1 < nlive) load(a.live[lb + i + 1]);
    const float *wa = &sW[buf][lh * kDgmLdsRow + wc * 32 + li];
    const float *ga = &sG[buf][lh * kDgmLdsRow + wp * 32 + li];
#pragma unroll
    for (int u = 0; u < kDgmStepK / 2; ++u)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[2 * u * kDgmLdsRow], ga[2 * u * kDgmLdsRow], acc, 0, 0, 0);
  }

  // C/D layout of the 32 x 32 block: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
  const long pe = p0 + wp * 32 + li;
  if (pe >= total) return;
  const int ne = (int)(pe / ppix), re = (int)(pe - (long)ne * ppix);
  const int he = re / cols, we = re - he * cols;
  const size_t plane = (size_t)a.H * a.W;
  float *__restrict__ out = a.bottom_diff + ((size_t)ne * a.C + (size_t)grp * a.Cg + c0) * plane +
                            (size_t)(h0 + a.stride_h * he) * a.W + (w0 + a.stride_w * we);
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int c = wc * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
    if (c0 + c < a.Cg) out[(size_t)c * plane] = acc[reg];
  }
}

int dgm_build(const escoin_plan *p, const DgmPlan &dp, DgmState *m, hipStream_t stream) {
  DgmTables t = dgrad_mfma_tables(csr_view(p), dp);
  std::vector<float> mat((size_t)std::max<long>(dp.mat_floats, 1), 0.f);
  const std::vector<float> flat = flat_entries(p->values);
  for (size_t e = 0; e < flat.size(); ++e) {
    if ((long)t.pos[e] < 0 || (long)t.pos[e] >= dp.mat_floats) return fail(ESCOIN_EINVAL, "backward_kernel: an entry's place lies outside the phase matrices");
    mat[(size_t)t.pos[e]] = flat[e];
  }
  m->phases = dp.phases_h * dp.phases_w;
  m->ctiles = dp.ctiles;
  m->cols_total = (int)dp.cols_total;
  m->lds_bytes = dp.lds_bytes;
  m->ppix.resize(dp.phase.size());
  for (size_t k = 0; k < dp.phase.size(); ++k) m->ppix[k] = dp.phase[k].rows * dp.phase[k].cols;
  ESCOIN_HIP_TRY(m->mat.upload(mat, stream));
  ESCOIN_HIP_TRY(m->phase.upload(t.phase, stream));
  ESCOIN_HIP_TRY(m->col.upload(t.col, stream));
  ESCOIN_HIP_TRY(m->lptr.upload(t.live_ptr, stream));
  ESCOIN_HIP_TRY(m->live.upload(t.live, stream));
  ESCOIN_HIP_TRY(hipStreamSynchronize(stream));   // host vectors die at scope exit
  t.pos.resize(flat.size());
  m->pos = std::move(t.pos);
  return ESCOIN_OK;
}

int launch_dgrad_mfma(const escoin_plan *p, const DgmState &m, const float *top, const float *top_diff,
                      float *bottom_diff, int n_images, hipStream_t stream) {
  const Geometry &g = p->g;
  const escoin_conv_desc &d = g.d;
  if (!m.mat.get<void>() || !m.phase.get<void>() || !m.col.get<void>() || !m.lptr.get<void>() || !m.live.get<void>())
    return fail(ESCOIN_ESTATE, "MFMA data-gradient kernel: the backward state has no tables for it");
  long tiles = 0;
  for (const int ppix : m.ppix) tiles = std::max(tiles, ((long)n_images * ppix + kDgmTileP - 1) / kDgmTileP);
  if (tiles == 0) return ESCOIN_OK;                        // nothing to write: no launch
  DgmArgs a;
  a.top_diff = top_diff; a.top = top; a.bottom_diff = bottom_diff;
  a.mat = m.mat.get<const float>(); a.col = m.col.get<const int4>(); a.phase = m.phase.get<const int>();
  a.live_ptr = m.lptr.get<const int>(); a.live = m.live.get<const int>();
  a.n_images = n_images;
  a.C = d.C; a.H = d.H; a.W = d.W; a.M = d.M; a.OH = g.OH; a.OW = g.OW;
  a.stride_h = d.stride_h; a.stride_w = d.stride_w;
  a.Cg = g.Cg; a.Mg = g.Mg; a.ctiles = m.ctiles; a.phases = m.phases; a.cols_total = m.cols_total;
  const dim3 grid((unsigned)tiles, (unsigned)m.phases, (unsigned)(d.group * m.ctiles)), block(kDgmThreads);
  if (d.fuse_relu) hipLaunchKernelGGL(escoin_sconv_dgrad_mfma_kernel<true>, grid, block, 0, stream, a);
  else hipLaunchKernelGGL(escoin_sconv_dgrad_mfma_kernel<false>, grid, block, 0, stream, a);
  ESCOIN_HIP_TRY(hipGetLastError());
  return ESCOIN_OK;
}

}  // namespace escoin
