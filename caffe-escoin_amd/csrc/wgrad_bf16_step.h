// wgrad_bf16_step.h -- the step loop of the bf16 math mode of the MFMA weight-gradient kernels (plan option "wgrad_math" =
// ESCOIN_MATH_BF16; wgrad_bf16.hip: the sparse-position kernel and the dense one, thin bodies around this loop as the fp32
// kernels are around wgrad_mfma_step.h).  Device code only; the tile constants are align_rules.h's.
//   wgb_tile_sum<RELU, GV, XV>(in, sG, sX, grp, m0, k0, q0, live) = the 64 x 64 tile (rows m0.. of conv group grp, columns
//   k0..) of bf16(G)[Mg x P] * bf16(im2col(bottom))[P x Kd] summed in fp32 over the `live` pixels from flattened
//   (n, oh, ow) pixel q0 on, as the calling wave's 32 x 32 block in the matrix instruction's C/D layout (wgm_out_row /
//   wgm_out_col of wgrad_mfma_step.h).  Called by all 256 threads of the workgroup with the same arguments.
//   steps     kWgbStepPixels = 64 pixels, one barrier each, two LDS buffers: the global loads of step s + 1 go out to
//             registers before the matrix instructions of step s and are converted and written to the other buffer at the
//             top of the next iteration.
//   staging   thread t owns the quad of pixels 4 (t % 16) .. + 3 of the step for rows / columns t / 16 + 16 j (j < 4) of
//             both tiles: a wave's 64 lanes are 4 rows x 16 quads, 4 runs of 256 contiguous bytes wherever the operand is
//             contiguous along the pixels.  The reduction axis IS the pixel axis, so a quad is 4 consecutive k of one row:
//             masked by the ReLU, rounded to bf16 (nearest even, NaN stays NaN: v_cvt_pk_bf16_f32) and written by ONE
//             8-byte LDS store into the k-contiguous tile [row][64 pixels].
//   GV        G's quad by one 16-byte load.  Needs OH*OW % 4 == 0 (q0 is a multiple of 1024, so the quad starts at a
//             multiple of 4 inside one image's row of OH*OW floats and ends inside it; the batch's pixel count is a multiple
//             of 4 too, so the quad is wholly live or wholly dead) and 16-byte aligned top_diff (and top, where it is read).
//             Otherwise four 4-byte loads, each pixel decoded by itself: a quad may straddle two images and the live end.
//   XV        the bottom's quad by one 16-byte load: on top of GV's terms a 1x1, stride-1, pad-0 layer (column k is channel
//             k, the output pixel is the input pixel) and a 16-byte aligned bottom.  Otherwise gathered through ktab with
//             the border test, per pixel, as in the fp32 loop.
//             Both variants stage the same values at the same LDS places: the staging path does not enter the sum.
//   multiply  wave (wm, wk) owns the 32 x 32 block (rows 32 wm.., columns 32 wk..): per step 4 v_mfma_f32_32x32x16_bf16
//             (exact products of the rounded operands, fp32 sums); in instruction u lane (i, h) feeds
//             G[32 wm + i][16 u + 8 h .. + 7] and X[16 u + 8 h .. + 7][32 wk + i], one 16-byte LDS read each.
//   zeros     pixels at or past q0 + live, taps outside the image, rows past Mg and columns past Kd are staged as zeros by
//             select (never 0 x a loaded value), so a non-finite bottom element reaches only the columns whose tap reads
//             it and a non-finite G only its own row; steps wholly past the last live pixel are not run.
// The order of an element's sum: steps ascending from q0, within a step instructions u = 0..3, within an instruction its own
// fixed order over its 16 pixels.
//
// LDS: a tile is 64 rows of 64 bf16 = 128 bytes = 8 chunks of 16 bytes; chunk c of row r sits in slot c ^ ((r >> 1) & 7) of
// the row (dense_bf16.hip's swizzle on rows of the same length); no padding: 2 buffers x 2 tiles x 8 KiB = kWgbLdsBytes.
// With 64 banks of 4 bytes a row covers half the banks, even rows banks 0..31, odd rows banks 32..63.
//   fragment read (16 bytes per lane, 16 lanes = 256 bytes per pass): 16 consecutive rows from a multiple of 16 at one
//     logical chunk are 8 even and 8 odd rows, and within either parity (r >> 1) & 7 takes its 8 values once: 8 different
//     slots of 4 banks in each bank half -- every bank once;
//   staging store (8 bytes per lane, 32 lanes = 256 bytes per pass): lanes 0..15 of a pass write the 16 quads of row r --
//     the row's 8 chunks in some order, both halves of each: its 32 banks once -- and lanes 16..31 those of row r + 1, the
//     other bank half.
// So both are free of bank conflicts by construction (under the pass sizes named; not measured).
#ifndef ESCOIN_WGRAD_BF16_STEP_H_
#define ESCOIN_WGRAD_BF16_STEP_H_

#include <hip/hip_runtime.h>

#include "align_rules.h"
#include "wgrad_mfma_step.h"

namespace escoin {

typedef __bf16 wgb_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 wgb_bf16x4 __attribute__((ext_vector_type(4)));
typedef float wgb_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWgbQuads = kWgbStepPixels / 4;                  // 16 quads per step
constexpr int kWgbSlots = kWgmThreads / kWgbQuads;             // 16 rows / columns a pass of the workgroup stages
constexpr int kWgbPerThread = kWgmTileM / kWgbSlots;           // 4 rows and 4 columns per thread and step
constexpr int kWgbRowChunks = kWgbStepPixels / 8;              // 16-byte chunks per LDS row
constexpr int kWgbTileChunks = kWgmTileM * kWgbRowChunks;      // chunks per tile
static_assert(kWgmTileM == 64 && kWgmTileK == 64 && kWgbStepPixels == 64 && kWgbRowChunks == 8,
              "the staging map and the swizzle are written for 64 x 64 tiles and steps of 64 pixels");
static_assert(sizeof(wgb_bf16x8) * 4 * kWgbTileChunks == kWgbLdsBytes, "align_rules.h reports these kernels' LDS");
static_assert(kBwdChunkPixels % kWgbStepPixels == 0, "a chunk is whole steps");

// index, in 8-byte halves of a chunk, of pixels 4 quad .. + 3 of row `row`; and in chunks, of logical chunk `chunk`
__device__ __forceinline__ int wgb_quad_at(int row, int quad) {
  return row * (2 * kWgbRowChunks) + (((quad >> 1) ^ ((row >> 1) & 7)) << 1) + (quad & 1);
}
__device__ __forceinline__ int wgb_chunk_at(int row, int chunk) { return row * kWgbRowChunks + (chunk ^ ((row >> 1) & 7)); }

template <bool RELU, bool GV, bool XV>
__device__ __forceinline__ wgm_f32x16 wgb_tile_sum(const WgmIn &a, wgb_bf16x8 (*sG)[kWgbTileChunks], wgb_bf16x8 (*sX)[kWgbTileChunks],
                                                   int grp, int m0, int k0, long q0, int live) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int opix = a.OH * a.OW;
  const size_t plane = (size_t)a.H * a.W;
  const int nsteps = (live + kWgbStepPixels - 1) / kWgbStepPixels;

  // staging role: quad sq of the step, rows m0 + sr + 16 j of G, columns k0 + sr + 16 j of X
  const int sq = tid & (kWgbQuads - 1), sr = tid / kWgbQuads;
  int xoff[kWgbPerThread], xdy[kWgbPerThread], xdx[kWgbPerThread];
  unsigned kvalid = 0;
#pragma unroll
  for (int j = 0; j < kWgbPerThread; ++j) {
    const int4 t = a.ktab[k0 + sr + kWgbSlots * j];     // (the table covers whole tiles)
    xoff[j] = t.x; xdy[j] = t.y; xdx[j] = t.z;
    kvalid |= t.w ? (1u << j) : 0u;
  }
  wgb_f32x4 gv[kWgbPerThread], xv[kWgbPerThread];
  auto load = [&](int s) {
    const int ql = s * kWgbStepPixels + 4 * sq;         // the quad's first pixel, counted from q0
    // the quad's pixels e = 0..3: image, pixel inside the image, output row and column (dead pixels: pixel 0 of image 0)
    int pn[4], pr[4], poh[4], pow_[4];
    bool pl[4];
    {
      const bool l0 = ql < live;
      const int q = l0 ? (int)(q0 + ql) : 0;            // (N*OH*OW < 2^31: wgm_plan)
      int n = q / opix, r = q - n * opix;
      int oh = 0, ow = 0;
      if (!XV) { oh = r / a.OW; ow = r - oh * a.OW; }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        pl[e] = ql + e < live;
        pn[e] = pl[e] ? n : 0; pr[e] = pl[e] ? r : 0; poh[e] = pl[e] ? oh : 0; pow_[e] = pl[e] ? ow : 0;
        if ((GV && XV) || e == 3) continue;             // (16-byte loads read the first pixel's place alone)
        if (++r == opix) { r = 0; ++n; }
        if (!XV && ++ow == a.OW) { ow = 0; if (++oh == a.OH) oh = 0; }
      }
    }
    // ---- G ----
    const size_t gi = ((size_t)pn[0] * a.M + (size_t)grp * a.Mg + m0 + sr) * opix + pr[0];
#pragma unroll
    for (int j = 0; j < kWgbPerThread; ++j) {
      wgb_f32x4 g = {0.f, 0.f, 0.f, 0.f};
      if (m0 + sr + kWgbSlots * j < a.Mg) {
        if (GV) {
          if (pl[0]) {
            const size_t at = gi + (size_t)(kWgbSlots * j) * opix;
            g = *reinterpret_cast<const wgb_f32x4 *>(a.top_diff + at);
            if (RELU) {
              const wgb_f32x4 t = *reinterpret_cast<const wgb_f32x4 *>(a.top + at);
#pragma unroll
              for (int e = 0; e < 4; ++e) g[e] = t[e] > 0.f ? g[e] : 0.f;
            }
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (!pl[e]) continue;
            const size_t at = ((size_t)pn[e] * a.M + (size_t)grp * a.Mg + m0 + sr + kWgbSlots * j) * opix + pr[e];
            float v = a.top_diff[at];
            if (RELU && !(a.top[at] > 0.f)) v = 0.f;
            g[e] = v;
          }
        }
      }
      gv[j] = g;
    }
    // ---- X ----
    if (XV) {
      // pointwise, stride 1, pad 0: column k0 + c is channel k0 + c of the group, the output pixel is the input pixel
      const size_t xi = ((size_t)pn[0] * a.C + (size_t)grp * a.Cg + k0 + sr) * plane + pr[0];
#pragma unroll
      for (int j = 0; j < kWgbPerThread; ++j) {
        wgb_f32x4 x = {0.f, 0.f, 0.f, 0.f};
        if (pl[0] && ((kvalid >> j) & 1u)) x = *reinterpret_cast<const wgb_f32x4 *>(a.bottom + xi + (size_t)(kWgbSlots * j) * plane);
        xv[j] = x;
      }
    } else {
#pragma unroll
      for (int j = 0; j < kWgbPerThread; ++j) xv[j] = wgb_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ih0 = poh[e] * a.stride_h - a.pad_h, iw0 = pow_[e] * a.stride_w - a.pad_w;
        const float *__restrict__ xb = a.bottom + ((size_t)pn[e] * a.C + (size_t)grp * a.Cg) * plane;
        const long xorg = (long)ih0 * a.W + iw0;
#pragma unroll
        for (int j = 0; j < kWgbPerThread; ++j) {
          const int ih = ih0 + xdy[j], iw = iw0 + xdx[j];
          if (pl[e] && ((kvalid >> j) & 1u) && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W)
            xv[j][e] = xb[xorg + xoff[j]];
        }
      }
    }
  };
  auto store = [&](int buf) {
    wgb_bf16x4 *tg = reinterpret_cast<wgb_bf16x4 *>(&sG[buf][0]);
    wgb_bf16x4 *tx = reinterpret_cast<wgb_bf16x4 *>(&sX[buf][0]);
#pragma unroll
    for (int j = 0; j < kWgbPerThread; ++j) {
      const int at = wgb_quad_at(sr + kWgbSlots * j, sq);
      tg[at] = __builtin_convertvector(gv[j], wgb_bf16x4);      // two v_cvt_pk_bf16_f32: nearest even, overflow to infinity
      tx[at] = __builtin_convertvector(xv[j], wgb_bf16x4);
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
    wgb_bf16x8 fg[kWgbStepPixels / 16], fx[kWgbStepPixels / 16];
#pragma unroll
    for (int u = 0; u < kWgbStepPixels / 16; ++u) {
      fg[u] = sG[buf][wgb_chunk_at(wm * 32 + li, 2 * u + lh)];
      fx[u] = sX[buf][wgb_chunk_at(wk * 32 + li, 2 * u + lh)];
    }
#pragma unroll
    for (int u = 0; u < kWgbStepPixels / 16; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fg[u], fx[u], acc, 0, 0, 0);
  }
  return acc;
}

}  // namespace escoin
#endif  // ESCOIN_WGRAD_BF16_STEP_H_
