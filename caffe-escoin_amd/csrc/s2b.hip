// s2b.hip -- the two rearrangements of plan option "s2b" (include/escoin.h "Space-to-batch"): a dilated stride-1 layer runs
// on the stride-1, dilation-1 kernels as a convolution of N * P images, each one residue class modulo (eh, ew) of the padded
// bottom.  Both kernels serve both directions; a launch names a SPREAD image of Hs x Ws (the bottom, bottom_diff, the top
// or top_diff), its offset in the padded frame (the pad for the bottom side, 0 for the top side) and the CLASS images of
// Hd x Wd (H' x W' or OH' x OW'), with padded position (hp, wp) = (i * eh + qh, j * ew + qw) and n' = (n * eh + qh) * ew + qw:
//   escoin_s2b_pack_kernel     class[n'][ch][i][j] = spread[n][ch][hp - off_h][wp - off_w] inside the spread image, +0
//                              outside (the pad, and the rows and columns of short classes past it); with a mask (the top
//                              blob, laid out as the spread image) the value is mask > 0 ? spread : 0 -- the expression
//                              that builds BwdState::g on the transposed path.  X' before the inner forward, G' before the
//                              inner data gradient.
//   escoin_s2b_unpack_kernel   spread[n][ch][h][w] = class[n'][ch][hp / eh][wp / ew], (hp, wp) = (h + off_h, w + off_w),
//                              every index inside the class image; optionally through v > 0 ? v : 0, the epilogues' ReLU.
//                              The top after the inner forward, bottom_diff after the inner data gradient.
// Both are one pass with one store per destination element, zeros included: no memset launch, no atomics, no workgroup
// waits for another.  The work is whole ROWS of the spread side, whose rows are the long contiguous ones (a class row is
// 1 / ew of one): pack walks the PADDED rows (hp, lane = padded column wp:
// consecutive reads of the spread row, and the ew classes of a row stored as ew runs of floats at stride 1), unpack walks
// the spread rows (consecutive stores; the reads gather the ew class rows).  A row gets the smallest power of two of lanes
// that covers it, up to a wave (s2d.hip's scheme; S2dDiv and s2d_lane_shift are align_rules.h's).  Every offset is a 32-bit
// one: align_rules.h s2b_plan refuses a layer whose bottom, top, X' or T' reaches 2^31 elements, and a row holds at least
// one element of the side it walks, so every row and workgroup count stays below 2^31.  Images at or past n_images are
// neither read nor written.
#include <hip/hip_runtime.h>

#include "escoin_plan.h"

namespace escoin {

struct S2bArgs {
  const float *src;
  const float *mask;        // pack: null, or the blob whose sign gates src
  float *dst;
  unsigned CH;              // planes per image: C (bottom side) or M (top side)
  unsigned Hs, Ws;          // the spread image
  unsigned Hd, Wd;          // a class image
  unsigned eh, ew, off_h, off_w;
  unsigned rows;            // rows of one (image, plane) a launch walks: pack Hd * eh, unpack Hs
  unsigned total_rows;      // n_images * CH * rows
  unsigned span;            // lanes' range along a row: pack Wd * ew, unpack Ws
  unsigned lane_shift;      // log2 of the lanes per row
  S2dDiv by_rows, by_ch, by_eh, by_ew;
};

constexpr int kS2bWaves = 4, kS2bPasses = 2;

// The row a lane works on in pass `pass` (>= total_rows: none), its first column and its step.
__device__ inline unsigned s2b_row(const S2bArgs &a, int pass, unsigned *col, unsigned *step) {
  const unsigned per_wave = 64u >> a.lane_shift;
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  *step = 1u << a.lane_shift;
  *col = lane & (*step - 1u);
  return ((blockIdx.x * kS2bPasses + (unsigned)pass) * kS2bWaves + wave) * per_wave + (lane >> a.lane_shift);
}

// Plane (n', ch) of the class images, in planes: row R's plane np = n * CH + ch and its class row qh.
__device__ inline unsigned s2b_class_plane0(const S2bArgs &a, unsigned np, unsigned qh) {
  const unsigned n = s2d_div(np, a.by_ch), ch = np - n * a.CH;
  return ((n * a.eh + qh) * a.ew) * a.CH + ch;           // class column qw adds qw * CH
}

template <bool MASK>
__global__ void __launch_bounds__(64 * kS2bWaves) escoin_s2b_pack_kernel(S2bArgs a) {
#pragma unroll
  for (int pass = 0; pass < kS2bPasses; ++pass) {
    unsigned col, step;
    const unsigned R = s2b_row(a, pass, &col, &step);
    if (R >= a.total_rows) continue;
    const unsigned np = s2d_div(R, a.by_rows), hp = R - np * a.rows;
    const unsigned i = s2d_div(hp, a.by_eh), qh = hp - i * a.eh;
    const int h = (int)hp - (int)a.off_h;
    const bool row_in = (unsigned)h < a.Hs;
    const unsigned sbase = (np * a.Hs + (row_in ? (unsigned)h : 0u)) * a.Ws;
    const unsigned plane0 = s2b_class_plane0(a, np, qh);
    for (unsigned wp = col; wp < a.span; wp += step) {
      const unsigned j = s2d_div(wp, a.by_ew), qw = wp - j * a.ew;
      const int w = (int)wp - (int)a.off_w;
      float v = 0.f;
      if (row_in && (unsigned)w < a.Ws) {
        v = a.src[sbase + (unsigned)w];
        if (MASK) v = a.mask[sbase + (unsigned)w] > 0.f ? v : 0.f;
      }
      a.dst[((plane0 + qw * a.CH) * a.Hd + i) * a.Wd + j] = v;
    }
  }
}

template <bool RELU>
__global__ void __launch_bounds__(64 * kS2bWaves) escoin_s2b_unpack_kernel(S2bArgs a) {
#pragma unroll
  for (int pass = 0; pass < kS2bPasses; ++pass) {
    unsigned col, step;
    const unsigned R = s2b_row(a, pass, &col, &step);
    if (R >= a.total_rows) continue;
    const unsigned np = s2d_div(R, a.by_rows), h = R - np * a.rows;
    const unsigned hp = h + a.off_h;
    const unsigned i = s2d_div(hp, a.by_eh), qh = hp - i * a.eh;       // i < Hd: hp < Hs + off_h <= Hd * eh
    const unsigned plane0 = s2b_class_plane0(a, np, qh);
    float *__restrict__ drow = a.dst + R * a.Ws;
    for (unsigned w = col; w < a.span; w += step) {
      const unsigned wp = w + a.off_w;
      const unsigned j = s2d_div(wp, a.by_ew), qw = wp - j * a.ew;     // j < Wd likewise
      float v = a.src[((plane0 + qw * a.CH) * a.Hd + i) * a.Wd + j];
      if (RELU) v = v > 0.f ? v : 0.f;
      drow[w] = v;
    }
  }
}

static int s2b_launch(const escoin_plan *p, const float *src, const float *mask, float *dst, bool pack, bool top_side, bool relu,
                      int n_images, hipStream_t stream) {
  const Geometry &g = p->g;
  const escoin_conv_desc &d = g.d;
  const S2bPlan &sp = p->s2b_state->sp;
  S2bArgs a;
  a.src = src; a.mask = mask; a.dst = dst;
  a.eh = sp.eh; a.ew = sp.ew;
  if (top_side) {
    a.CH = d.M; a.Hs = g.OH; a.Ws = g.OW; a.off_h = a.off_w = 0;
    a.Hd = sp.inner.H - d.KH + 1; a.Wd = sp.inner.W - d.KW + 1;
  } else {
    a.CH = d.C; a.Hs = d.H; a.Ws = d.W; a.off_h = d.pad_h; a.off_w = d.pad_w;
    a.Hd = sp.inner.H; a.Wd = sp.inner.W;
  }
  // (the class images cover the spread image at its offset: the kernels' indices stay inside both sides)
  if ((long)a.Hd * a.eh < (long)a.Hs + a.off_h || (long)a.Wd * a.ew < (long)a.Ws + a.off_w)
    return fail(ESCOIN_EINVAL, "s2b: the class images do not cover the image");
  a.rows = pack ? a.Hd * a.eh : a.Hs;
  a.span = pack ? a.Wd * a.ew : a.Ws;
  // (below 2^31: s2b_plan bounds all four blobs, and a row holds at least one element of the side it walks)
  const long total = (long)n_images * a.CH * a.rows;
  if (total <= 0 || total > 0x7fffffffL || (long)total * a.span > 0x7fffffffL) return fail(ESCOIN_EINVAL, "s2b: row count out of range");
  a.total_rows = (unsigned)total;
  a.lane_shift = s2d_lane_shift(a.span);
  a.by_rows = s2d_div_make(a.rows), a.by_ch = s2d_div_make(a.CH), a.by_eh = s2d_div_make(a.eh), a.by_ew = s2d_div_make(a.ew);
  const long per_wg = (long)kS2bPasses * kS2bWaves * (64 >> a.lane_shift);
  const dim3 grid((unsigned)((total + per_wg - 1) / per_wg)), block(64 * kS2bWaves);
  if (pack) hipLaunchKernelGGL(mask ? escoin_s2b_pack_kernel<true> : escoin_s2b_pack_kernel<false>, grid, block, 0, stream, a);
  else hipLaunchKernelGGL(relu ? escoin_s2b_unpack_kernel<true> : escoin_s2b_unpack_kernel<false>, grid, block, 0, stream, a);
  ESCOIN_HIP_TRY(hipGetLastError());
  return ESCOIN_OK;
}

static int launch_s2b_pack(const escoin_plan *p, const float *src, const float *mask, float *dst, bool top_side, int n_images,
                           hipStream_t stream) {
  return s2b_launch(p, src, mask, dst, true, top_side, false, n_images, stream);
}

static int launch_s2b_unpack(const escoin_plan *p, const float *src, float *dst, bool top_side, bool relu, int n_images,
                             hipStream_t stream) {
  return s2b_launch(p, src, nullptr, dst, false, top_side, relu, n_images, stream);
}

// (the plan's core -- escoin_capi.hip, sconv_backward.hip -- reaches these through g_s2b_hooks: escoin_plan.h)
namespace {
__attribute__((used)) const bool g_registered =
    (g_s2b_hooks = S2bHooks{launch_s2b_pack, launch_s2b_unpack, "escoin_s2b_pack_kernel", "escoin_s2b_unpack_kernel"}, true);
}  // namespace

}  // namespace escoin
