// s2d.hip -- the two rearrangements of plan option "s2d" (include/escoin.h "Space-to-depth"): a strided layer runs on the
// stride-1 kernels as a convolution of X', the padded bottom split into its stride phases with each phase a channel.
//   escoin_s2d_pack_kernel     X'[n][c'][i][j] = bottom[n][c][i * stride_h + ph - pad_h][j * stride_w + pw - pad_w], +0
//                              outside the image, c' = (c * PH + ph) * PW + pw -- before the inner forward
//   escoin_s2d_unpack_kernel   bottom_diff[n][c][h][w] = dX'[n][c'(c, hp % stride_h, wp % stride_w)][hp / stride_h]
//                              [wp / stride_w], hp = h + pad_h, wp = w + pad_w, +0 where the phase owns no tap or the
//                              index lies past the inner image -- after the inner data gradient
// Both are one pass with one store per destination element, zeros included: no memset launch, no atomics, no workgroup
// waits for another.  The work is whole ROWS of the side that is contiguous in memory, numbered through all images and
// channels: pack walks BOTTOM rows (a row (i, ph) of X''s PW phase rows; lane = padded column: each bottom element is
// read at most once, the PW phases of a row are stored as PW runs of consecutive floats), unpack walks BOTTOM_DIFF rows
// (consecutive stores; the reads gather the PW phase rows).  A row gets the smallest power of two of lanes that covers
// it, up to a wave, so that a 14-wide image fills a wave with four consecutive rows -- 256 contiguous bytes -- instead of
// a quarter of one; a workgroup of four waves takes two such passes.  Every offset is a 32-bit one: align_rules.h
// s2d_plan refuses a layer whose bottom or X' reaches 2^31 elements, and with them every row and workgroup count here
// stays below 2^31; the divisions by the launch's constants are multiplications (S2dDiv, checked on the host by
// tests/test_s2d_host.py).  Images at or past n_images are neither read nor written.
#include <hip/hip_runtime.h>

#include "escoin_plan.h"

namespace escoin {

struct S2dArgs {
  const float *src;
  float *dst;
  unsigned H, W;            // the bottom image
  unsigned Hi, Wi;          // the inner image H' x W'
  unsigned PH, PW;          // phases that own a tap
  unsigned sh, sw, pad_h, pad_w;
  unsigned rows;            // rows of one (image, channel) a launch walks: pack H' * PH, unpack H
  unsigned total_rows;      // n_images * C * rows
  unsigned span;            // lanes' range along a row: pack W' * stride_w (the padded columns X' covers), unpack W
  unsigned lane_shift;      // log2 of the lanes per row
  S2dDiv by_rows, by_ph, by_sh, by_sw;
};

constexpr int kS2dWaves = 4, kS2dPasses = 2;

// The row a lane works on in pass `pass` (>= total_rows: none) and its first column.
__device__ inline unsigned s2d_row(const S2dArgs &a, int pass, unsigned *col, unsigned *step) {
  const unsigned per_wave = 64u >> a.lane_shift;
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  *step = 1u << a.lane_shift;
  *col = lane & (*step - 1u);
  return ((blockIdx.x * kS2dPasses + (unsigned)pass) * kS2dWaves + wave) * per_wave + (lane >> a.lane_shift);
}

__global__ void __launch_bounds__(64 * kS2dWaves) escoin_s2d_pack_kernel(S2dArgs a) {
#pragma unroll
  for (int pass = 0; pass < kS2dPasses; ++pass) {
    unsigned col, step;
    const unsigned R = s2d_row(a, pass, &col, &step);
    if (R >= a.total_rows) continue;
    const unsigned nc = s2d_div(R, a.by_rows), r = R - nc * a.rows;     // row (i, ph), ph fastest: consecutive bottom rows
    const unsigned i = s2d_div(r, a.by_ph), ph = r - i * a.PH;
    const int h = (int)(i * a.sh + ph) - (int)a.pad_h;
    const bool row_in = (unsigned)h < a.H;
    const float *__restrict__ srow = a.src + (nc * a.H + (row_in ? (unsigned)h : 0u)) * a.W;
    const unsigned cbase = (nc * a.PH + ph) * a.PW;                    // channel c' of phase column 0
    for (unsigned wp = col; wp < a.span; wp += step) {
      const unsigned j = s2d_div(wp, a.by_sw), pw = wp - j * a.sw;
      if (pw >= a.PW) continue;                                        // (stride_w > KW: columns no tap reads)
      const int w = (int)wp - (int)a.pad_w;
      const float v = row_in && (unsigned)w < a.W ? srow[w] : 0.f;
      a.dst[((cbase + pw) * a.Hi + i) * a.Wi + j] = v;
    }
  }
}

__global__ void __launch_bounds__(64 * kS2dWaves) escoin_s2d_unpack_kernel(S2dArgs a) {
#pragma unroll
  for (int pass = 0; pass < kS2dPasses; ++pass) {
    unsigned col, step;
    const unsigned R = s2d_row(a, pass, &col, &step);
    if (R >= a.total_rows) continue;
    const unsigned nc = s2d_div(R, a.by_rows), h = R - nc * a.rows;
    const unsigned hp = h + a.pad_h;
    const unsigned i = s2d_div(hp, a.by_sh), ph = hp - i * a.sh;
    const bool row_live = ph < a.PH && i < a.Hi;                       // else: a row no window reads
    const unsigned cbase = (nc * a.PH + (row_live ? ph : 0u)) * a.PW;
    float *__restrict__ drow = a.dst + R * a.W;
    for (unsigned w = col; w < a.span; w += step) {
      const unsigned wp = w + a.pad_w;
      const unsigned j = s2d_div(wp, a.by_sw), pw = wp - j * a.sw;
      float v = 0.f;
      if (row_live && pw < a.PW && j < a.Wi) v = a.src[((cbase + pw) * a.Hi + i) * a.Wi + j];
      drow[w] = v;
    }
  }
}

static int s2d_launch(const escoin_plan *p, const float *src, float *dst, bool pack, int n_images, hipStream_t stream) {
  const escoin_conv_desc &d = p->g.d;
  const S2dPlan &sp = p->s2d_state->sp;
  S2dArgs a;
  a.src = src; a.dst = dst;
  a.H = d.H; a.W = d.W; a.Hi = sp.inner.H; a.Wi = sp.inner.W; a.PH = sp.PH; a.PW = sp.PW;
  a.sh = d.stride_h; a.sw = d.stride_w; a.pad_h = d.pad_h; a.pad_w = d.pad_w;
  a.rows = pack ? (unsigned)sp.inner.H * sp.PH : (unsigned)d.H;
  a.span = pack ? (unsigned)sp.inner.W * d.stride_w : (unsigned)d.W;
  // (below 2^31: s2d_plan bounds N * C' * H' * W' and N * C * H * W, and a row holds at least one element of either)
  const long total = (long)n_images * d.C * a.rows;
  if (total <= 0 || total > 0x7fffffffL || (long)a.span > 0x7fffffffL) return fail(ESCOIN_EINVAL, "s2d: row count out of range");
  a.total_rows = (unsigned)total;
  a.lane_shift = s2d_lane_shift(a.span);
  a.by_rows = s2d_div_make(a.rows), a.by_ph = s2d_div_make(a.PH), a.by_sh = s2d_div_make(a.sh), a.by_sw = s2d_div_make(a.sw);
  const long per_wg = (long)kS2dPasses * kS2dWaves * (64 >> a.lane_shift);
  const dim3 grid((unsigned)((total + per_wg - 1) / per_wg)), block(64 * kS2dWaves);
  if (pack) hipLaunchKernelGGL(escoin_s2d_pack_kernel, grid, block, 0, stream, a);
  else hipLaunchKernelGGL(escoin_s2d_unpack_kernel, grid, block, 0, stream, a);
  ESCOIN_HIP_TRY(hipGetLastError());
  return ESCOIN_OK;
}

static int launch_s2d_pack(const escoin_plan *p, const float *bottom, float *x, int n_images, hipStream_t stream) {
  return s2d_launch(p, bottom, x, true, n_images, stream);
}

static int launch_s2d_unpack(const escoin_plan *p, const float *dx, float *bottom_diff, int n_images, hipStream_t stream) {
  return s2d_launch(p, dx, bottom_diff, false, n_images, stream);
}

// (the plan's core -- escoin_capi.hip, sconv_backward.hip -- reaches these through g_s2d_hooks: escoin_plan.h)
namespace {
__attribute__((used)) const bool g_registered = (g_s2d_hooks = S2dHooks{launch_s2d_pack, launch_s2d_unpack, "escoin_s2d_pack_kernel"}, true);
}  // namespace

}  // namespace escoin
