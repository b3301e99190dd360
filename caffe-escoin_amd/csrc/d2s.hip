// d2s.hip -- the rearrangements of plan option "deconv" (include/escoin.h "Deconvolution"): a Deconvolution layer of stride
// (sh, sw) runs on the stride-1 kernels as a convolution of the bottom itself with P = sh * sw times the output channels,
// inner channel m' = (m * sh + ph) * sw + pw holding output phase (ph, pw) of channel m on the H' x W' inner image.
//   escoin_d2s_unpack_kernel   top[n][m][oh][ow] = T'[n][m'(m, hp % sh, wp % sw)][hp / sh][wp / sw] + bias[m], hp = oh + pad_h,
//                              wp = ow + pad_w, then v > 0 ? v : 0 on a fuse_relu plan -- after the inner forward.  The
//                              depth-to-space interleave, the crop by the pad, the bias and the ReLU in one pass.
//   escoin_d2s_pack_kernel     G'[n][m'][i][j] = top_diff[n][m][i * sh + ph - pad_h][j * sw + pw - pad_w] inside OH x OW
//                              (top > 0 ? that : 0 on a fuse_relu plan), +0 outside -- before the inner backward
// Both are one pass with one plain store per destination element, zeros included: no memset launch, no atomics.  The work is
// whole ROWS of the destination, numbered through all images and channels, by s2d.hip's scheme: a row gets the smallest
// power of two of lanes that covers it, up to a wave; a workgroup of four waves takes two such passes.  A wave's stores run
// along ow (unpack) and along j (pack): consecutive addresses.  Unpack's reads of a row come from the sw phase planes of
// one inner row, each a run of consecutive floats; every (hp / sh, wp / sw) lies inside H' x W' (hp <= sh * (H - 1) + KH - 1),
// so no read is masked.  Pack reads every sw-th element of one top_diff row; a lane outside OH x OW reads element 0 (which
// exists: a launch has n_images >= 1) and selects +0 -- no branch around a store.  Every offset is a 32-bit one:
// align_rules.h d2s_plan refuses a layer whose top or T' reaches 2^31 elements, and every row count, hp and wp is below
// them; the divisions by the launch's constants are multiplications (S2dDiv).  Images at or past n_images are neither read
// nor written.
// The three small kernels of the backward's tail: escoin_d2s_carry_kernel adds the inner plan's compact weight gradient to
// the caller's values_diff (through the entry map) or weight_diff (through the entries' positions in blobs_[0]) -- the map is
// injective, one lane per entry, no atomics; escoin_d2s_bias_sum_kernel adds the P inner bias gradients of an output channel,
// in ascending phase order, one lane per channel.
#include <hip/hip_runtime.h>

#include "escoin_plan.h"

namespace escoin {

struct D2sArgs {
  const float *src;
  const float *aux;         // unpack: the bias [M] (BIAS); pack: the top blob whose sign gates src (RELU)
  float *dst;
  unsigned OH, OW;          // the top image
  unsigned Hi, Wi;          // the inner image H' x W'
  unsigned M, P;            // output channels, phases per channel
  unsigned sh, sw, pad_h, pad_w;
  unsigned rows;            // rows of one plane a launch walks: unpack OH (planes: n_images * M), pack H' (planes: n_images * M * P)
  unsigned total_rows;
  unsigned span;            // elements of a row: unpack OW, pack W'
  unsigned lane_shift;      // log2 of the lanes per row
  S2dDiv by_rows, by_sh, by_sw, by_M, by_P;
};

constexpr int kD2sWaves = 4, kD2sPasses = 2;

// The row a lane works on in pass `pass` (>= total_rows: none), its first column and its step along the row.
__device__ inline unsigned d2s_row(const D2sArgs &a, int pass, unsigned *col, unsigned *step) {
  const unsigned per_wave = 64u >> a.lane_shift;
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  *step = 1u << a.lane_shift;
  *col = lane & (*step - 1u);
  return ((blockIdx.x * kD2sPasses + (unsigned)pass) * kD2sWaves + wave) * per_wave + (lane >> a.lane_shift);
}

template <bool RELU, bool BIAS>
__global__ void __launch_bounds__(64 * kD2sWaves) escoin_d2s_unpack_kernel(D2sArgs a) {
#pragma unroll
  for (int pass = 0; pass < kD2sPasses; ++pass) {
    unsigned col, step;
    const unsigned R = d2s_row(a, pass, &col, &step);
    if (R >= a.total_rows) continue;
    const unsigned nm = s2d_div(R, a.by_rows), oh = R - nm * a.rows;     // plane (n, m), top row oh
    const unsigned hp = oh + a.pad_h;
    const unsigned i = s2d_div(hp, a.by_sh), ph = hp - i * a.sh;
    const unsigned cbase = nm * a.P + ph * a.sw;                         // inner plane of phase column 0
    float b = 0.f;
    if (BIAS) b = a.aux[nm - s2d_div(nm, a.by_M) * a.M];
    float *__restrict__ drow = a.dst + R * a.OW;
    for (unsigned ow = col; ow < a.span; ow += step) {
      const unsigned wp = ow + a.pad_w;
      const unsigned j = s2d_div(wp, a.by_sw), pw = wp - j * a.sw;
      float v = a.src[((cbase + pw) * a.Hi + i) * a.Wi + j];
      if (BIAS) v += b;
      if (RELU) v = v > 0.f ? v : 0.f;
      drow[ow] = v;
    }
  }
}

template <bool RELU>
__global__ void __launch_bounds__(64 * kD2sWaves) escoin_d2s_pack_kernel(D2sArgs a) {
#pragma unroll
  for (int pass = 0; pass < kD2sPasses; ++pass) {
    unsigned col, step;
    const unsigned R = d2s_row(a, pass, &col, &step);
    if (R >= a.total_rows) continue;
    const unsigned q = s2d_div(R, a.by_rows), i = R - q * a.rows;        // inner plane q = (n * M + m) * P + phase, inner row i
    const unsigned nm = s2d_div(q, a.by_P), phase = q - nm * a.P;
    const unsigned ph = s2d_div(phase, a.by_sw), pw = phase - ph * a.sw;
    const unsigned oh = i * a.sh + ph - a.pad_h;                         // (wraps below 0: then >= OH)
    const bool row_in = oh < a.OH;
    const unsigned rbase = (nm * a.OH + (row_in ? oh : 0u)) * a.OW;
    float *__restrict__ drow = a.dst + R * a.Wi;
    for (unsigned j = col; j < a.span; j += step) {
      const unsigned ow = j * a.sw + pw - a.pad_w;
      const bool in = row_in && ow < a.OW;
      const unsigned at = in ? rbase + ow : 0u;
      float v = a.src[at];
      if (RELU) v = a.aux[at] > 0.f ? v : 0.f;
      drow[j] = in ? v : 0.f;
    }
  }
}

__global__ void __launch_bounds__(256) escoin_d2s_carry_kernel(const float *__restrict__ src, const int *__restrict__ idx,
                                                                float *__restrict__ dst, unsigned n) {
  const unsigned k = blockIdx.x * 256u + threadIdx.x;
  if (k < n) dst[idx[k]] += src[k];
}

__global__ void __launch_bounds__(256) escoin_d2s_bias_sum_kernel(const float *__restrict__ inner, float *__restrict__ bias_diff,
                                                                   unsigned M, unsigned P) {
  const unsigned m = blockIdx.x * 256u + threadIdx.x;
  if (m >= M) return;
  float s = 0.f;
  for (unsigned ph = 0; ph < P; ++ph) s += inner[m * P + ph];
  bias_diff[m] += s;
}

static int d2s_launch(const escoin_plan *p, const float *src, const float *aux, float *dst, bool pack, bool relu, int n_images,
                      hipStream_t stream) {
  const D2sPlan &dp = p->d2s_state->dp;
  const escoin_conv_desc &d = p->user_desc;
  if (n_images <= 0) return ESCOIN_OK;
  D2sArgs a;
  a.src = src; a.aux = aux; a.dst = dst;
  a.OH = dp.OH; a.OW = dp.OW; a.Hi = d.H + dp.inner.KH - 1; a.Wi = d.W + dp.inner.KW - 1;
  a.M = d.M; a.P = dp.P; a.sh = dp.sh; a.sw = dp.sw; a.pad_h = d.pad_h; a.pad_w = d.pad_w;
  a.rows = pack ? a.Hi : a.OH;
  a.span = pack ? a.Wi : a.OW;
  // (below 2^31: d2s_plan bounds N * M * OH * OW and N * M * P * H' * W', and a row holds at least one element of either)
  const long total = (long)n_images * d.M * (pack ? (long)dp.P : 1L) * a.rows;
  if (total <= 0 || total > 0x7fffffffL || total * (long)a.span > 0x7fffffffL) return fail(ESCOIN_EINVAL, "deconv: row count out of range");
  // (pack: i * sh + ph and the pad are both below 2^31, so their unsigned difference is the row or at least 2^31)
  a.total_rows = (unsigned)total;
  a.lane_shift = s2d_lane_shift(a.span);
  a.by_rows = s2d_div_make(a.rows), a.by_sh = s2d_div_make(a.sh), a.by_sw = s2d_div_make(a.sw);
  a.by_M = s2d_div_make(a.M), a.by_P = s2d_div_make(a.P);
  const long per_wg = (long)kD2sPasses * kD2sWaves * (64 >> a.lane_shift);
  const dim3 grid((unsigned)((total + per_wg - 1) / per_wg)), block(64 * kD2sWaves);
  if (pack) {
    hipLaunchKernelGGL(aux ? escoin_d2s_pack_kernel<true> : escoin_d2s_pack_kernel<false>, grid, block, 0, stream, a);
  } else {
    auto k = relu ? (aux ? escoin_d2s_unpack_kernel<true, true> : escoin_d2s_unpack_kernel<true, false>)
                  : (aux ? escoin_d2s_unpack_kernel<false, true> : escoin_d2s_unpack_kernel<false, false>);
    hipLaunchKernelGGL(k, grid, block, 0, stream, a);
  }
  ESCOIN_HIP_TRY(hipGetLastError());
  return ESCOIN_OK;
}

static int launch_d2s_unpack(const escoin_plan *p, const float *t, const float *bias, float *top, bool relu, int n_images,
                             hipStream_t stream) {
  return d2s_launch(p, t, bias, top, false, relu, n_images, stream);
}

static int launch_d2s_pack(const escoin_plan *p, const float *top_diff, const float *mask, float *g, int n_images, hipStream_t stream) {
  return d2s_launch(p, top_diff, mask, g, true, false, n_images, stream);
}

static int launch_d2s_carry(const float *src, const int *idx, float *dst, long n, hipStream_t stream) {
  if (n <= 0) return ESCOIN_OK;
  if (n > 0x7fffffffL) return fail(ESCOIN_EINVAL, "deconv: more than 2^31 nonzeros");
  hipLaunchKernelGGL(escoin_d2s_carry_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, src, idx, dst, (unsigned)n);
  ESCOIN_HIP_TRY(hipGetLastError());
  return ESCOIN_OK;
}

static int launch_d2s_bias_sum(const float *inner, float *bias_diff, int M, int P, hipStream_t stream) {
  hipLaunchKernelGGL(escoin_d2s_bias_sum_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, stream, inner, bias_diff,
                     (unsigned)M, (unsigned)P);
  ESCOIN_HIP_TRY(hipGetLastError());
  return ESCOIN_OK;
}

// (the plan's core -- escoin_capi.hip, sconv_backward.hip -- reaches these through g_d2s_hooks: escoin_plan.h)
namespace {
__attribute__((used)) const bool g_registered =
    (g_d2s_hooks = D2sHooks{launch_d2s_unpack, launch_d2s_pack, launch_d2s_carry, launch_d2s_bias_sum, "escoin_d2s_unpack_kernel",
                            "escoin_d2s_pack_kernel"}, true);
}  // namespace

}  // namespace escoin
