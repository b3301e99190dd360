// w2b.hip -- the three rearrangements of plan option "w2b" (include/escoin.h "Width-to-batch"): a stride-1, dilation-1 layer
// whose rows are wider than the tiled kernels take runs on them as a convolution of N * S images, each one column STRIP of
// the bottom with its halo.  A launch names a SPREAD blob of n_images x CH x Hr rows of Ws elements (the bottom or
// bottom_diff: CH = C, Hr = H, Ws = W; the top or top_diff: CH = M, Hr = OH, Ws = OW) and the STRIP blob of n_images * S x
// CH x Hr rows of Wd elements (bottom side Wd = Wi = SW + KW - 1, top side Wd = SW), strip s of image n being image
// n' = n * S + s.  Column x of a strip row is column s * SW - off + x of the spread row, off = pad_w on the bottom side and 0
// on the top side: a strip row is ONE contiguous run of the spread row, so both sides of every copy are unit-stride.
//   escoin_w2b_pack_kernel        strip[n'][ch][h][x] = spread[n][ch][h][s * SW - off + x] inside the spread row, +0 outside
//                                 (the pad, and the tail of the last strip); with a mask (the top blob, laid out as the
//                                 spread blob) the value is mask > 0 ? spread : 0 -- s2b.hip's expression.  X' before the
//                                 inner forward and the inner weight gradient, G' before the inner backward.
//   escoin_w2b_unpack_kernel      spread[n][ch][h][w] = strip[n * S + w / SW][ch][h][w % SW]: the top after the inner
//                                 forward, every element from exactly one strip; optionally through v > 0 ? v : 0.
//   escoin_w2b_unpack_sum_kernel  the data gradient: spread[n][c][h][w] = the sum, in ascending s, of strip[n * S + s][c][h]
//                                 [w + pad_w - s * SW] over the strips whose [0, Wi) holds that column.  With p = w + pad_w,
//                                 s0 = p / SW and j0 = p % SW those are s0 (where s0 < S) and s0 - 1 (where s0 >= 1 and
//                                 j0 < KW - 1: the halo) and no other, because SW >= KW - 1 (align_rules.h w2b_plan): one
//                                 or two terms, gathered per destination element -- deterministic, no atomics.  Columns of
//                                 the padded frame outside the bottom are never visited.
// All three are one pass with one store per destination element, zeros included: no memset launch, no atomics, no workgroup
// waits for another.  pack walks the rows of the STRIP side, the two unpacks the rows of the SPREAD side; a row gets the
// smallest power of two of lanes that covers it, up to a wave, and longer rows go in a lane-strided loop (s2d.hip's scheme;
// S2dDiv and s2d_lane_shift are align_rules.h's): a wave's lanes read and write consecutive addresses.
// Quads (V = 4): on the top side SW is a multiple of 4, so where OW is one too and the three pointers are 16-byte aligned
// every row of both sides starts on a quad, a quad of the spread row at column w = 4 k lies inside ONE strip (s * SW is a
// multiple of 4) at column j = w - s * SW, itself a multiple of 4, and a quad of a strip row lies wholly inside the spread
// row or wholly outside it (OW is a multiple of 4).  pack and unpack then move float4s.  The bottom side (a strip starts at
// s * SW - pad_w, and Wi is a multiple of 4 for KW = 1, 5, 9, ... only) and the sum stay scalar.
// Every offset is a 32-bit one: w2b_plan refuses a layer whose bottom, top, X' or T' reaches 2^31 elements, and a row holds at
// least one element of the side it walks, so every row and workgroup count stays below 2^31.  Images at or past n_images are
// neither read nor written, on either side.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "escoin_plan.h"

namespace escoin {

struct W2bArgs {
  const float *src;
  const float *mask;        // pack: null, or the blob whose sign gates src
  float *dst;
  unsigned plane_rows;      // CH * Hr: the rows of one image, on either side
  unsigned Ws, Wd;          // elements of a spread row / of a strip row
  unsigned S, SW, off;      // strips per image, a strip's output width, the spread row's offset in the padded frame
  unsigned halo;            // KW - 1 (unpack_sum)
  unsigned total_rows;      // the rows a launch walks: pack n_images * S * plane_rows, the unpacks n_images * plane_rows
  unsigned span;            // lanes' range along a row, in units of V elements: pack Wd / V, the unpacks Ws / V
  unsigned lane_shift;      // log2 of the lanes per row
  S2dDiv by_plane_rows, by_S, by_SW;
};

constexpr int kW2bWaves = 4, kW2bPasses = 2;

// The row a lane works on in pass `pass` (>= total_rows: none), its first unit and its step.
__device__ inline unsigned w2b_row(const W2bArgs &a, int pass, unsigned *col, unsigned *step) {
  const unsigned per_wave = 64u >> a.lane_shift;
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  *step = 1u << a.lane_shift;
  *col = lane & (*step - 1u);
  return ((blockIdx.x * kW2bPasses + (unsigned)pass) * kW2bWaves + wave) * per_wave + (lane >> a.lane_shift);
}

// V consecutive floats at p (V = 4: p is 16-byte aligned)
template <int V> struct W2bVec;
template <> struct W2bVec<1> {
  float v;
  __device__ static W2bVec load(const float *p) { return {*p}; }
  __device__ static W2bVec zero() { return {0.f}; }
  __device__ void store(float *p) const { *p = v; }
  // mask > 0 ? this : 0 per element; v > 0 ? v : 0
  __device__ W2bVec gate(const W2bVec &m) const { return {m.v > 0.f ? v : 0.f}; }
};
template <> struct W2bVec<4> {
  float4 v;
  __device__ static W2bVec load(const float *p) { return {*reinterpret_cast<const float4 *>(p)}; }
  __device__ static W2bVec zero() { return {make_float4(0.f, 0.f, 0.f, 0.f)}; }
  __device__ void store(float *p) const { *reinterpret_cast<float4 *>(p) = v; }
  __device__ W2bVec gate(const W2bVec &m) const {
    return {make_float4(m.v.x > 0.f ? v.x : 0.f, m.v.y > 0.f ? v.y : 0.f, m.v.z > 0.f ? v.z : 0.f, m.v.w > 0.f ? v.w : 0.f)};
  }
};

template <bool MASK, int V>
__global__ void __launch_bounds__(64 * kW2bWaves) escoin_w2b_pack_kernel(W2bArgs a) {
  typedef W2bVec<V> Vec;
#pragma unroll
  for (int pass = 0; pass < kW2bPasses; ++pass) {
    unsigned col, step;
    const unsigned R = w2b_row(a, pass, &col, &step);            // a strip row
    if (R >= a.total_rows) continue;
    const unsigned np = s2d_div(R, a.by_plane_rows), r = R - np * a.plane_rows;
    const unsigned n = s2d_div(np, a.by_S), s = np - n * a.S;
    const float *__restrict__ srow = a.src + (n * a.plane_rows + r) * a.Ws;
    const float *__restrict__ mrow = MASK ? a.mask + (n * a.plane_rows + r) * a.Ws : nullptr;
    float *__restrict__ drow = a.dst + R * a.Wd;
    const int c0 = (int)(s * a.SW) - (int)a.off;                 // the spread column of strip column 0
    for (unsigned u = col; u < a.span; u += step) {
      const unsigned x = u * V;
      const int c = c0 + (int)x;
      // (V = 4: c and Ws are multiples of 4, so the quad is inside the row or outside it as a whole)
      Vec v = Vec::zero();
      if ((unsigned)c < a.Ws) {
        v = Vec::load(srow + c);
        if (MASK) v = v.gate(Vec::load(mrow + c));
      }
      v.store(drow + x);
    }
  }
}

template <bool RELU, int V>
__global__ void __launch_bounds__(64 * kW2bWaves) escoin_w2b_unpack_kernel(W2bArgs a) {
  typedef W2bVec<V> Vec;
#pragma unroll
  for (int pass = 0; pass < kW2bPasses; ++pass) {
    unsigned col, step;
    const unsigned R = w2b_row(a, pass, &col, &step);            // a spread row
    if (R >= a.total_rows) continue;
    const unsigned n = s2d_div(R, a.by_plane_rows), r = R - n * a.plane_rows;
    const unsigned row0 = n * a.S * a.plane_rows + r;            // the row in strip 0; strip s adds s * plane_rows
    float *__restrict__ drow = a.dst + R * a.Ws;
    for (unsigned u = col; u < a.span; u += step) {
      const unsigned w = u * V;
      const unsigned s = s2d_div(w, a.by_SW), j = w - s * a.SW;  // s < S: w < Ws <= S * SW
      Vec v = Vec::load(a.src + (row0 + s * a.plane_rows) * a.Wd + j);
      if (RELU) v = v.gate(v);
      v.store(drow + w);
    }
  }
}

__global__ void __launch_bounds__(64 * kW2bWaves) escoin_w2b_unpack_sum_kernel(W2bArgs a) {
#pragma unroll
  for (int pass = 0; pass < kW2bPasses; ++pass) {
    unsigned col, step;
    const unsigned R = w2b_row(a, pass, &col, &step);            // a spread row
    if (R >= a.total_rows) continue;
    const unsigned n = s2d_div(R, a.by_plane_rows), r = R - n * a.plane_rows;
    const unsigned row0 = n * a.S * a.plane_rows + r;
    float *__restrict__ drow = a.dst + R * a.Ws;
    for (unsigned w = col; w < a.span; w += step) {
      const unsigned p = w + a.off;
      const unsigned s0 = s2d_div(p, a.by_SW), j0 = p - s0 * a.SW;
      // s0 <= S (p < Ws + 2 off = OW + halo <= S * SW + SW), and at s0 == S the column is in strip S - 1's halo:
      // j0 = p - S * SW < halo.  So at least one of the two terms exists, and neither index leaves its strip row:
      // j0 < SW <= Wd, j0 + SW < halo + SW = Wd.
      const bool lo = s0 >= 1u && j0 < a.halo, hi = s0 < a.S;
      float v = 0.f;
      if (lo) v = a.src[(row0 + (s0 - 1u) * a.plane_rows) * a.Wd + j0 + a.SW];
      if (hi) {
        const float b = a.src[(row0 + s0 * a.plane_rows) * a.Wd + j0];
        v = lo ? v + b : b;
      }
      drow[w] = v;
    }
  }
}

enum W2bKind { kW2bPack, kW2bUnpack, kW2bUnpackSum };

static bool w2b_quad_aligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

static int w2b_launch(const escoin_plan *p, const float *src, const float *mask, float *dst, W2bKind kind, bool top_side, bool relu,
                      int n_images, hipStream_t stream) {
  const Geometry &g = p->g;
  const escoin_conv_desc &d = g.d;
  const W2bPlan &wp = p->w2b_state->wp;
  if (n_images <= 0) return ESCOIN_OK;
  W2bArgs a;
  a.src = src; a.mask = mask; a.dst = dst;
  a.S = (unsigned)wp.S; a.SW = (unsigned)wp.SW; a.halo = (unsigned)(d.KW - 1);
  if (top_side) {
    a.plane_rows = (unsigned)d.M * (unsigned)g.OH; a.Ws = (unsigned)g.OW; a.Wd = (unsigned)wp.SW; a.off = 0;
  } else {
    a.plane_rows = (unsigned)d.C * (unsigned)d.H; a.Ws = (unsigned)d.W; a.Wd = (unsigned)wp.Wi; a.off = (unsigned)d.pad_w;
  }
  // (what the kernels' indices rely on: the strips' outputs cover the top row -- unpack's s < S -- their inputs the padded bottom
  //  row, and a column lies in at most two strips)
  if ((long)wp.S * wp.SW < (top_side ? (long)a.Ws : (long)a.Ws + 2L * a.off - a.halo) || a.halo > a.SW || a.Wd > a.SW + a.halo)
    return fail(ESCOIN_EINVAL, "w2b: the strips do not cover the image");
  // (below 2^31: w2b_plan bounds all four blobs, and a row holds at least one element of the side it walks)
  const bool pack = kind == kW2bPack;
  const long rows = (long)n_images * (pack ? wp.S : 1) * a.plane_rows;
  const long strip_floats = (long)n_images * wp.S * a.plane_rows * a.Wd, spread_floats = (long)n_images * a.plane_rows * a.Ws;
  if (rows <= 0 || strip_floats > 0x7fffffffL || spread_floats > 0x7fffffffL) return fail(ESCOIN_EINVAL, "w2b: row count out of range");
  a.total_rows = (unsigned)rows;
  const bool quads = kind != kW2bUnpackSum && top_side && a.Ws % 4 == 0 && a.Wd % 4 == 0 && w2b_quad_aligned(src) && w2b_quad_aligned(dst) &&
                     (!mask || w2b_quad_aligned(mask));
  a.span = (pack ? a.Wd : a.Ws) / (quads ? 4u : 1u);
  a.lane_shift = s2d_lane_shift(a.span);
  a.by_plane_rows = s2d_div_make(a.plane_rows), a.by_S = s2d_div_make(a.S), a.by_SW = s2d_div_make(a.SW);
  const long per_wg = (long)kW2bPasses * kW2bWaves * (64 >> a.lane_shift);
  const dim3 grid((unsigned)((rows + per_wg - 1) / per_wg)), block(64 * kW2bWaves);
  if (kind == kW2bUnpackSum) {
    hipLaunchKernelGGL(escoin_w2b_unpack_sum_kernel, grid, block, 0, stream, a);
  } else if (pack) {
    auto k = mask ? (quads ? escoin_w2b_pack_kernel<true, 4> : escoin_w2b_pack_kernel<true, 1>)
                  : (quads ? escoin_w2b_pack_kernel<false, 4> : escoin_w2b_pack_kernel<false, 1>);
    hipLaunchKernelGGL(k, grid, block, 0, stream, a);
  } else {
    auto k = relu ? (quads ? escoin_w2b_unpack_kernel<true, 4> : escoin_w2b_unpack_kernel<true, 1>)
                  : (quads ? escoin_w2b_unpack_kernel<false, 4> : escoin_w2b_unpack_kernel<false, 1>);
    hipLaunchKernelGGL(k, grid, block, 0, stream, a);
  }
  ESCOIN_HIP_TRY(hipGetLastError());
  return ESCOIN_OK;
}

static int launch_w2b_pack(const escoin_plan *p, const float *src, const float *mask, float *dst, bool top_side, int n_images,
                           hipStream_t stream) {
  return w2b_launch(p, src, mask, dst, kW2bPack, top_side, false, n_images, stream);
}

static int launch_w2b_unpack(const escoin_plan *p, const float *src, float *dst, bool relu, int n_images, hipStream_t stream) {
  return w2b_launch(p, src, nullptr, dst, kW2bUnpack, true, relu, n_images, stream);
}

static int launch_w2b_unpack_sum(const escoin_plan *p, const float *src, float *dst, int n_images, hipStream_t stream) {
  return w2b_launch(p, src, nullptr, dst, kW2bUnpackSum, false, false, n_images, stream);
}

// (the plan's core -- escoin_capi.hip, sconv_backward.hip, dense_wgrad.hip -- reaches these through g_w2b_hooks: escoin_plan.h)
namespace {
__attribute__((used)) const bool g_registered =
    (g_w2b_hooks = W2bHooks{launch_w2b_pack, launch_w2b_unpack, launch_w2b_unpack_sum, "escoin_w2b_pack_kernel",
                            "escoin_w2b_unpack_kernel", "escoin_w2b_unpack_sum_kernel"},
     true);
}  // namespace

}  // namespace escoin
