// b2s.hip -- the two transposes of plan option "b2s" (include/escoin.h "Batch-to-space"): an inner-product layer runs on the
// pointwise kernels as a 1x1 convolution of ceil(N / B) images of 1 x B pixels, the batch as the pixel axis.  Both kernels
// serve both sides; a launch names a BATCH blob of n_images x CH (the bottom or bottom_diff with CH = C, the top or top_diff
// with CH = M: the channel is its contiguous axis) and the INNER blob of ceil(n_images / B) x CH x B (the batch position j
// is its contiguous axis), with batch position p = n' * B + j:
//   escoin_b2s_pack_kernel     inner[n'][ch][j] = batch[p][ch] for p < n_images, +0 for the positions of the last touched
//                              inner image past n_images; with a mask (the top blob, laid out as the batch blob) the value
//                              is mask > 0 ? batch : 0 -- s2b.hip's expression.  X' before the inner forward and the
//                              inner weight gradient, G' before the inner backward.
//   escoin_b2s_unpack_kernel   batch[p][ch] = inner[n'][ch][j] for p < n_images; optionally through v > 0 ? v : 0, the
//                              epilogues' ReLU.  The top after the inner forward, bottom_diff after the inner backward.
// The contiguous axes of the two sides differ, so a workgroup moves a TILE of kB2sTile batch positions x kB2sTile channels
// through LDS: a wave reads a run of consecutive addresses of the source (pack: 64 channels of one batch position; unpack:
// 64 positions of one channel), the tile turns in LDS, and a wave stores a run of consecutive addresses of the destination
// (pack: 64 positions of one channel -- consecutive within an inner image, B floats; unpack: 64 channels of one position).
// The LDS tile is [64][65] floats.  The LDS has 64 banks of 4 bytes; a wave's 4-byte accesses are served as two groups of
// 32 lanes, each over the banks (word mod 32), and only lanes of one group conflict.  With a row pitch of 65 words both
// accesses are conflict-free: a wave's row-wise stores go to words r * 65 + lane, consecutive words; its column-wise reads to
// words lane * 65 + c, and since 65 = 1 (mod 32, and mod 64) that is bank (lane + c), distinct within a group.  A pitch of 64
// would put a whole column in one bank (a 32-way conflict per group); 65 is the smallest pitch without one, at 16.6 KB per
// workgroup.
// Both are one pass with one store per destination element, zeros included: no memset launch, no atomics, no workgroup
// waits for another.  Edge tiles are masked by select: a lane outside the blob reads element 0 (which exists: a launch has
// n_images >= 1) and selects +0, and its store is skipped.  Every offset is a 32-bit one: align_rules.h b2s_plan refuses a
// layer whose X' or T' reaches 2^31 elements, and the bottom and the top are no larger.  Images at or past n_images are
// neither read nor written on the batch side; inner images past the last touched one are not written.
#include <hip/hip_runtime.h>

#include "escoin_plan.h"

namespace escoin {

struct B2sArgs {
  const float *src;
  const float *mask;        // pack: null, or the blob whose sign gates src
  float *dst;
  unsigned CH;              // channels: C (bottom side) or M (top side)
  unsigned B;               // batch positions per inner image
  unsigned n_images;        // batch positions that exist
  unsigned positions;       // pack: ceil(n_images / B) * B, the positions that are stored; unpack: n_images
  unsigned ctiles;          // tiles along the channels
  S2dDiv by_ctiles, by_B;
};

constexpr unsigned kB2sTile = 64, kB2sPitch = kB2sTile + 1, kB2sWaves = 4, kB2sRowsPerWave = kB2sTile / kB2sWaves;

// Element (ch, p) of the inner blob.
__device__ inline unsigned b2s_inner_at(const B2sArgs &a, unsigned ch, unsigned p) {
  const unsigned np = s2d_div(p, a.by_B), j = p - np * a.B;
  return (np * a.CH + ch) * a.B + j;
}

template <bool MASK>
__global__ void __launch_bounds__(64 * kB2sWaves) escoin_b2s_pack_kernel(B2sArgs a) {
  __shared__ float tile[kB2sTile * kB2sPitch];
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const unsigned pt = s2d_div(blockIdx.x, a.by_ctiles), ct = blockIdx.x - pt * a.ctiles;
  const unsigned p0 = pt * kB2sTile, c0 = ct * kB2sTile;
  // rows of the batch blob: lane = channel
#pragma unroll
  for (unsigned r = 0; r < kB2sRowsPerWave; ++r) {
    const unsigned pl = wave * kB2sRowsPerWave + r, p = p0 + pl, ch = c0 + lane;
    const bool in = p < a.n_images && ch < a.CH;
    const unsigned at = in ? p * a.CH + ch : 0u;
    float v = a.src[at];
    if (MASK) v = a.mask[at] > 0.f ? v : 0.f;
    tile[pl * kB2sPitch + lane] = in ? v : 0.f;
  }
  __syncthreads();
  // rows of the inner blob: lane = batch position
#pragma unroll
  for (unsigned r = 0; r < kB2sRowsPerWave; ++r) {
    const unsigned cl = wave * kB2sRowsPerWave + r, ch = c0 + cl, p = p0 + lane;
    if (ch < a.CH && p < a.positions) a.dst[b2s_inner_at(a, ch, p)] = tile[lane * kB2sPitch + cl];
  }
}

template <bool RELU>
__global__ void __launch_bounds__(64 * kB2sWaves) escoin_b2s_unpack_kernel(B2sArgs a) {
  __shared__ float tile[kB2sTile * kB2sPitch];
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const unsigned pt = s2d_div(blockIdx.x, a.by_ctiles), ct = blockIdx.x - pt * a.ctiles;
  const unsigned p0 = pt * kB2sTile, c0 = ct * kB2sTile;
  // rows of the inner blob: lane = batch position
#pragma unroll
  for (unsigned r = 0; r < kB2sRowsPerWave; ++r) {
    const unsigned cl = wave * kB2sRowsPerWave + r, ch = c0 + cl, p = p0 + lane;
    const bool in = ch < a.CH && p < a.positions;
    float v = a.src[in ? b2s_inner_at(a, ch, p) : 0u];
    if (RELU) v = v > 0.f ? v : 0.f;
    tile[cl * kB2sPitch + lane] = in ? v : 0.f;
  }
  __syncthreads();
  // rows of the batch blob: lane = channel
#pragma unroll
  for (unsigned r = 0; r < kB2sRowsPerWave; ++r) {
    const unsigned pl = wave * kB2sRowsPerWave + r, p = p0 + pl, ch = c0 + lane;
    if (p < a.positions && ch < a.CH) a.dst[p * a.CH + ch] = tile[lane * kB2sPitch + pl];
  }
}

static int b2s_launch(const escoin_plan *p, const float *src, const float *mask, float *dst, bool pack, bool top_side, bool relu,
                      int n_images, hipStream_t stream) {
  const B2sPlan &bp = p->b2s_state->bp;
  if (n_images <= 0) return ESCOIN_OK;      // (no image touches an inner image: nothing is stored)
  B2sArgs a;
  a.src = src; a.mask = mask; a.dst = dst;
  a.CH = (unsigned)(top_side ? p->g.d.M : p->g.d.C);
  a.B = (unsigned)bp.B;
  a.n_images = (unsigned)n_images;
  const long touched = ((long)n_images + bp.B - 1) / bp.B;
  const long positions = pack ? touched * bp.B : (long)n_images;
  // (below 2^31: b2s_plan bounds X' and T', of which this is a part)
  if (touched > bp.inner.N || positions * (long)a.CH > 0x7fffffffL) return fail(ESCOIN_EINVAL, "b2s: element count out of range");
  a.positions = (unsigned)positions;
  a.ctiles = (a.CH + kB2sTile - 1) / kB2sTile;
  const long tiles = (positions + kB2sTile - 1) / kB2sTile * (long)a.ctiles;
  if (tiles > 0x7fffffffL) return fail(ESCOIN_EINVAL, "b2s: tile count out of range");
  a.by_ctiles = s2d_div_make(a.ctiles), a.by_B = s2d_div_make(a.B);
  const dim3 grid((unsigned)tiles), block(64 * kB2sWaves);
  if (pack) hipLaunchKernelGGL(mask ? escoin_b2s_pack_kernel<true> : escoin_b2s_pack_kernel<false>, grid, block, 0, stream, a);
  else hipLaunchKernelGGL(relu ? escoin_b2s_unpack_kernel<true> : escoin_b2s_unpack_kernel<false>, grid, block, 0, stream, a);
  ESCOIN_HIP_TRY(hipGetLastError());
  return ESCOIN_OK;
}

static int launch_b2s_pack(const escoin_plan *p, const float *src, const float *mask, float *dst, bool top_side, int n_images,
                           hipStream_t stream) {
  return b2s_launch(p, src, mask, dst, true, top_side, false, n_images, stream);
}

static int launch_b2s_unpack(const escoin_plan *p, const float *src, float *dst, bool top_side, bool relu, int n_images,
                             hipStream_t stream) {
  return b2s_launch(p, src, nullptr, dst, false, top_side, relu, n_images, stream);
}

// (the plan's core -- escoin_capi.hip, sconv_backward.hip, dense_wgrad.hip -- reaches these through g_b2s_hooks: escoin_plan.h)
namespace {
__attribute__((used)) const bool g_registered =
    (g_b2s_hooks = B2sHooks{launch_b2s_pack, launch_b2s_unpack, "escoin_b2s_pack_kernel", "escoin_b2s_unpack_kernel"}, true);
}  // namespace

}  // namespace escoin
