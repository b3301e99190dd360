// dgrad_bf16.hip -- the bf16 math mode of the MFMA data-gradient kernel (plan option "dgrad_math" = ESCOIN_MATH_BF16;
// include/escoin.h "bf16 data gradient"): per conv group and stride phase
//     dX_phase[Cg x P] = bf16(Wt_phase)[Cg x Kp] * bf16(gather(G))[Kp x P],   fp32 sums,
// G = top_diff (x [top > 0] on fuse_relu plans, masked BEFORE the rounding), on v_mfma_f32_32x32x16_bf16.  The twin of
// escoin_sconv_dgrad_mfma_kernel (dgrad_mfma.hip): its phase decomposition, its workgroup tile (64 input channels x 64 phase
// pixels, four waves in 2 x 2 blocks of 32 x 32), its grid, its argument block and every table of DgmState -- the one fp32
// phase matrix included, so the option holds no state and weight updates need nothing new --, its zero-by-select rule, its
// epilogue and its partial-batch behaviour.  The staging and the multiply are this file's.
//   iteration two consecutive entries of the (group, phase, channel tile)'s live list -- two steps of 32 columns, which need
//             not be adjacent in the matrix -- per barrier: 64 columns.  An odd list ends in a half iteration of one step
//             behind a wave-uniform branch.  An empty list is the zero-fill case.
//   staging   the reduction axis is the column axis k = (ocl, tap), and the bf16 instruction takes 8 consecutive k of one
//             row from a lane, so both LDS tiles are k-contiguous: [64 channels][64 k] and [64 pixels][64 k], 128 bytes a
//             row, 8 chunks of 8 columns.  Chunks 0..3 are the first step's columns, chunks 4..7 the second's.  A thread
//             keeps its lane as the tile's channel / pixel and wave w takes chunks w and w + 4: per chunk 8 weight loads,
//             each one run of 256 contiguous bytes per wave from the step's [column][64 channels] block, and 8 gathered G
//             values through the wave-uniform column decode, the lanes along consecutive phase pixels.  Dead pixels, invalid
//             columns, taps outside the top, dead channels and elements masked by the ReLU are taken by select; then the 8
//             values are rounded to bf16 (nearest even, NaN stays NaN: v_cvt_pk_bf16_f32) and written by ONE 16-byte LDS
//             store.
//   pipeline  two LDS buffers, one barrier per iteration: the global loads of iteration i + 1 go out to registers before the
//             matrix instructions of iteration i and are converted and written to the other buffer at the top of the next
//             iteration.
//   multiply  wave (wc, wp) owns the 32 x 32 block (channels 32 wc.., pixels 32 wp..): per iteration 4 (a half one: 2)
//             v_mfma_f32_32x32x16_bf16 (exact products of the rounded operands, fp32 sums); in instruction u lane (i, h)
//             feeds Wt[32 wc + i][16 u + 8 h .. + 7] and G[16 u + 8 h .. + 7][32 wp + i], one 16-byte LDS read each.  The
//             accumulators are in the C/D layout the fp32 kernel's epilogue decodes.
// The order of an element's sum -- live steps ascending, within a step its two instructions ascending, within an instruction
// its own fixed order over its 16 columns -- is a function of the geometry and the pattern only: not of n_images, not of the
// image's place in the batch, not of the blobs' alignment (every load is 4 bytes), and not of how the steps pair up.
// As in the fp32 kernel a pruned position inside a live block contributes 0 x bf16(G): a non-finite G there gives NaN.
//
// LDS: a tile is 64 rows of 64 bf16 = 128 bytes = 8 chunks of 16 bytes; chunk c of row r sits in slot c ^ ((r >> 1) & 7) of
// the row (the swizzle of dense_bf16.hip and wgrad_bf16_step.h on rows of the same length); no padding: 2 buffers x 2 tiles x
// 8 KiB = kDgbLdsBytes.  With 64 banks of 4 bytes a row covers half the banks, even rows banks 0..31, odd rows banks 32..63.
// The staging store and the fragment read are the same access: 16 bytes per lane, the lanes along consecutive rows at ONE
// logical chunk (the store: lane = row, chunk w or w + 4; the read: lanes 0..31 rows 32 wc.. at chunk 2 u, lanes 32..63 the
// same rows at chunk 2 u + 1), 16 lanes = 256 bytes per pass.  16 consecutive rows from a multiple of 16 are 8 even and 8 odd
// rows, and within either parity (r >> 1) & 7 takes its 8 values once: 8 different slots of 4 banks in each bank half --
// every bank once.  So both are free of bank conflicts by construction (under the pass size named; an argument from the
// layout, not a measurement).
#include <hip/hip_runtime.h>

#include "align_rules.h"
#include "escoin_plan.h"

namespace escoin {

typedef float dgb_f32x16 __attribute__((ext_vector_type(16)));
typedef float dgb_f32x8 __attribute__((ext_vector_type(8)));
typedef __bf16 dgb_bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kDgbThreads = 256;
constexpr int kDgbChunk = 8;                                   // columns per 16-byte chunk: what a lane feeds an instruction
constexpr int kDgbRowChunks = kDgbStepK / kDgbChunk;           // 8 chunks per LDS row
constexpr int kDgbHalfChunks = kDgmStepK / kDgbChunk;          // 4: the chunks of one live step, one per wave
constexpr int kDgbTileChunks = kDgmTileC * kDgbRowChunks;      // chunks per tile
static_assert(kDgmTileC == 64 && kDgmTileP == 64 && kDgmStepK == 32 && kDgbStepK == 2 * kDgmStepK && kDgbRowChunks == 8 &&
                  kDgbHalfChunks * 64 == kDgbThreads,
              "the staging map and the swizzle are written for 64 x 64 tiles, live steps of 32 columns taken two at a time");
static_assert(sizeof(dgb_bf16x8) * 4 * kDgbTileChunks == kDgbLdsBytes, "align_rules.h reports this kernel's LDS");

__device__ __forceinline__ int dgb_chunk_at(int row, int chunk) { return row * kDgbRowChunks + (chunk ^ ((row >> 1) & 7)); }

template <bool RELU>
__global__ void __launch_bounds__(kDgbThreads)
escoin_sconv_dgrad_bf16_kernel(DgmArgs a) {
  __shared__ __attribute__((aligned(16))) dgb_bf16x8 sW[2][kDgbTileChunks];
  __shared__ __attribute__((aligned(16))) dgb_bf16x8 sG[2][kDgbTileChunks];
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
  const int niter = (nlive + 1) >> 1;
  const int c0 = ct * kDgmTileC;
  const int opix = a.OH * a.OW;

  // staging role: pixel / channel `lane` of the tile, columns 8 wave .. + 7 of either live step of the iteration
  const long p = p0 + lane;
  const bool plive = p < total;
  const int n = plive ? (int)(p / ppix) : 0, r = plive ? (int)(p - (long)n * ppix) : 0;
  const int hh = r / cols, ww = r - hh * cols;
  const float *__restrict__ gimg = a.top_diff + ((size_t)n * a.M + (size_t)grp * a.Mg) * opix;
  const float *__restrict__ timg = RELU ? a.top + ((size_t)n * a.M + (size_t)grp * a.Mg) * opix : nullptr;
  const bool clive = c0 + lane < a.Cg;
  const float *__restrict__ wblk = a.mat + (((size_t)grp * a.ctiles + ct) * a.cols_total + col0) * kDgmTileC + lane;
  dgb_f32x8 wv[2], gv[2];
  // half `half` of the iteration: this wave's chunk of live step s
  auto load = [&](int half, int s) {
    const int kb = s * kDgmStepK + kDgbChunk * wave;
#pragma unroll
    for (int j = 0; j < kDgbChunk; ++j) {
      const int k = kb + j;
      const int4 t = a.col[col0 + k];                       // (the table covers whole steps)
      const int oh = hh + t.y, ow = ww + t.z;
      float g = 0.f;
      if (plive && t.w && (unsigned)oh < (unsigned)a.OH && (unsigned)ow < (unsigned)a.OW) {
        const int at = t.x + oh * a.OW + ow;                // (Mg*OH*OW < 2^31: dgm_plan)
        g = gimg[at];
        if (RELU && !(timg[at] > 0.f)) g = 0.f;
      }
      gv[half][j] = g;
      wv[half][j] = clive ? wblk[(size_t)k * kDgmTileC] : 0.f;
    }
  };
  // iteration it: entries 2 it and, where the list has it, 2 it + 1 of the live list (wave-uniform)
  auto load_iter = [&](int it) {
    load(0, a.live[lb + 2 * it]);
    if (2 * it + 1 < nlive) load(1, a.live[lb + 2 * it + 1]);
  };
  auto store = [&](int buf, int half) {
    const int at = dgb_chunk_at(lane, wave + kDgbHalfChunks * half);
    sW[buf][at] = __builtin_convertvector(wv[half], dgb_bf16x8);      // four v_cvt_pk_bf16_f32: nearest even, overflow to infinity
    sG[buf][at] = __builtin_convertvector(gv[half], dgb_bf16x8);
  };

  const int wc = wave >> 1, wp = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  dgb_f32x16 acc = {0};
  auto multiply = [&](int buf, int half) {
    dgb_bf16x8 fw[2], fg[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      fw[u] = sW[buf][dgb_chunk_at(wc * 32 + li, kDgbHalfChunks * half + 2 * u + lh)];
      fg[u] = sG[buf][dgb_chunk_at(wp * 32 + li, kDgbHalfChunks * half + 2 * u + lh)];
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw[u], fg[u], acc, 0, 0, 0);
  };
  if (niter > 0) load_iter(0);
  for (int it = 0; it < niter; ++it) {
    const int buf = it & 1;
    const bool pair = 2 * it + 1 < nlive;
    store(buf, 0);
    if (pair) store(buf, 1);
    // everyone's part of iteration it is in buf -- and everyone is past the multiply of iteration it - 1, which read the
    // other buffer
    __syncthreads();
    if (it + 1 < niter) load_iter(it + 1);
    multiply(buf, 0);
    if (pair) multiply(buf, 1);                             // (a half iteration's chunks 4..7 are neither written nor read)
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

// The launch launch_dgrad_mfma hands its filled argument block and grid to for a plan whose option "dgrad_math" is
// ESCOIN_MATH_BF16.  No allocation, no synchronisation (capturable into a graph), as the fp32 launch.
static int launch_dgrad_bf16(const DgmArgs &a, dim3 grid, bool relu, hipStream_t stream) {
  const dim3 block(kDgbThreads);
  if (relu) hipLaunchKernelGGL(escoin_sconv_dgrad_bf16_kernel<true>, grid, block, 0, stream, a);
  else hipLaunchKernelGGL(escoin_sconv_dgrad_bf16_kernel<false>, grid, block, 0, stream, a);
  ESCOIN_HIP_TRY(hipGetLastError());
  return ESCOIN_OK;
}

// (launch_dgrad_mfma reaches this through g_dgrad_bf16_launch, escoin_plan.h: a program that links the core's objects alone
// still links, and refuses the option there)
namespace {
__attribute__((used)) const bool g_registered = (g_dgrad_bf16_launch = launch_dgrad_bf16, true);
}  // namespace

}  // namespace escoin
