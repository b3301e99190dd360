// dense_bf16.hip -- the dense forward kernel's bf16 math mode (plan option "dense_math" = ESCOIN_MATH_BF16): the implicit
// GEMM of dense_mfma.hip,
//     C[Mg x P] = A[Mg x K] * B[K x P]   per conv group,   K = Cg*KH*KW,  P = N*OH*OW,
// with both operands rounded to bf16 (nearest even, v_cvt_pk_bf16_f32) on their way into LDS and multiplied by
// v_mfma_f32_32x32x16_bf16: exact products of the rounded operands, fp32 sums.  The blobs and the plan's weight matrix stay
// fp32 -- dense.w is read as it is, so whatever updates it (update_values, the solver step, prune, rewire) needs no second
// copy -- and bias and ReLU are applied in fp32 in the epilogue.
//
// The tiles, the persistent workgroups (two per CU, four waves each; BM = 128: waves 2 x 2, 64 x 64 outputs each; BM = 64
// for Mg <= 64: waves 1 x 4, 64 x 32 each), the group mask, the `ktab` decode, the range-checked buffer loads that deliver
// the padding's zeros and the epilogue are the fp32 kernel's.  The k-loop is its own:
//   * k-steps of 64 (four matrix instructions of 16 k per 32 x 32 block), one barrier each, across tile boundaries.
//   * The data changes type on the way, so LDS-DMA cannot carry it: the loads of step s + 1 go out to REGISTERS before the
//     matrix instructions of step s and are converted and written to the other LDS buffer after them.  An operand is
//     converted once, by the lane that stages it, never by the waves that consume it.
//   * Both tiles are k-contiguous in LDS -- A [m][64 k], B [p][64 k], rows of 128 bytes = 8 chunks of 8 bf16 -- because the
//     instruction takes 8 consecutive k of row / column lane % 32 per lane (k-group lane / 32): one ds_read_b128 is one
//     operand.  A fragment of A serves all of a wave's column blocks.
//   * A staging: a lane loads 8 consecutive k of one row (two 16-byte loads; 8 lanes cover a row's 256 bytes), packs them
//     and writes one chunk.  B staging: a lane owns ONE pixel and 8 consecutive k -- eight 4-byte loads, each coalesced
//     across the wave along p, addressed directly in the pointwise case (BMODE 1) and through ktab and the (dy, dx) border
//     test otherwise (BMODE 0) -- and writes one chunk.
//   * Swizzle (chunk_at): chunk c of row r sits in slot c ^ ((r >> 1) & 7) of the row, the fp32 kernel's a_swizzle on rows
//     of the same 128 bytes.  Sixteen consecutive rows at one logical chunk -- a quarter of a fragment read, and a quarter
//     of a B staging write (64 consecutive pixels, one chunk) -- are 8 even rows in bank half 0 and 8 odd rows in bank
//     half 1 (a row is 32 of the 64 banks), each in 8 different slots: all 64 banks once.  An A staging write covers whole
//     rows (8 lanes = the 8 slots of a row in some order): contiguous, conflict-free as well.
// Rows past K: B stages zeros there (ktab entries past K fail the border test; the pointwise path compares k with K; past
// ktab's end -- K rounded up to 32 -- nothing is read), and so does A past lda (up to lda the matrix's own zero padding).
// The tile walk, the B staging, the swizzle and the epilogue live in dense_common.h: dense_sp24.hip shares them.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "align_rules.h"
#include "dense_common.h"
#include "escoin_plan.h"

namespace escoin {

constexpr int kBK16 = kDb16StepK;                 // k per step
constexpr int kRowChunks = kB16RowChunks;         // 16-byte chunks per LDS row
static_assert(kBN == kDb16TileP && kBK16 == kB16StepK && kRowChunks == 8, "the swizzle and the staging maps are written for 128 x 64 tiles");

// BMODE: how the B tile's elements are addressed (dense_common.h DenseB16Stage)
template <int WROWS, int BMODE>
__global__ void __launch_bounds__(256, 2) escoin_dense_bf16_kernel(DenseArgs a) {
  constexpr int BM = 64 * WROWS;
  constexpr int WCOLS = 4 / WROWS;           // waves along the pixel axis
  constexpr int WN = kBN / WCOLS;            // columns per wave: 64 or 32
  constexpr int NB = WN / 32;                // 32-column blocks per wave
  constexpr int AQ = BM / 32;                // A chunks a lane stages per k-step: rows 32 q + tid / 8, chunk tid % 8
  // one array per buffer: A tile then B tile, in bf16 (the epilogue reuses a whole buffer as its fp32 staging area:
  // 4 waves x 32 x WN floats = 32 KiB of the 32 KiB buffer at BM = 128, 16 of 24 KiB at BM = 64)
  constexpr int kBufChunks = (BM + kBN) * kRowChunks;
  constexpr int kBufFloats = kBufChunks * 4;
  static_assert(4 * 32 * WN <= kBufFloats, "the epilogue's staging area is one buffer");
  __shared__ __attribute__((aligned(1024))) float sAB[2][kBufFloats];
  auto sA = [&](int b) -> bf16x8 * { return reinterpret_cast<bf16x8 *>(&sAB[b][0]); };
  auto sB = [&](int b) -> bf16x8 * { return reinterpret_cast<bf16x8 *>(&sAB[b][0]) + BM * kRowChunks; };
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WCOLS, wn = wave % WCOLS;
  const int li = lane & 31, lh = lane >> 5;
  const int ohw = a.OH * a.OW;
  const int hw = a.H * a.W;
  const int nk = (a.K + kBK16 - 1) / kBK16;
  const long n_tiles = (long)a.n_ptiles * a.n_mtiles * a.n_groups;
  const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.w), 0, a.w_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.in), 0, a.in_bytes, 0x00020000);

  auto tile_coords = [&](long tile, int &cg, int &m0, int &p0) { dense_tile_coords(a, BM, tile, cg, m0, p0); };

  // ---- addressing of the tile being FETCHED (recomputed when the fetch moves to a new tile) ----
  //  A: rows 32 q + tid / 8 of the tile, chunk tid % 8
  //  B: dense_common.h DenseB16Stage
  unsigned fa_row = 0u;              // byte offset of the lane's first A row, column 0
  DenseB16Stage<BMODE> bs;
  int f_cg = 0, f_m0 = 0, f_p0 = 0;
  auto fetch_setup = [&](long tile) {
    tile_coords(tile, f_cg, f_m0, f_p0);
    fa_row = (unsigned)(((size_t)f_cg * a.Mg + f_m0 + (tid >> 3)) * a.lda * 4);
    bs.setup(a, f_cg, f_p0, lane, ohw, hw);
  };
  // the staging registers: one k-step of this lane's share of both tiles, fp32 as loaded
  f32x4b ra[AQ][2];
  auto fetch = [&](int kstep) {
    const int k0 = kstep * kBK16;
    // A: 8 floats at column k0 + 8 (tid % 8); columns at or past lda are other rows' (or nothing): zeros
    const int ka = k0 + 8 * (tid & 7);
    const bool a_in = ka < a.lda;
#pragma unroll
    for (int q = 0; q < AQ; ++q) {
      const unsigned vq = fa_row + (unsigned)((32 * q * a.lda + ka) * 4);
      ra[q][0] = __builtin_bit_cast(f32x4b, __builtin_amdgcn_raw_buffer_load_b128(rA, (int)(a_in ? vq : kB16OOB), 0, 0));
      ra[q][1] = __builtin_bit_cast(f32x4b, __builtin_amdgcn_raw_buffer_load_b128(rA, (int)(a_in ? vq + 16u : kB16OOB), 0, 0));
    }
    bs.fetch(a, rB, k0, wave, hw);
  };
  // ... converted and written to buffer `buf`: one chunk per (row, 8 k)
  auto stage = [&](int buf) {
#pragma unroll
    for (int q = 0; q < AQ; ++q) {
      const float v[8] = {ra[q][0][0], ra[q][0][1], ra[q][0][2], ra[q][0][3], ra[q][1][0], ra[q][1][1], ra[q][1][2], ra[q][1][3]};
      sA(buf)[chunk_at(32 * q + (tid >> 3), tid & 7)] = pack8(v);
    }
    bs.stage(sB(buf), lane, wave);
  };

  f32x16 acc[2][NB];
  long tile = (long)blockIdx.x;
  if (tile >= n_tiles) return;
  fetch_setup(tile);
  fetch(0);
  stage(0);
  long f_tile = tile;             // tile of the step being fetched next
  int f_k = 1;                    // ... and its k-step
  if (f_k == nk) {
    f_tile += gridDim.x;
    f_k = 0;
    if (f_tile < n_tiles) fetch_setup(f_tile);
  }
  int buf = 0;
  for (; tile < n_tiles; tile += gridDim.x) {
    int cg, m0, p0;
    tile_coords(tile, cg, m0, p0);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < NB; ++j) acc[i][j] = f32x16{0};
    for (int ks = 0; ks < nk; ++ks, buf ^= 1) {
      // everyone's chunks of this step are in `buf`, and everyone is done with the other buffer (the last step's reads,
      // the last epilogue's staging)
      __syncthreads();
      const bool do_fetch = f_tile < n_tiles;
      // the next step's operands go out now and land under the matrix instructions below
      if (do_fetch) fetch(f_k);
      __builtin_amdgcn_sched_barrier(0);
      // lane (i, h) of 16-k group kk: A rows wm * 64 + {0, 32} + i, B columns wn * WN + 32 j + i, k = 16 kk + 8 h .. + 7;
      // the fragments of group kk + 1 are read while the instructions of group kk run
      const int ra0 = wm * 64 + li, cb0 = wn * WN + li;
      bf16x8 fa[2][2], fb[2][NB];
      auto read_frags = [&](int kk, int s) {
        fa[s][0] = sA(buf)[chunk_at(ra0, 2 * kk + lh)];
        fa[s][1] = sA(buf)[chunk_at(ra0 + 32, 2 * kk + lh)];
#pragma unroll
        for (int j = 0; j < NB; ++j) fb[s][j] = sB(buf)[chunk_at(cb0 + 32 * j, 2 * kk + lh)];
      };
      read_frags(0, 0);
#pragma unroll
      for (int kk = 0; kk < kBK16 / 16; ++kk) {
        const int s = kk & 1;
        if (kk + 1 < kBK16 / 16) read_frags(kk + 1, s ^ 1);
        __builtin_amdgcn_sched_barrier(0);      // (next group's LDS reads first, then this group's instructions)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[s][0], fb[s][j], acc[0][j], 0, 0, 0);
          acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[s][1], fb[s][j], acc[1][j], 0, 0, 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (do_fetch) {
        stage(buf ^ 1);
        if (++f_k == nk) {
          f_tile += gridDim.x;
          f_k = 0;
          if (f_tile < n_tiles) fetch_setup(f_tile);
        }
      }
    }

    // ---- epilogue (dense_common.h): staged through the buffer the tile's last k-step was read from ----
    dense_b16_epilogue<NB>(a, acc, cg, m0, p0, wm, wn, lane, ohw, &sAB[buf ^ 1][wave * 32 * WN]);
  }
}

// The launch launch_dense makes for a plan whose option "dense_math" is ESCOIN_MATH_BF16: the same argument checks, no
// allocation, no synchronisation (capturable into a graph).  The refusals and the tile plan are align_rules.h db16_plan's.
static int launch_dense_bf16(const escoin_plan *p, const float *bottom, const float *bias, float *top, int n_images,
                             hipStream_t stream) {
  const Geometry &g = p->g;
  const DenseArrays &dn = p->dense;
  if (!dn.ktab.get<void>() || !dn.w.get<void>()) return fail(ESCOIN_ESTATE, "dense kernel: plan has no dense weights");
  if (g.d.dil_h * (g.d.KH - 1) > 0x7FFE || g.d.dil_w * (g.d.KW - 1) > 0x7FFE)
    return fail(ESCOIN_EINVAL, "dense kernel: dilated kernel extent does not fit 15 bits");
  Db16Plan dp;
  const int groups = p->use_dense ? g.d.group : p->n_dense_groups;
  if (const LaunchVerdict v = db16_plan(g, p->is_f64, n_images, groups, tiled_device_cus(), &dp); !v.ok()) return fail(v.rc, v.error);
  DenseArgs a = {};
  a.in = bottom; a.w = dn.w.get<const float>(); a.bias = bias; a.out = top;
  a.ktab = dn.ktab.get<const int2>();
  a.n_images = n_images; a.C = g.d.C; a.H = g.d.H; a.W = g.d.W; a.M = g.d.M; a.OH = g.OH; a.OW = g.OW;
  a.pad_h = g.d.pad_h; a.pad_w = g.d.pad_w; a.stride_h = g.d.stride_h; a.stride_w = g.d.stride_w;
  a.Cg = g.Cg; a.Mg = g.Mg; a.K = g.kdim; a.lda = dense_lda(g.kdim); a.relu = g.d.fuse_relu;
  a.P = (int)((long)n_images * g.OH * g.OW);
  a.in_bytes = (unsigned)dp.in_bytes;
  a.w_bytes = (unsigned)dp.w_bytes;
  // the operand path and the store path by the fp32 kernel's predicates: stat "dense_variant" keeps its terms
  const bool pointwise = g.d.KH == 1 && g.d.KW == 1 && g.d.stride_h == 1 && g.d.stride_w == 1 && g.d.pad_h == 0 && g.d.pad_w == 0;
  const bool vec_b = pointwise && (g.d.H * g.d.W) % 4 == 0 && (reinterpret_cast<uintptr_t>(bottom) & 15) == 0 && a.P >= 4;
  a.vec_out = (g.OH * g.OW) % 4 == 0 && (reinterpret_cast<uintptr_t>(top) & 15) == 0;
  a.group_mask = p->use_dense ? ~0ull : p->dense_mask;
  a.n_ptiles = dp.n_ptiles;
  a.n_mtiles = dp.n_mtiles;
  a.n_groups = groups;
  dn.sk_used = false;
  dn.math_last = ESCOIN_MATH_BF16;
  dn.variant_last = (dp.bm == 64 ? 1 : 2) + 4 * (vec_b ? 1 : 0) + 8 * (a.vec_out ? 1 : 0) + 32;
  const dim3 grid((unsigned)dp.workgroups, 1, 1);
  if (dp.bm == 64) {
    if (vec_b) hipLaunchKernelGGL((escoin_dense_bf16_kernel<1, 1>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((escoin_dense_bf16_kernel<1, 0>), grid, dim3(256), 0, stream, a);
  } else {
    if (vec_b) hipLaunchKernelGGL((escoin_dense_bf16_kernel<2, 1>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((escoin_dense_bf16_kernel<2, 0>), grid, dim3(256), 0, stream, a);
  }
  ESCOIN_HIP_TRY(hipGetLastError());
  return ESCOIN_OK;
}

// (launch_dense reaches this through g_dense_bf16_launch, escoin_plan.h: a program that links the core's objects alone
// still links, and refuses the option there)
namespace {
__attribute__((used)) const bool g_registered = (g_dense_bf16_launch = launch_dense_bf16, true);
}  // namespace

}  // namespace escoin
