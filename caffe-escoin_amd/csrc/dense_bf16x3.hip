// dense_bf16x3.hip -- the dense forward kernel's split-bf16 math mode (plan option "dense_split" = 1; BF16x3 elsewhere): the
// implicit GEMM of dense_mfma.hip,
//     C[Mg x P] = A[Mg x K] * B[K x P]   per conv group,   K = Cg*KH*KW,  P = N*OH*OW,
// with every fp32 operand split into two bf16 terms on its way into LDS -- hi = rne(v), lo = rne(v - hi), dense_common.h
// split8 -- and three of the four term products, hi*hi, hi*lo and lo*hi, summed into the same fp32 accumulators by
// v_mfma_f32_32x32x16_bf16.  The dropped lo*lo and the terms' own rounding are below 2^-16 |w||x| per product (the
// derivation is in include/escoin.h): the fp32 kernel's order of error at the bf16 kernel's operand traffic from memory.
// The blobs and the plan's one weight matrix stay fp32 and are read as they are; bias and ReLU are applied in fp32.
//
// From dense_bf16.hip / dense_common.h: the tiles, the persistent workgroups (two per CU, four waves each; BM = 128: waves
// 2 x 2, 64 x 64 outputs each; BM = 64 for Mg <= 64: waves 1 x 4, 64 x 32 each), the group mask, the `ktab` decode, the
// range-checked buffer loads that deliver the padding's zeros (a zero splits into two zeros), the swizzle and the epilogue.
// The k-loop and the LDS layout are this kernel's:
//   * k-steps of 32, one barrier each, across tile boundaries.  LDS keeps the bf16 kernel's footprint -- two buffers of
//     (BM + 128) rows of 128 bytes, 2 x 32 KiB at BM = 128 -- so two workgroups per CU stay resident and the epilogue's staging
//     area is unchanged: a row's 8 chunks of 8 bf16 now hold 32 k twice.  The 8 k of k-chunk kc (k = 8 kc .. 8 kc + 7 of the
//     step, kc = 0 .. 3) are logical chunk 2 kc (hi terms) and 2 kc + 1 (lo terms) of the row.
//   * The loads of step s + 1 go out to registers before the matrix instructions of step s; they are split and written to
//     the other buffer after them.  An operand is split once, by the lane that stages it.
//   * A staging: a lane loads 8 consecutive k of one row (two 16-byte loads; 4 lanes cover a row's 128 bytes, the workgroup
//     64 rows per pass, BM / 64 passes) and writes two chunks.  B staging (DenseSplitStage): a lane owns one pixel of each
//     half of the tile and the 8 k of its wave's k-chunk -- eight 4-byte loads, coalesced along p -- and writes two chunks.
//   * Per step and 32 x 32 block: two 16-k groups of three instructions (hi hi, hi lo, lo hi; A term first), issued term by
//     term over the wave's blocks so that no instruction waits for the one before it.  Lane (i, h) of group kk holds k-chunk
//     2 kk + h of row / column i: four ds_read_b128 per operand row block and group.  The fragments of group 1 are read
//     while the instructions of group 0 run.
// Banks (chunk_at: chunk c of row r in slot c ^ ((r >> 1) & 7); a row is 32 of the 64 banks, even rows in one half, odd rows
// in the other; a 16-byte access is served 16 lanes at a time):
//   * fragment reads, and B staging writes (64 consecutive pixels): 16 consecutive rows at ONE logical chunk -- 8 even rows
//     in 8 different slots of one half, 8 odd rows likewise: all 64 banks once, whichever chunk.  As in the bf16 kernel.
//   * A staging writes: 16 consecutive lanes are 4 consecutive rows r .. r + 3 (r % 4 == 0) times 4 k-chunks at one term.
//     With the hi terms in chunks 0 - 3 and the lo terms in 4 - 7 this CONFLICTS two ways: rows r and r + 2 lie in the same
//     bank half, their swizzles t = r / 2 and t + 1 differ in bit 0 only, and {0,1,2,3} ^ t is the same set of four slots for
//     both.  Interleaving the terms (the layout above) removes it: the four chunks of one term are {0,2,4,6} + term, and
//     {0,2,4,6} ^ t and {0,2,4,6} ^ (t + 1) are the even and the odd slots.  Two rows per half, four slots each, disjoint:
//     all 64 banks once.
// Rows past K: B stages zeros there (ktab entries past K fail the border test; the pointwise path compares k with K), and
// so does A (up to lda the matrix's own zero padding).  K rounded up to 32 -- lda, and ktab's length -- is a whole number of
// steps: nothing is read past either.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "align_rules.h"
#include "dense_common.h"
#include "escoin_plan.h"

namespace escoin {

constexpr int kBK3 = kDb3StepK;                  // k per step
static_assert(kBN == kDb16TileP && kBK3 == 32 && kB16RowChunks == 2 * kBK3 / 8, "a 128-byte LDS row holds one step's k as two bf16 terms");

// BMODE: how the B tile's elements are addressed (dense_common.h DenseB16Stage)
template <int WROWS, int BMODE>
__global__ void __launch_bounds__(256, 2) escoin_dense_bf16x3_kernel(DenseArgs a) {
  constexpr int BM = 64 * WROWS;
  constexpr int WCOLS = 4 / WROWS;           // waves along the pixel axis
  constexpr int WN = kBN / WCOLS;            // columns per wave: 64 or 32
  constexpr int NB = WN / 32;                // 32-column blocks per wave
  constexpr int AQ = BM / 64;                // A rows a lane stages per k-step: rows 64 q + tid / 4, k-chunk tid % 4
  // one array per buffer: A tile then B tile, in bf16 (the epilogue reuses a whole buffer as its fp32 staging area, as in
  // dense_bf16.hip)
  constexpr int kBufChunks = (BM + kBN) * kB16RowChunks;
  constexpr int kBufFloats = kBufChunks * 4;
  static_assert(4 * 32 * WN <= kBufFloats, "the epilogue's staging area is one buffer");
  __shared__ __attribute__((aligned(1024))) float sAB[2][kBufFloats];
  auto sA = [&](int b) -> bf16x8 * { return reinterpret_cast<bf16x8 *>(&sAB[b][0]); };
  auto sB = [&](int b) -> bf16x8 * { return reinterpret_cast<bf16x8 *>(&sAB[b][0]) + BM * kB16RowChunks; };
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WCOLS, wn = wave % WCOLS;
  const int li = lane & 31, lh = lane >> 5;
  const int ohw = a.OH * a.OW;
  const int hw = a.H * a.W;
  const int nk = (a.K + kBK3 - 1) / kBK3;
  const long n_tiles = (long)a.n_ptiles * a.n_mtiles * a.n_groups;
  const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.w), 0, a.w_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.in), 0, a.in_bytes, 0x00020000);

  // ---- addressing of the tile being FETCHED (recomputed when the fetch moves to a new tile) ----
  unsigned fa_row = 0u;              // byte offset of the lane's first A row, column 0
  DenseSplitStage<BMODE> bs;
  int f_cg = 0, f_m0 = 0, f_p0 = 0;
  auto fetch_setup = [&](long tile) {
    dense_tile_coords(a, BM, tile, f_cg, f_m0, f_p0);
    fa_row = (unsigned)(((size_t)f_cg * a.Mg + f_m0 + (tid >> 2)) * a.lda * 4);
    bs.setup(a, f_cg, f_p0, lane, ohw, hw);
  };
  // the staging registers: one k-step of this lane's share of both tiles, fp32 as loaded
  f32x4b ra[AQ][2];
  auto fetch = [&](int kstep) {
    const int k0 = kstep * kBK3;
    // A: 8 floats at column k0 + 8 (tid % 4), inside the row (k0 + 32 <= lda); rows past the matrix: the descriptor's zeros
    const int ka = k0 + 8 * (tid & 3);
#pragma unroll
    for (int q = 0; q < AQ; ++q) {
      const unsigned vq = fa_row + (unsigned)((64 * q * a.lda + ka) * 4);
      ra[q][0] = __builtin_bit_cast(f32x4b, __builtin_amdgcn_raw_buffer_load_b128(rA, (int)vq, 0, 0));
      ra[q][1] = __builtin_bit_cast(f32x4b, __builtin_amdgcn_raw_buffer_load_b128(rA, (int)(vq + 16u), 0, 0));
    }
    bs.fetch32(a, rB, k0, wave, hw);
  };
  // ... split and written to buffer `buf`: two chunks per (row, 8 k)
  auto stage = [&](int buf) {
#pragma unroll
    for (int q = 0; q < AQ; ++q) {
      const float v[8] = {ra[q][0][0], ra[q][0][1], ra[q][0][2], ra[q][0][3], ra[q][1][0], ra[q][1][1], ra[q][1][2], ra[q][1][3]};
      bf16x8 hi, lo;
      split8(v, hi, lo);
      sA(buf)[chunk_at(64 * q + (tid >> 2), 2 * (tid & 3))] = hi;
      sA(buf)[chunk_at(64 * q + (tid >> 2), 2 * (tid & 3) + 1)] = lo;
    }
    bs.stage_split(sB(buf), lane, wave);
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
    dense_tile_coords(a, BM, tile, cg, m0, p0);
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
      // lane (i, h) of 16-k group kk: A rows wm * 64 + {0, 32} + i, B columns wn * WN + 32 j + i, k-chunk 2 kk + h, both terms
      const int ra0 = wm * 64 + li, cb0 = wn * WN + li;
      bf16x8 fa[2][2][2], fb[2][NB][2];      // [group][block][term]
      auto read_frags = [&](int kk) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int c = 2 * (2 * kk + lh) + t;
          fa[kk][0][t] = sA(buf)[chunk_at(ra0, c)];
          fa[kk][1][t] = sA(buf)[chunk_at(ra0 + 32, c)];
#pragma unroll
          for (int j = 0; j < NB; ++j) fb[kk][j][t] = sB(buf)[chunk_at(cb0 + 32 * j, c)];
        }
      };
      read_frags(0);
#pragma unroll
      for (int kk = 0; kk < kBK3 / 16; ++kk) {
        if (kk + 1 < kBK3 / 16) read_frags(kk + 1);
        __builtin_amdgcn_sched_barrier(0);      // (next group's LDS reads first, then this group's instructions)
#pragma unroll
        for (int term = 0; term < 3; ++term) {
          const int ta = term >> 1, tb = term & 1;      // (hi, hi), (hi, lo), (lo, hi)
#pragma unroll
          for (int j = 0; j < NB; ++j) {
            acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[kk][0][ta], fb[kk][j][tb], acc[0][j], 0, 0, 0);
            acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[kk][1][ta], fb[kk][j][tb], acc[1][j], 0, 0, 0);
          }
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

// The launch launch_dense makes for a plan whose option "dense_split" is 1: launch_dense_bf16's argument checks, no
// allocation, no synchronisation (capturable into a graph).  The refusals and the tile plan are align_rules.h db3_plan's.
static int launch_dense_bf16x3(const escoin_plan *p, const float *bottom, const float *bias, float *top, int n_images,
                               hipStream_t stream) {
  const Geometry &g = p->g;
  const DenseArrays &dn = p->dense;
  if (!dn.ktab.get<void>() || !dn.w.get<void>()) return fail(ESCOIN_ESTATE, "dense kernel: plan has no dense weights");
  if (g.d.dil_h * (g.d.KH - 1) > 0x7FFE || g.d.dil_w * (g.d.KW - 1) > 0x7FFE)
    return fail(ESCOIN_EINVAL, "dense kernel: dilated kernel extent does not fit 15 bits");
  Db16Plan dp;
  const int groups = p->use_dense ? g.d.group : p->n_dense_groups;
  if (const LaunchVerdict v = db3_plan(g, p->is_f64, n_images, groups, tiled_device_cus(), &dp); !v.ok()) return fail(v.rc, v.error);
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
  dn.split_last = true;
  dn.variant_last = (dp.bm == 64 ? 1 : 2) + 4 * (vec_b ? 1 : 0) + 8 * (a.vec_out ? 1 : 0) + 128;
  const dim3 grid((unsigned)dp.workgroups, 1, 1);
  if (dp.bm == 64) {
    if (vec_b) hipLaunchKernelGGL((escoin_dense_bf16x3_kernel<1, 1>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((escoin_dense_bf16x3_kernel<1, 0>), grid, dim3(256), 0, stream, a);
  } else {
    if (vec_b) hipLaunchKernelGGL((escoin_dense_bf16x3_kernel<2, 1>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((escoin_dense_bf16x3_kernel<2, 0>), grid, dim3(256), 0, stream, a);
  }
  ESCOIN_HIP_TRY(hipGetLastError());
  return ESCOIN_OK;
}

// (launch_dense reaches this through g_dense_split_launch, escoin_plan.h: a program that links the core's objects alone
// still links, and refuses the option there)
namespace {
__attribute__((used)) const bool g_registered = (g_dense_split_launch = launch_dense_bf16x3, true);
}  // namespace

}  // namespace escoin
