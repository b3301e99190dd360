// dense_sp24.hip -- the dense forward kernel for 2:4 structured-sparse weights (plan option "sp24"): the implicit GEMM of
// dense_bf16.hip,
//     C[Mg x P] = A[Mg x K] * B[K x P]   per conv group,   K = Cg*KH*KW,  P = N*OH*OW,
// on v_smfmac_f32_32x32x32_bf16: A keeps 2 of every 4 values along k plus a 2-bit position per kept value, and one issue
// does the k-work of two v_mfma_f32_32x32x16_bf16.  The weights stay in the plan's one fp32 matrix dense.w; which two
// columns of each aligned group of 4 are kept is the index table csr_tables.h sp24_index built at the align (one 16-bit word
// per row and run of 16 columns).  Products are exact products of the operands rounded to bf16 (nearest even), sums fp32,
// bias and ReLU fp32 in the epilogue -- the bf16 kernel's contract over the pattern's positions.
//
// The instruction (tools/probes/probe_smfmac.hip, one-hot A values against numbered B values on an MI355X):
//   * A, 8 bf16 per lane: lane l holds row l % 32; its values cover the 16 dense k 16 (l / 32) .. + 15 of the instruction's
//     32, two per group of 4, in k order.
//   * Index, one VGPR per lane: 16 bits are used, bits 0..15 with ABID = 0 and bits 16..31 with ABID = 1 (CBSZ = 0).  Field
//     i = bits 2 i + 1 .. 2 i is the position (0..3) of A value i inside its group i / 2: value i meets dense k
//     16 (l / 32) + 4 (i / 2) + field.  Fields need not differ or ascend for the instruction; the table's do.
//   * B, 16 bf16 per lane: lane l holds column l % 32; elements 0..7 are k 8 (l / 32) .. + 7 and elements 8..15 are
//     k 16 + 8 (l / 32) .. + 7 -- TWO runs of 8, the B fragments of two v_mfma_f32_32x32x16_bf16 side by side.
//   * C/D: the 32 x 32 layout of the dense instructions.
// Only which A value meets which B value matters, so the kernel numbers k to suit its staging: instruction kk (0, 1) of a
// k-step takes, for lane half h, the step's run 2 h + kk of 16 dense k (A), and for B lane half h the step's chunks of 8 k
// 2 kk + h and 4 + 2 kk + h -- the chunks the bf16 kernel reads, in its LDS layout.
//
// The frame is the bf16 kernel's and shared with it through dense_common.h: persistent workgroups (two per CU, four waves;
// BM = 128: waves 2 x 2, BM = 64 for Mg <= 64: waves 1 x 4), whole 128-pixel tiles, the group mask, B's staging ([p][64 k]
// rows of 128 bytes, pointwise or gathered through ktab with the border test, range-checked loads) and the epilogue.  The
// k-loop: steps of 64 dense k, one barrier each; the loads of step s + 1 go to registers before the matrix instructions of
// step s and are converted and written to the other LDS buffer after them; 2 instructions per 32 x 32 block and step.
//   * A staging: lane (row = tid / 2, h = tid % 2) of the first 2 BM lanes stages runs 2 h and 2 h + 1 of its row: 32
//     consecutive fp32 (eight 16-byte loads) and the two index words, which are adjacent in the table (one 4-byte load).  Per
//     kept value it picks one of the group's four with three v_cndmask on the field's two bits -- registers only -- rounds
//     with v_cvt_pk_bf16_f32 and writes two 16-byte chunks of the compressed tile A[m][32 kept], rows of 64 bytes.
//   * The index words go through LDS next to the tile, 8 bytes per row and k-step: the staging lane holds them anyway and
//     writes its 4 bytes; consumer lane (row, h) reads dword h = the words of runs 2 h (bits 0..15, ABID 0: instruction 0) and
//     2 h + 1 (bits 16..31, ABID 1: instruction 1).  Fetching them from memory in the consumers instead would load every word
//     three times (the staging lane and a lane in each of the two waves that share the row) and hold another step's worth
//     of registers; through LDS they ride on the barrier the tile needs anyway.
//   * Swizzle of the A tile (a_chunk_at): chunk c (0..3) of row r sits in slot c ^ ((r >> 2) & 3) of the row.  A fragment
//     read (ds_read_b128, 16 lanes = 16 consecutive rows at one logical chunk per pass): four rows fill 256 bytes = all 64
//     banks, so rows with equal r % 4 share banks -- and those four rows (r >> 2 = x .. x + 3) sit in four different slots:
//     all 64 banks once.  A staging write (16 lanes = 8 consecutive rows from a multiple of 8, logical chunks 2 h + j):
//     rows r and r + 4 share banks, r >> 2 = x (even) and x + 1; slots {j ^ x, j ^ x ^ 2} and {j ^ x ^ 1, j ^ x ^ 3}: all
//     different.  The index dwords are contiguous (row-major [row][2]): a read or write of 64 lanes covers 64 banks once.
//   * LDS: per buffer A 64 BM + index 8 BM + B 16 KiB = 25 KiB (BM = 128), padded to the epilogue's 32 KiB staging area;
//     two buffers = 64 KiB per workgroup, two workgroups per CU.
// Rows past K: B stages zeros there (dense_common.h); A past lda reads zeros and an index word of 0 (the descriptors' range
// checks); up to lda the matrix's own zero padding.  Filler positions of the table (groups with fewer than 2 entries) are
// multiplied by the matrix's 0: a non-finite activation there gives NaN; positions outside the table are never multiplied.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "align_rules.h"
#include "dense_common.h"
#include "escoin_plan.h"

namespace escoin {

typedef __bf16 bf16x16 __attribute__((ext_vector_type(16)));

static_assert(kBN == kDb16TileP && kDb16StepK == kB16StepK && kSp24StepKept == 32 && kSp24StepInstr == 2,
              "the swizzles and the staging maps are written for 128 x 64 tiles");
constexpr int kARowChunks = kSp24StepKept / 8;      // 16-byte chunks per row of the compressed A tile

// index (in chunks of 8 bf16) of logical chunk `chunk` of row `row` of the compressed A tile
__device__ __forceinline__ int a_chunk_at(int row, int chunk) { return row * kARowChunks + (chunk ^ ((row >> 2) & 3)); }

// the 8 values index word `w` keeps of a run of 16 (q0 .. q3: its 4 groups of 4), rounded to bf16
__device__ __forceinline__ float keep1(f32x4b q, unsigned w, int i) {
  const bool b0 = (w >> (2 * i)) & 1u, b1 = (w >> (2 * i + 1)) & 1u;
  const float lo = b0 ? q[1] : q[0], hi = b0 ? q[3] : q[2];
  return b1 ? hi : lo;
}
__device__ __forceinline__ bf16x8 keep8(f32x4b q0, f32x4b q1, f32x4b q2, f32x4b q3, unsigned w) {
  const f32x8 f = {keep1(q0, w, 0), keep1(q0, w, 1), keep1(q1, w, 2), keep1(q1, w, 3),
                   keep1(q2, w, 4), keep1(q2, w, 5), keep1(q3, w, 6), keep1(q3, w, 7)};
  return __builtin_convertvector(f, bf16x8);      // four v_cvt_pk_bf16_f32: round to nearest even, overflow to infinity
}

template <int WROWS, int BMODE>
__global__ void __launch_bounds__(256, 2) escoin_dense_sp24_kernel(DenseArgs a) {
  constexpr int BM = 64 * WROWS;
  constexpr int WCOLS = 4 / WROWS;           // waves along the pixel axis
  constexpr int WN = kBN / WCOLS;            // columns per wave: 64 or 32
  constexpr int NB = WN / 32;                // 32-column blocks per wave
  // one array per buffer: compressed A tile, index dwords, B tile; at least the epilogue's staging area (4 waves x 32 x WN floats)
  constexpr int kAChunks = BM * kARowChunks;
  constexpr int kIdxFloats = BM * 2;
  constexpr int kTileFloats = kAChunks * 4 + kIdxFloats + kBN * kB16RowChunks * 4;
  constexpr int kBufFloats = kTileFloats > 4 * 32 * WN ? kTileFloats : 4 * 32 * WN;
  __shared__ __attribute__((aligned(1024))) float sAB[2][kBufFloats];
  auto sA = [&](int b) -> bf16x8 * { return reinterpret_cast<bf16x8 *>(&sAB[b][0]); };
  auto sI = [&](int b) -> unsigned * { return reinterpret_cast<unsigned *>(&sAB[b][kAChunks * 4]); };
  auto sB = [&](int b) -> bf16x8 * { return reinterpret_cast<bf16x8 *>(&sAB[b][kAChunks * 4 + kIdxFloats]); };
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WCOLS, wn = wave % WCOLS;
  const int li = lane & 31, lh = lane >> 5;
  const int ohw = a.OH * a.OW;
  const int hw = a.H * a.W;
  const int nk = (a.K + kB16StepK - 1) / kB16StepK;
  const long n_tiles = (long)a.n_ptiles * a.n_mtiles * a.n_groups;
  const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.w), 0, a.w_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.in), 0, a.in_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rI = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short *>(a.sp_idx), 0, a.sp_bytes, 0x00020000);

  // ---- addressing of the tile being FETCHED (recomputed when the fetch moves to a new tile) ----
  //  A: row tid / 2 of the tile, runs 2 (tid % 2) and 2 (tid % 2) + 1 of the step -- the waves that hold rows of the tile
  //  B: dense_common.h DenseB16Stage
  const bool a_lane = tid < 2 * BM;       // (wave-uniform)
  const int srow = tid >> 1, sh = tid & 1;
  unsigned fa_row = 0u;              // byte offset of the lane's A row, column 0
  unsigned fi_row = 0u;              // byte offset of the row's first index word
  DenseB16Stage<BMODE> bs;
  int f_cg = 0, f_m0 = 0, f_p0 = 0;
  auto fetch_setup = [&](long tile) {
    dense_tile_coords(a, BM, tile, f_cg, f_m0, f_p0);
    const size_t row = (size_t)f_cg * a.Mg + f_m0 + srow;
    fa_row = (unsigned)(row * a.lda * 4);
    fi_row = (unsigned)(row * (a.lda / 16) * 2);
    bs.setup(a, f_cg, f_p0, lane, ohw, hw);
  };
  // the staging registers: one k-step of this lane's share of both tiles, fp32 as loaded, and the two index words
  f32x4b ra[8];
  unsigned ri = 0u;
  auto fetch = [&](int kstep) {
    const int k0 = kstep * kB16StepK;
    if (a_lane) {
      // 32 floats at column k0 + 32 sh; lda is a multiple of 32: the lane's columns are all inside the row or all past it,
      // where the loads deliver zeros and the index word 0
      const int ka = k0 + 32 * sh;
      const bool a_in = ka < a.lda;
      const unsigned va = fa_row + (unsigned)(ka * 4);
#pragma unroll
      for (int q = 0; q < 8; ++q)
        ra[q] = __builtin_bit_cast(f32x4b, __builtin_amdgcn_raw_buffer_load_b128(rA, (int)(a_in ? va + 16u * q : kB16OOB), 0, 0));
      ri = __builtin_amdgcn_raw_buffer_load_b32(rI, (int)(a_in ? fi_row + (unsigned)(ka / 16 * 2) : kB16OOB), 0, 0);
    }
    bs.fetch(a, rB, k0, wave, hw);
  };
  // ... selected, converted and written to buffer `buf`
  auto stage = [&](int buf) {
    if (a_lane) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
        sA(buf)[a_chunk_at(srow, 2 * sh + j)] = keep8(ra[4 * j], ra[4 * j + 1], ra[4 * j + 2], ra[4 * j + 3], ri >> (16 * j));
      sI(buf)[2 * srow + sh] = ri;
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
      // lane (i, h): A rows wm * 64 + {0, 32} + i, B columns wn * WN + 32 j + i; the fragments of instruction 1 are read
      // while the instructions 0 run
      const int ra0 = wm * 64 + li, cb0 = wn * WN + li;
      const int ix0 = (int)sI(buf)[2 * ra0 + lh], ix1 = (int)sI(buf)[2 * (ra0 + 32) + lh];
      bf16x8 fa[2][2];
      bf16x16 fb[2][NB];
      auto read_frags = [&](int kk) {
        fa[kk][0] = sA(buf)[a_chunk_at(ra0, 2 * lh + kk)];
        fa[kk][1] = sA(buf)[a_chunk_at(ra0 + 32, 2 * lh + kk)];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          const bf16x8 b0 = sB(buf)[chunk_at(cb0 + 32 * j, 2 * kk + lh)], b1 = sB(buf)[chunk_at(cb0 + 32 * j, 4 + 2 * kk + lh)];
          fb[kk][j] = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
        }
      };
      read_frags(0);
      read_frags(1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        acc[0][j] = __builtin_amdgcn_smfmac_f32_32x32x32_bf16(fa[0][0], fb[0][j], acc[0][j], ix0, 0, 0);
        acc[1][j] = __builtin_amdgcn_smfmac_f32_32x32x32_bf16(fa[0][1], fb[0][j], acc[1][j], ix1, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        acc[0][j] = __builtin_amdgcn_smfmac_f32_32x32x32_bf16(fa[1][0], fb[1][j], acc[0][j], ix0, 0, 1);
        acc[1][j] = __builtin_amdgcn_smfmac_f32_32x32x32_bf16(fa[1][1], fb[1][j], acc[1][j], ix1, 0, 1);
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

// The launch launch_dense makes for a plan whose option "sp24" is on and whose index table exists: the bf16 launch's argument
// checks, no allocation, no synchronisation (capturable into a graph).  The refusals and the tile plan are align_rules.h
// sp24_plan's.
static int launch_dense_sp24(const escoin_plan *p, const float *bottom, const float *bias, float *top, int n_images,
                             hipStream_t stream) {
  const Geometry &g = p->g;
  const DenseArrays &dn = p->dense;
  if (!dn.ktab.get<void>() || !dn.w.get<void>() || !dn.sp_idx.get<void>()) return fail(ESCOIN_ESTATE, "2:4 dense kernel: plan has no dense weights or no index table");
  if (g.d.dil_h * (g.d.KH - 1) > 0x7FFE || g.d.dil_w * (g.d.KW - 1) > 0x7FFE)
    return fail(ESCOIN_EINVAL, "dense kernel: dilated kernel extent does not fit 15 bits");
  Sp24Plan sp;
  const int groups = p->use_dense ? g.d.group : p->n_dense_groups;
  if (const LaunchVerdict v = sp24_plan(g, p->is_f64, n_images, groups, tiled_device_cus(), &sp); !v.ok()) return fail(v.rc, v.error);
  if (sp.idx_bytes != dn.sp_idx.bytes() || sp.idx_row_words * 16 != dense_lda(g.kdim))
    return fail(ESCOIN_ESTATE, "2:4 dense kernel: the index table does not match the weight matrix");
  const Db16Plan &dp = sp.t;
  DenseArgs a = {};
  a.in = bottom; a.w = dn.w.get<const float>(); a.bias = bias; a.out = top;
  a.ktab = dn.ktab.get<const int2>();
  a.sp_idx = dn.sp_idx.get<const unsigned short>();
  a.n_images = n_images; a.C = g.d.C; a.H = g.d.H; a.W = g.d.W; a.M = g.d.M; a.OH = g.OH; a.OW = g.OW;
  a.pad_h = g.d.pad_h; a.pad_w = g.d.pad_w; a.stride_h = g.d.stride_h; a.stride_w = g.d.stride_w;
  a.Cg = g.Cg; a.Mg = g.Mg; a.K = g.kdim; a.lda = dense_lda(g.kdim); a.relu = g.d.fuse_relu;
  a.P = (int)((long)n_images * g.OH * g.OW);
  a.in_bytes = (unsigned)dp.in_bytes;
  a.w_bytes = (unsigned)dp.w_bytes;
  a.sp_bytes = (unsigned)sp.idx_bytes;
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
  dn.sp24_last = true;
  dn.variant_last = (dp.bm == 64 ? 1 : 2) + 4 * (vec_b ? 1 : 0) + 8 * (a.vec_out ? 1 : 0) + 64;
  const dim3 grid((unsigned)dp.workgroups, 1, 1);
  if (dp.bm == 64) {
    if (vec_b) hipLaunchKernelGGL((escoin_dense_sp24_kernel<1, 1>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((escoin_dense_sp24_kernel<1, 0>), grid, dim3(256), 0, stream, a);
  } else {
    if (vec_b) hipLaunchKernelGGL((escoin_dense_sp24_kernel<2, 1>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((escoin_dense_sp24_kernel<2, 0>), grid, dim3(256), 0, stream, a);
  }
  ESCOIN_HIP_TRY(hipGetLastError());
  return ESCOIN_OK;
}

// (launch_dense reaches this through g_dense_sp24_launch, escoin_plan.h: a program that links the core's objects alone
// still links, and refuses the option there)
namespace {
__attribute__((used)) const bool g_registered = (g_dense_sp24_launch = launch_dense_sp24, true);
}  // namespace

}  // namespace escoin
