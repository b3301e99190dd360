// dense_common.h -- what the dense forward kernels (dense_mfma.hip: fp32 products; dense_bf16.hip: plan option
// "dense_math" = ESCOIN_MATH_BF16; dense_sp24.hip: plan option "sp24"; dense_bf16x3.hip: plan option "dense_split") share:
// the GEMM view's pixel tile, the launch's argument block, and -- between the kernels that multiply bf16 -- the tile walk, the
// B tile's staging and the epilogue.
#pragma once
#include <hip/hip_runtime.h>

#include "escoin_plan.h"

namespace escoin {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4d __attribute__((ext_vector_type(4)));

constexpr int kBN = 128;      // pixels per output tile

struct DenseArgs {
  const float *__restrict__ in;
  const float *__restrict__ w;     // dense (M + 128) x lda, zero-padded: rows of lda = K rounded up to 32
  const float *__restrict__ bias;
  const int2 *__restrict__ ktab;   // [K rounded up to 32]: {element offset of tap k in the image, dy | dx << 16}
  float *__restrict__ out;
  int n_images, C, H, W, M, OH, OW;
  int pad_h, pad_w, stride_h, stride_w;
  int Cg, Mg, K, lda, P, relu;
  int n_ptiles, n_mtiles, n_groups;        // tiles: pixel x channel x conv group (of this launch)
  unsigned in_bytes, w_bytes;              // buffer descriptor ranges
  int vec_out;                             // OH*OW % 4 == 0 and top 16-byte aligned: 16-byte stores through LDS
  unsigned long long group_mask;           // conv groups this launch covers (all ones: every group)
  unsigned long long *prof;                // ESCOIN_STAMPS builds: stamp profile [workgroup][wave][8] (ESC_DPROF)
  // stream-K (STREAMK instantiations): every workgroup takes an equal, contiguous run of (tile, k-step) units;
  // a tile cut by a run boundary is finished by the workgroup holding its last k-steps, which adds the others'
  // partial accumulators from `sk_ws` ([workgroup][wave][16 quads][64 lanes] floats x 4) once their `sk_flag`
  // words (zeroed by the launch function before every launch) carry 1
  float *sk_ws;
  unsigned *sk_flag;     // [0 .. gridDim.x): published flags; [gridDim.x]: set when a bounded spin gave up
  unsigned *sk_fail;     // the same give-up, sticky, in pinned HOST memory: the next escoin_forward on the plan fails loudly
  // dense_sp24.hip: the 2:4 index table (csr_tables.h sp24_index), one 16-bit word per (row, 16 columns), and its bytes
  const unsigned short *__restrict__ sp_idx;
  unsigned sp_bytes;
};

// ---- shared by the kernels that multiply bf16 (dense_bf16.hip, dense_sp24.hip) ------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4b __attribute__((ext_vector_type(4)));

constexpr int kB16StepK = 64;                     // k per step (align_rules.h kDb16StepK)
constexpr int kB16RowChunks = kB16StepK / 8;      // 16-byte chunks per 128-byte LDS row
constexpr unsigned kB16OOB = 0xFFFFFFF0u;         // a byte offset no descriptor of these kernels covers: the load delivers zero

// index (in chunks of 8 bf16) of logical chunk `chunk` of row `row` of a tile of 128-byte rows
__device__ __forceinline__ int chunk_at(int row, int chunk) { return row * kB16RowChunks + (chunk ^ ((row >> 1) & 7)); }

__device__ __forceinline__ bf16x8 pack8(const float (&v)[8]) {
  const f32x8 f = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]};
  return __builtin_convertvector(f, bf16x8);      // four v_cvt_pk_bf16_f32: round to nearest even, overflow to infinity
}

// tile number -> conv group, first row, first pixel (tiles of bm x kBN outputs: channel tiles fastest, then pixel tiles)
__device__ __forceinline__ void dense_tile_coords(const DenseArgs &a, int bm, long tile, int &cg, int &m0, int &p0) {
  const int mt = (int)(tile % a.n_mtiles);
  const long r = tile / a.n_mtiles;
  const int pt = (int)(r % a.n_ptiles);
  const int gsel = (int)(r / a.n_ptiles);
  cg = a.group_mask == ~0ull ? gsel : nth_set_bit(a.group_mask, gsel);
  m0 = mt * bm;
  p0 = pt * kBN;
}

// The B tile's staging, [p][64 k] in bf16: a lane owns ONE pixel of each half of the tile (p0 + 64 half + lane) and the 16 k
// of the step that its wave covers (chunks 2 wave + cc, cc = 0, 1) -- sixteen 4-byte loads per half, each coalesced across
// the wave along p.  BMODE: how the elements are addressed --
//   0  gathered through ktab with the border test (any kernel / stride / padding / dilation)
//   1  pointwise (the fp32 kernel's predicate: 1x1, stride 1, no padding, H*W % 4 == 0, bottom 16-byte aligned): row k of
//      the column matrix is channel k of the bottom blob
template <int BMODE>
struct DenseB16Stage {
  unsigned pix[2] = {0u, 0u};      // byte offset of the lane's pixel (window origin) in the blob
  int ih0[2] = {0, 0}, iw0[2] = {0, 0};
  float rb[2][2][8];               // [half][cc][k]: one k-step of the lane's share, fp32 as loaded

  // the tile being FETCHED moved to conv group cg, first pixel p0
  __device__ __forceinline__ void setup(const DenseArgs &a, int cg, int p0, int lane, int ohw, int hw) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int p = min(p0 + 64 * half + lane, a.P - 1);
      const int n = p / ohw, rem = p - n * ohw;
      if (BMODE == 1) {
        pix[half] = (unsigned)((((size_t)n * a.C + (size_t)cg * a.Cg) * hw + rem) * 4);
      } else {
        const int oh = rem / a.OW, ow = rem - oh * a.OW;
        ih0[half] = oh * a.stride_h - a.pad_h;
        iw0[half] = ow * a.stride_w - a.pad_w;
        pix[half] = (unsigned)((((long)n * a.C + (long)cg * a.Cg) * hw + (long)ih0[half] * a.W + iw0[half]) * 4);
      }
    }
  }
  // the loads of the step that begins at column k0
  __device__ __forceinline__ void fetch(const DenseArgs &a, __amdgpu_buffer_rsrc_t rB, int k0, int wave, int hw) {
    const int kw = k0 + 16 * wave;
    if (BMODE == 1) {
#pragma unroll
      for (int cc = 0; cc < 2; ++cc)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int k = kw + 8 * cc + e;
          // rows past K are channels of the next conv group, of the next image or memory past the blob: zeros
          const unsigned ko = (unsigned)k * (unsigned)hw * 4u;
#pragma unroll
          for (int half = 0; half < 2; ++half)
            rb[half][cc][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rB, (int)(k < a.K ? pix[half] + ko : kB16OOB), 0, 0));
        }
    } else {
      // this wave's 16 taps of the step: 128 contiguous bytes at a wave-uniform address; the table ends at lda (= K rounded
      // up to 32, a multiple of 16: a wave's taps are all inside it or all past it)
      const bool in_tab = kw < a.lda;
      const int4 *tp = reinterpret_cast<const int4 *>(a.ktab + (in_tab ? kw : 0));
#pragma unroll
      for (int cc = 0; cc < 2; ++cc)
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) {
          int4 t = {0, 0x7FFF7FFF, 0, 0x7FFF7FFF};
          if (in_tab) t = tp[4 * cc + e2];
#pragma unroll
          for (int o = 0; o < 2; ++o) {
            const int toff = o ? t.z : t.x, tdyx = o ? t.w : t.y;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
              const int ih = ih0[half] + (tdyx & 0xFFFF), iw = iw0[half] + (tdyx >> 16);
              const bool ok = (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W;
              rb[half][cc][2 * e2 + o] =
                  __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rB, (int)(ok ? pix[half] + (unsigned)(toff * 4) : kB16OOB), 0, 0));
            }
          }
        }
    }
  }
  // ... converted and written to the B tile at sB: one chunk per (pixel, 8 k)
  __device__ __forceinline__ void stage(bf16x8 *sB, int lane, int wave) const {
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) sB[chunk_at(64 * half + lane, 2 * wave + cc)] = pack8(rb[half][cc]);
  }
};

// ---- dense_bf16x3.hip (plan option "dense_split"): every fp32 operand as two bf16 terms ----------------------------------
// hi = rne(v), lo = rne(v - float(hi)): the subtraction is exact (hi is v's leading 8 bits), so |v - hi - lo| <= 2^-18 |v|
// while lo does not underflow.  A zero gives two zeros; a value past bf16's largest finite one gives hi = +-inf and a lo of
// the other sign (NaN where v itself is infinite).
__device__ __forceinline__ void split8(const float (&v)[8], bf16x8 &hi, bf16x8 &lo) {
  const f32x8 f = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]};
  hi = __builtin_convertvector(f, bf16x8);       // four v_cvt_pk_bf16_f32, as pack8
  // float(hi) from the packed pairs -- a shift for the low half, a mask for the high one -- so that hi stays packed
  const u32x4d hu = __builtin_bit_cast(u32x4d, hi);
  f32x8 d;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    d[2 * p] = v[2 * p] - __builtin_bit_cast(float, hu[p] << 16);
    d[2 * p + 1] = v[2 * p + 1] - __builtin_bit_cast(float, hu[p] & 0xFFFF0000u);
  }
  lo = __builtin_convertvector(d, bf16x8);
}

// The B tile's staging in k-steps of 32, [p][32 k hi and lo]: the pixels and their addressing are DenseB16Stage's (setup);
// a lane owns the same two pixels and the 8 k of the step that its wave covers (k-chunk `wave`) -- eight 4-byte loads per
// half -- and writes two chunks per pixel: the hi terms at logical chunk 2 wave, the lo terms at 2 wave + 1.  A step never
// reaches past ktab's end (K rounded up to 32 is a whole number of steps).
template <int BMODE>
struct DenseSplitStage : DenseB16Stage<BMODE> {
  float rs[2][8];                  // [half][k]: one k-step of the lane's share, fp32 as loaded

  __device__ __forceinline__ void fetch32(const DenseArgs &a, __amdgpu_buffer_rsrc_t rB, int k0, int wave, int hw) {
    const int kw = k0 + 8 * wave;
    if (BMODE == 1) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        // rows past K are channels of the next conv group, of the next image or memory past the blob: zeros
        const unsigned ko = (unsigned)(kw + e) * (unsigned)hw * 4u;
#pragma unroll
        for (int half = 0; half < 2; ++half)
          rs[half][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rB, (int)(kw + e < a.K ? this->pix[half] + ko : kB16OOB), 0, 0));
      }
    } else {
      // this wave's 8 taps of the step: 64 contiguous bytes at a wave-uniform address, inside the table (kw < lda)
      const int4 *tp = reinterpret_cast<const int4 *>(a.ktab + kw);
#pragma unroll
      for (int e2 = 0; e2 < 4; ++e2) {
        const int4 t = tp[e2];
#pragma unroll
        for (int o = 0; o < 2; ++o) {
          const int toff = o ? t.z : t.x, tdyx = o ? t.w : t.y;
#pragma unroll
          for (int half = 0; half < 2; ++half) {
            const int ih = this->ih0[half] + (tdyx & 0xFFFF), iw = this->iw0[half] + (tdyx >> 16);
            const bool ok = (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W;
            rs[half][2 * e2 + o] =
                __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rB, (int)(ok ? this->pix[half] + (unsigned)(toff * 4) : kB16OOB), 0, 0));
          }
        }
      }
    }
  }
  // ... split and written to the B tile at sB: two chunks per (pixel, 8 k)
  __device__ __forceinline__ void stage_split(bf16x8 *sB, int lane, int wave) const {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      bf16x8 hi, lo;
      split8(rs[half], hi, lo);
      sB[chunk_at(64 * half + lane, 2 * wave)] = hi;
      sB[chunk_at(64 * half + lane, 2 * wave + 1)] = lo;
    }
  }
};

// The epilogue (the fp32 kernel's) of a wave's 64 x (32 NB) outputs at rows m0 + 64 wm, pixels p0 + 32 NB wn of conv group cg.
// C/D layout: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).  `stg`: the wave's 32 x (32 NB) floats of
// LDS for the 16-byte store path (a.vec_out), in a buffer nobody reads any more once the barrier inside has been passed.
template <int NB>
__device__ __forceinline__ void dense_b16_epilogue(const DenseArgs &a, const f32x16 (&acc)[2][NB], int cg, int m0, int p0, int wm,
                                                   int wn, int lane, int ohw, float *stg) {
  constexpr int WN = 32 * NB;
  const int li = lane & 31, lh = lane >> 5;
  // The bias of the lane's 32 rows is fetched in one go and pinned down: a load still pending when the stores start
  // makes the compiler wait for the previous store in front of every one of them.
  float bv[2][16];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int m = m0 + wm * 64 + 32 * i + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
      bv[i][reg] = (a.bias && m < a.Mg) ? a.bias[cg * a.Mg + m] : 0.f;
    }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) asm volatile("" : "+v"(bv[i][reg]));
  if (a.vec_out) {
    // Output rows of whole pixel quads (OH*OW % 4 == 0): transposed through LDS and stored 16 bytes per lane.  Staging
    // area: the buffer the tile's last k-step was read from (the other one holds the next tile's first step); a barrier
    // says everybody is done reading it, the barrier at the next k-step's top that everybody is done with the staging.
    // A wave transposes its own 32 x WN half-tiles: no cross-wave traffic.
    __syncthreads();
    constexpr int kQPR = WN / 4;                     // quads per staged row
    constexpr int kRowsPerIt = 64 / kQPR;            // rows one 64-lane read covers
    const int c4 = lane % kQPR, r0 = lane / kQPR;
    const int pq = p0 + wn * WN + 4 * c4;
    const int nq = pq / ohw, rq = pq - nq * ohw;
    float *oq = a.out + ((size_t)nq * a.M + (size_t)cg * a.Mg) * ohw + rq;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int row = (reg & 3) + 8 * (reg >> 2) + 4 * lh;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          float v = acc[i][j][reg] + bv[i][reg];
          if (a.relu) v = fmaxf(v, 0.f);
          stg[row * WN + 32 * j + li] = v;
        }
      }
      // (the wave reads back what it wrote itself: LDS operations of a wave complete in order; the compiler must keep
      // the order too)
      asm volatile("" ::: "memory");
      float4 vq[32 / kRowsPerIt];
#pragma unroll
      for (int it = 0; it < 32 / kRowsPerIt; ++it)
        vq[it] = *reinterpret_cast<const float4 *>(&stg[(it * kRowsPerIt + r0) * WN + 4 * c4]);
#pragma unroll
      for (int it = 0; it < 32 / kRowsPerIt; ++it) {
        const int m = m0 + wm * 64 + 32 * i + it * kRowsPerIt + r0;
        if (m < a.Mg && pq < a.P) *reinterpret_cast<float4 *>(oq + (size_t)m * ohw) = vq[it];
      }
      asm volatile("" ::: "memory");
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int pj = p0 + wn * WN + 32 * j + li;
    if (pj >= a.P) continue;
    const int nn = pj / ohw;
    const int rr = pj - nn * ohw;
    float *obase = a.out + ((size_t)nn * a.M + (size_t)cg * a.Mg) * ohw + rr;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int m = m0 + wm * 64 + 32 * i + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
        if (m >= a.Mg) continue;
        float v = acc[i][j][reg] + bv[i][reg];
        if (a.relu) v = fmaxf(v, 0.f);
        obase[(size_t)m * ohw] = v;
      }
    }
  }
}

}  // namespace escoin
