// sconv_backward.hip -- ConvolutionLayer::Backward_gpu (conv_layer.cu:42-73) that keeps the sparsity pattern:
// gradients flow through the plan's CSR nonzeros only, and the weight gradient is written at the CSR's positions only
// (the reference's dense im2col + GEMM backward, base_conv_layer.cpp:859-897, revives pruned weights the sparse
// forward never reads).  Let G = top_diff (x [top > 0] for fuse_relu plans).
//
//   data gradient   bottom_diff[n][c][h][w] = sum over the CSR entries (oc, c, kr, kc) and the output pixels that read
//                   (h, w) of value * G[n][oc][oh][ow]; overwritten.
//     (a) stride-1 float plans with pad <= dil * (K - 1): a FORWARD sparse convolution of G with the transposed,
//         flipped weights (colidx' = ocl*KH*KW + (KH-1-kr)*KW + (KW-1-kc), pad' = dil*(K-1) - pad), run by an internal
//         plan built through set_csr -- so the data gradient gets the generated-code / tiled / MFMA kernels of the
//         forward with no new device code;
//     (b) everything else (stride > 1, larger pads, double, option backward_kernel = GENERIC):
//         escoin_sconv_bwd_data_kernel, one lane per bottom pixel, the wave walking its input channel's transposed-CSR
//         row in ascending (ocl, kr, kc) order with one fma per contributing entry from 0 -- the order of the CPU mode's
//         data gradient (sconv_cpu_backward.cpp), so the two are bit-identical;
//     (c) option backward_kernel = ESCOIN_BWD_MFMA (never AUTO's choice): escoin_sconv_dgrad_mfma_kernel of dgrad_mfma.hip,
//         one stride-1 gather-GEMM per stride phase on the fp32 matrix cores, for float plans of any geometry.
//   weight gradient weight_diff[oc][colidx] += sum over (n, oh, ow) of G * bottom[...], at the CSR positions only;
//   bias gradient   bias_diff[oc] += sum over (n, oh, ow) of G.
//     Two deterministic stages, no float atomics (the order of every sum is a function of the geometry and n_images):
//     escoin_sconv_wgrad_partial_kernel  one workgroup per (chunk of kChunkPixels flattened (n, oh, ow) pixels, output
//                                        channel): every lane holds G for its kPixPerLane pixels in registers, the waves
//                                        walk the row's CSR entries (tap wave-uniform), reduce each entry's per-lane
//                                        partial with a fixed butterfly, then over the four waves in wave order, and
//                                        write one partial per (chunk, entry) -- and per (chunk, oc) for the bias --
//                                        into a slab with plain stores;
//     escoin_sconv_wgrad_sum_kernel      one lane per entry (and per bias): its slab column summed in chunk order, the
//                                        total added into weight_diff / bias_diff.  Every position has one owner.
//     (option "wgrad_kernel": stage 1 by the LDS-staged kernel below, or by the fp32-MFMA kernel of wgrad_mfma.hip -- same
//     chunks, same slab; the MFMA kernel's bias gradient is the entry kernel's, launched for the bias alone.  option
//     "wgrad_pointwise": stage 1 of pointwise layers by the kernel of wgrad_pointwise.hip where AUTO would decide)
//
// Which of these kernels a plan gets, and what it refuses, is decided by the host-only rule bwd_choice (align_rules.h);
// bwd_build here calls it once and does the device work.  The backward state (BwdState, escoin_plan.h: one sub-struct per
// kernel -- GatherDgrad, DgmState, StagedWgrad, WgmState, PwWgrad -- next to the transposed plan, the slab and the ReLU scratch) is
// built by the first backward on an aligned plan -- its index tables by the host-only builders of csr_tables.h, this file
// uploads them -- and dropped with the device side (free_device: weight_align / set_csr / import_aligned; destroy); later
// calls allocate nothing and synchronise nothing, so they can be captured into a graph.  backward_gpu is the driver:
// checks, state, then data_gradient (a switch over BwdState::data, one function per path) and weight_gradient
// (wgrad_entry / wgrad_staged / wgrad_mfma / wgrad_pointwise over the shared stage-1 and stage-2 launch helpers).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "align_rules.h"
#include "escoin_plan.h"

namespace escoin {

constexpr int kBwdWaves = 4;                         // waves per workgroup (both kernels)
constexpr int kPixPerLane = 4;                       // wgrad: pixels each lane holds
constexpr int kChunkPixels = kBwdChunkPixels;
static_assert(kChunkPixels == 64 * kBwdWaves * kPixPerLane, "a chunk is one pixel per lane and step");
constexpr int kEntryBatch = 64;                      // wgrad: entries reduced per barrier pair


template <typename T> __device__ inline T bfma(T a, T b, T c);
template <> __device__ inline float bfma<float>(float a, float b, float c) { return fmaf(a, b, c); }
template <> __device__ inline double bfma<double>(double a, double b, double c) { return fma(a, b, c); }

// ---- data gradient: gather kernel -------------------------------------------------------------------------------
template <typename T>
struct BwdDataArgs {
  const T *__restrict__ top_diff;
  const T *__restrict__ top;       // fuse_relu only
  T *__restrict__ bottom_diff;
  const int *__restrict__ trow;
  const int *__restrict__ ttap;
  const T *__restrict__ tval;
  int C, H, W, M, OH, OW;
  int pad_h, pad_w, stride_h, stride_w, dil_h, dil_w;
  int Cg, Mg;
};

template <typename T, bool RELU>
__device__ inline void bwd_data_body(const BwdDataArgs<T> &a) {
  const int lane = threadIdx.x;
  const int c = __builtin_amdgcn_readfirstlane(blockIdx.y * kBwdWaves + threadIdx.y);
  if (c >= a.C) return;
  const int n = blockIdx.z;
  const int npix = a.H * a.W;
  const int p = blockIdx.x * 64 + lane;
  const bool live = p < npix;
  const int h = live ? p / a.W : 0;
  const int w = live ? p - h * a.W : 0;
  const int grp = c / a.Cg;
  const size_t opix = (size_t)a.OH * a.OW;
  const T *__restrict__ gd = a.top_diff + ((size_t)n * a.M + (size_t)grp * a.Mg) * opix;
  const T *__restrict__ tp = RELU ? a.top + ((size_t)n * a.M + (size_t)grp * a.Mg) * opix : nullptr;
  const int jb = a.trow[c], je = a.trow[c + 1];
  T sum = 0;
  for (int j = jb; j < je; ++j) {
    const unsigned tap = (unsigned)a.ttap[j];
    const T v = a.tval[j];
    const int ocl = (int)(tap >> 16), kr = (tap >> 8) & 0xff, kc = tap & 0xff;
    const int th = h + a.pad_h - kr * a.dil_h;
    const int tw = w + a.pad_w - kc * a.dil_w;
    if (!live || th < 0 || tw < 0) continue;
    const int oh = th / a.stride_h, ow = tw / a.stride_w;
    if (oh * a.stride_h != th || ow * a.stride_w != tw || oh >= a.OH || ow >= a.OW) continue;
    const size_t gi = (size_t)ocl * opix + (size_t)oh * a.OW + ow;
    T g = gd[gi];
    if (RELU && !(tp[gi] > T(0))) g = T(0);
    sum = bfma<T>(v, g, sum);
  }
  if (live) a.bottom_diff[((size_t)n * a.C + c) * npix + p] = sum;
}

template <bool RELU>
__global__ void __launch_bounds__(64 * kBwdWaves)
escoin_sconv_bwd_data_kernel(BwdDataArgs<float> a) { bwd_data_body<float, RELU>(a); }

template <bool RELU>
__global__ void __launch_bounds__(64 * kBwdWaves)
escoin_sconv_bwd_data_f64_kernel(BwdDataArgs<double> a) { bwd_data_body<double, RELU>(a); }

// fuse_relu + transposed plan: G = top_diff * [top > 0] into scratch, the transposed plan's bottom
__global__ void __launch_bounds__(256)
escoin_sconv_bwd_relu_mask_kernel(const float *__restrict__ top_diff, const float *__restrict__ top,
                                  float *__restrict__ g, size_t count) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256)
    g[i] = top[i] > 0.f ? top_diff[i] : 0.f;
}

// ---- weight / bias gradient -------------------------------------------------------------------------------------
template <typename T>
struct WgradArgs {
  const T *__restrict__ bottom;
  const T *__restrict__ top_diff;
  const T *__restrict__ top;       // fuse_relu only
  const int *__restrict__ rowptr;  // [M + 1] absolute
  const int *__restrict__ taps;    // packed (ic, kr, kc), ic group-local
  T *__restrict__ slab_w;          // [chunks][nnz]
  T *__restrict__ slab_b;          // [chunks][M]
  long total;                      // n_images * OH * OW
  int nnz;
  int C, H, W, M, OH, OW;
  int pad_h, pad_w, stride_h, stride_w, dil_h, dil_w;
  int Cg, Mg;
  int want_w, want_b;
};

// Sum over the wave's 64 lanes with a fixed butterfly: the same tree on every call.
template <typename T>
__device__ inline T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <typename T, bool RELU>
__device__ inline void wgrad_partial_body(const WgradArgs<T> &a) {
  __shared__ T red[kBwdWaves][kEntryBatch];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int chunk = blockIdx.x;
  const int oc = blockIdx.y;
  const int grp = oc / a.Mg;
  const int opix = a.OH * a.OW;
  const size_t plane = (size_t)a.H * a.W;
  T g[kPixPerLane];
  size_t img[kPixPerLane];
  int ih0[kPixPerLane], iw0[kPixPerLane];
#pragma unroll
  for (int i = 0; i < kPixPerLane; ++i) {
    const long q = (long)chunk * kChunkPixels + i * 64 * kBwdWaves + tid;
    const bool live = q < a.total;
    const long n = live ? q / opix : 0;
    const int r = live ? (int)(q - n * opix) : 0;
    const int oh = r / a.OW, ow = r - oh * a.OW;
    const size_t gi = ((size_t)n * a.M + oc) * opix + r;
    T gv = live ? a.top_diff[gi] : T(0);
    if (RELU && live && !(a.top[gi] > T(0))) gv = T(0);
    g[i] = gv;
    img[i] = ((size_t)n * a.C + (size_t)grp * a.Cg) * plane;
    // a dead lane gets an origin no tap can bring inside the image: it reads nothing
    ih0[i] = live ? oh * a.stride_h - a.pad_h : -(1 << 29);
    iw0[i] = ow * a.stride_w - a.pad_w;
  }
  if (a.want_b) {
    T s = g[0];
#pragma unroll
    for (int i = 1; i < kPixPerLane; ++i) s += g[i];
    s = wave_sum(s);
    if (lane == 0) red[wave][0] = s;
    __syncthreads();
    if (tid == 0) {
      T t = red[0][0];
      for (int k = 1; k < kBwdWaves; ++k) t += red[k][0];
      a.slab_b[(size_t)chunk * a.M + oc] = t;
    }
    __syncthreads();
  }
  if (!a.want_w) return;
  const int jb = a.rowptr[oc], je = a.rowptr[oc + 1];
  for (int j0 = jb; j0 < je; j0 += kEntryBatch) {
    const int jn = min(kEntryBatch, je - j0);
    for (int k = 0; k < jn; ++k) {
      const int tap = a.taps[j0 + k];
      const int ic = tap >> 16, kr = (tap >> 8) & 0xff, kc = tap & 0xff;
      T acc = 0;
#pragma unroll
      for (int i = 0; i < kPixPerLane; ++i) {
        const int ih = ih0[i] + kr * a.dil_h;
        const int iw = iw0[i] + kc * a.dil_w;
        T x = 0;
        if ((unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W)
          x = a.bottom[img[i] + (size_t)ic * plane + (size_t)ih * a.W + iw];
        acc = bfma<T>(g[i], x, acc);
      }
      acc = wave_sum(acc);
      if (lane == 0) red[wave][k] = acc;
    }
    __syncthreads();
    if (tid < jn) {
      T t = red[0][tid];
      for (int k = 1; k < kBwdWaves; ++k) t += red[k][tid];
      a.slab_w[(size_t)chunk * a.nnz + j0 + tid] = t;
    }
    __syncthreads();
  }
}

template <bool RELU>
__global__ void __launch_bounds__(64 * kBwdWaves)
escoin_sconv_wgrad_partial_kernel(WgradArgs<float> a) { wgrad_partial_body<float, RELU>(a); }

template <bool RELU>
__global__ void __launch_bounds__(64 * kBwdWaves)
escoin_sconv_wgrad_partial_f64_kernel(WgradArgs<double> a) { wgrad_partial_body<double, RELU>(a); }

// One lane per weight entry, then one per bias: the slab column in chunk order, then += into the gradient.
template <typename T>
__device__ inline void wgrad_sum_body(const T *__restrict__ slab_w, const T *__restrict__ slab_b,
                                      const int *__restrict__ wpos, T *__restrict__ weight_diff,
                                      T *__restrict__ bias_diff, int nnz, int M, int chunks) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (weight_diff && e < nnz) {
    T s = 0;
    for (int c = 0; c < chunks; ++c) s += slab_w[(size_t)c * nnz + e];
    const long pos = wpos ? wpos[e] : e;   // compact output (escoin_backward_values): entry e itself
    weight_diff[pos] = weight_diff[pos] + s;
    return;
  }
  const long b = e - (weight_diff ? nnz : 0);
  if (bias_diff && b >= 0 && b < M) {
    T s = 0;
    for (int c = 0; c < chunks; ++c) s += slab_b[(size_t)c * M + b];
    bias_diff[b] = bias_diff[b] + s;
  }
}

__global__ void __launch_bounds__(256)
escoin_sconv_wgrad_sum_kernel(const float *slab_w, const float *slab_b, const int *wpos, float *weight_diff,
                              float *bias_diff, int nnz, int M, int chunks) {
  wgrad_sum_body<float>(slab_w, slab_b, wpos, weight_diff, bias_diff, nnz, M, chunks);
}

__global__ void __launch_bounds__(256)
escoin_sconv_wgrad_sum_f64_kernel(const double *slab_w, const double *slab_b, const int *wpos, double *weight_diff,
                                  double *bias_diff, int nnz, int M, int chunks) {
  wgrad_sum_body<double>(slab_w, slab_b, wpos, weight_diff, bias_diff, nnz, M, chunks);
}

// ---- weight / bias gradient, LDS-staged (option "wgrad_kernel" = STAGED; float plans, stride 1) ---------------------
// Stage 1 of the same two-stage reduction (same chunks, same slab), with the bottom read from global memory once per
// workgroup instead of once per nonzero.  Stride 1 makes the padded input image the natural frame: with Hp = H + 2 pad_h
// = OH + dil_h (KH - 1) and Wp likewise, output pixel (n, oh, ow) and tap (kr, kc) read padded pixel
// (n * Hp + oh + kr * dil_h, ow + kc * dil_w) -- a per-lane base plus a wave-uniform tap offset.  One workgroup per
// (chunk, slice of a conv group's output channels, block of input channels):
//   staging   the padded rows the chunk's pixels touch (images stacked Hp rows apart, the halo and images past n_images
//             as zeros), for the block's channels, into LDS -- once;
//   walk      each wave takes whole output channels: G for all 1024 pixels of the chunk in registers (16 per lane), then
//             the channel's CSR entries of this block (the host table blk: rows are sorted by input channel); per
//             entry 16 LDS reads and 16 FMAs into the lane's own partial, no cross-lane step;
//   reduce    eight entries at a time: three halving exchanges (a lane keeps half the entries and receives its partner's
//             partials for them), then a butterfly over the last three lane bits -- per entry the pairing (lane ^ 32,
//             ^ 16, ... ^ 1) of wave_sum, so an entry's bits depend neither on its place in a batch nor on the blocking;
//   bias      summed from the same registers by the workgroups of block 0; a bias-only call launches those alone, stages
//             nothing and walks nothing.
// An entry belongs to one (output channel, input-channel block): every slab element has one writer.  Dead pixels of the
// last chunk are masked by select (their G is 0, but 0 x a staged non-finite value is not): a non-finite bottom element
// reaches only the entries whose tap reads it.
// (kStgWaves waves per workgroup, kStgBatch entries per batched reduction, kStgLdsBudget, kStgSmallInt: align_rules.h,
// with the rule that plans the blocks)
constexpr int kStgPix = kChunkPixels / 64;           // pixels per lane: a wave covers the whole chunk

struct StagedArgs {
  const float *__restrict__ bottom;
  const float *__restrict__ top_diff;
  const float *__restrict__ top;      // fuse_relu only
  const int *__restrict__ blk;        // [M][nblk + 1]
  const int *__restrict__ off;        // [nnz]
  float *__restrict__ slab_w;         // [chunks][nnz]
  float *__restrict__ slab_b;         // [chunks][M]
  long total;                         // n_images * OH * OW
  int nnz, n_images;
  int C, H, W, M, OH, OW;
  int pad_h, pad_w, span_h;           // span_h = dil_h * (KH - 1)
  int Cg, Mg, Hp, Wp;
  int icb, nblk, rows_max, cs;        // cs = rows_max * Wp: floats per staged channel
  int osplit, mper;                   // slices per conv group, output channels per slice
  int want_w, want_b;
  float inv_opix, inv_ow, inv_wp, inv_hp;
};

// x / d for 0 <= x < kStgSmallInt through the float reciprocal, corrected: exact.
__device__ inline int div_small(int x, int d, float inv, int &rem) {
  int k = (int)((float)x * inv);
  rem = x - k * d;
  if (rem < 0) { --k; rem += d; }
  else if (rem >= d) { ++k; rem -= d; }
  return k;
}

// Sums v[k] over the wave for k < 8; lane l returns the total of entry l >> 3.
__device__ inline float stg_reduce8(const float (&v)[kStgBatch], int lane) {
  float t[4], u[2];
  bool hi = (lane & 32) != 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) t[j] = (hi ? v[j + 4] : v[j]) + __shfl_xor(hi ? v[j] : v[j + 4], 32, 64);
  hi = (lane & 16) != 0;
#pragma unroll
  for (int j = 0; j < 2; ++j) u[j] = (hi ? t[j + 2] : t[j]) + __shfl_xor(hi ? t[j] : t[j + 2], 16, 64);
  hi = (lane & 8) != 0;
  float w = (hi ? u[1] : u[0]) + __shfl_xor(hi ? u[0] : u[1], 8, 64);
  w += __shfl_xor(w, 4, 64);
  w += __shfl_xor(w, 2, 64);
  w += __shfl_xor(w, 1, 64);
  return w;
}

template <bool RELU, bool PARTIAL>
__device__ inline void stg_walk(const StagedArgs &a, const float *tile, int chunk, int grp, int part, int b, int wave,
                                int lane, int n0, int r0, int P0) {
  const int opix = a.OH * a.OW;
  int base[kStgPix];
  unsigned gb[kStgPix];
  unsigned livemask = 0;
#pragma unroll
  for (int i = 0; i < kStgPix; ++i) {
    const int ql = i * 64 + lane;
    const bool live = (long)chunk * kChunkPixels + ql < a.total;
    int r, ow;
    const int dn = div_small(r0 + ql, opix, a.inv_opix, r);
    const int oh = div_small(r, a.OW, a.inv_ow, ow);
    const int n = n0 + dn;
    base[i] = live ? ((n * a.Hp + oh - P0) * a.Wp + ow) : 0;
    gb[i] = live ? (unsigned)n * (unsigned)a.M * (unsigned)opix + (unsigned)r : 0u;
    livemask |= live ? (1u << i) : 0u;
  }
  const int m_end = min(a.Mg, (part + 1) * a.mper);
  const bool bias_here = a.want_b && b == 0;
  for (int m = part * a.mper + wave; m < m_end; m += kStgWaves) {
    const int oc = grp * a.Mg + m;
    const int jb = a.blk[(size_t)oc * (a.nblk + 1) + b];
    const int je = a.want_w ? a.blk[(size_t)oc * (a.nblk + 1) + b + 1] : jb;
    if (jb == je && !bias_here) continue;
    float g[kStgPix];
    const unsigned oco = (unsigned)oc * (unsigned)opix;
#pragma unroll
    for (int i = 0; i < kStgPix; ++i) {
      float gv = 0.f;
      if (!PARTIAL || ((livemask >> i) & 1u)) {
        gv = a.top_diff[gb[i] + oco];
        if (RELU && !(a.top[gb[i] + oco] > 0.f)) gv = 0.f;
      }
      g[i] = gv;
    }
    if (bias_here) {
      float sb = g[0];
#pragma unroll
      for (int i = 1; i < kStgPix; ++i) sb += g[i];
      sb = wave_sum(sb);
      if (lane == 0) a.slab_b[(size_t)chunk * a.M + oc] = sb;
    }
    // the tap offsets of a batch are fetched one batch ahead (off is padded by two batches): a scalar load shares
    // its counter with the LDS reads, so waiting for one inside the walk would drain the other
    int o[kStgBatch], o_next[kStgBatch] = {};
    if (jb != je) {   // (a bias-only walk fetches nothing)
#pragma unroll
      for (int k = 0; k < kStgBatch; ++k) o_next[k] = a.off[jb + k];
    }
    for (int j0 = jb; j0 < je; j0 += kStgBatch) {
      const int jn = min(kStgBatch, je - j0);
#pragma unroll
      for (int k = 0; k < kStgBatch; ++k) {
        o[k] = o_next[k];
        o_next[k] = a.off[j0 + kStgBatch + k];
      }
      float acc[kStgBatch];
#pragma unroll
      for (int k = 0; k < kStgBatch; ++k) {
        acc[k] = 0.f;
        if (k < jn) {
#pragma unroll
          for (int i = 0; i < kStgPix; ++i) {
            float x = tile[base[i] + o[k]];
            if (PARTIAL) x = ((livemask >> i) & 1u) ? x : 0.f;
            acc[k] = fmaf(g[i], x, acc[k]);
          }
        }
      }
      const float t = stg_reduce8(acc, lane);
      if ((lane & 7) == 0 && (lane >> 3) < jn) a.slab_w[(size_t)chunk * a.nnz + j0 + (lane >> 3)] = t;
    }
  }
}

template <bool RELU>
__global__ void __launch_bounds__(64 * kStgWaves)
escoin_sconv_wgrad_staged_kernel(StagedArgs a) {
  extern __shared__ float stg_tile[];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int chunk = blockIdx.x;
  const int grp = blockIdx.y / a.osplit, part = blockIdx.y - grp * a.osplit;
  const int b = blockIdx.z;
  const int opix = a.OH * a.OW;
  const long q0 = (long)chunk * kChunkPixels;
  const long q1 = min(a.total, q0 + kChunkPixels) - 1;
  const int n0 = (int)(q0 / opix), r0 = (int)(q0 - (long)n0 * opix);
  const int n1 = (int)(q1 / opix), r1 = (int)(q1 - (long)n1 * opix);
  const int P0 = n0 * a.Hp + r0 / a.OW;
  const int rows = min(n1 * a.Hp + r1 / a.OW + a.span_h - P0 + 1, a.rows_max);
  if (a.want_w) {
    const int ic0 = b * a.icb;
    const int nch = min(a.icb, a.Cg - ic0);
    const int count = nch * rows * a.Wp;
    const size_t plane = (size_t)a.H * a.W;
    const float inv_rows = 1.0f / (float)rows;
    const int ihp0 = P0 - n0 * a.Hp;
    const float *__restrict__ src = a.bottom + ((size_t)grp * a.Cg + ic0) * plane;
    for (int idx = tid; idx < count; idx += 64 * kStgWaves) {
      int col, r, ihp;
      const int pr = div_small(idx, a.Wp, a.inv_wp, col);
      const int ch = div_small(pr, rows, inv_rows, r);
      const int n = n0 + div_small(ihp0 + r, a.Hp, a.inv_hp, ihp);
      const int ih = ihp - a.pad_h, iw = col - a.pad_w;
      float v = 0.f;
      if (n < a.n_images && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W)
        v = src[((size_t)n * a.C + ch) * plane + (size_t)ih * a.W + iw];
      stg_tile[ch * a.cs + r * a.Wp + col] = v;
    }
    __syncthreads();
  }
  if (q0 + kChunkPixels > a.total) stg_walk<RELU, true>(a, stg_tile, chunk, grp, part, b, wave, lane, n0, r0, P0);
  else stg_walk<RELU, false>(a, stg_tile, chunk, grp, part, b, wave, lane, n0, r0, P0);
}

// Stage 2 of the staged path: 16 items (weight entries, then biases) per workgroup, the chunk axis dealt over 16 lanes
// per item (lane c sums chunks c, c + 16, ... in that order), then the 16 partials in lane order, then += into the
// gradient.  wpos == nullptr: compact output, entry e goes to weight_diff[e].
__global__ void __launch_bounds__(256)
escoin_sconv_wgrad_tree_sum_kernel(const float *__restrict__ slab_w, const float *__restrict__ slab_b,
                                   const int *__restrict__ wpos, float *weight_diff, float *bias_diff, int nnz, int M,
                                   int chunks) {
  __shared__ float red[16][17];
  const int el = threadIdx.x & 15, cl = threadIdx.x >> 4;
  const long n_w = weight_diff ? nnz : 0;
  const long items = n_w + (bias_diff ? M : 0);
  const long item = (long)blockIdx.x * 16 + el;
  float s = 0.f;
  if (item < items) {
    const float *col = item < n_w ? slab_w + item : slab_b + (item - n_w);
    const size_t stride = item < n_w ? (size_t)nnz : (size_t)M;
    for (int c = cl; c < chunks; c += 16) s += col[(size_t)c * stride];
  }
  red[cl][el] = s;
  __syncthreads();
  if (cl == 0 && item < items) {
    float t = red[0][el];
#pragma unroll
    for (int k = 1; k < 16; ++k) t += red[k][el];
    if (item < n_w) {
      const long pos = wpos ? wpos[item] : item;
      weight_diff[pos] = weight_diff[pos] + t;
    } else {
      bias_diff[item - n_w] = bias_diff[item - n_w] + t;
    }
  }
}

// ---- backward state: the device work for what align_rules.h bwd_choice decided ------------------------------------
// The transposed forward plan of path (a): geometry of the data gradient as a stride-1 forward of G; for fuse_relu plans
// also the scratch that holds G.
static int build_transposed_plan(escoin_plan *p, BwdState *s, hipStream_t stream) {
  const Geometry &g = p->g;
  const escoin_conv_desc &d = g.d;
  escoin_conv_desc t = d;
  t.C = d.M; t.H = g.OH; t.W = g.OW; t.M = d.C;
  t.pad_h = d.dil_h * (d.KH - 1) - d.pad_h;
  t.pad_w = d.dil_w * (d.KW - 1) - d.pad_w;
  t.stride_h = t.stride_w = 1;
  t.has_bias = 0;
  t.fuse_relu = 0;
  // the forced data-gradient kernel is this plan's forward kernel; it has no backward of its own
  const int rc = build_derived_plan(p, t, p->bwd_kernel, ESCOIN_KERNEL_AUTO, forward_transpose(csr_view(p)), stream, &s->transposed);
  if (rc != ESCOIN_OK || !d.fuse_relu) return rc;
  ESCOIN_HIP_TRY(s->g.alloc(sizeof(float) * (size_t)d.N * d.M * g.OH * g.OW));
  return ESCOIN_OK;
}

// The gather kernel's transposed CSR (csr_tables.h gather_transpose), with the values in its order.
template <typename T>
static int build_gather(escoin_plan *p, GatherDgrad *ga, hipStream_t stream) {
  GatherTables t = gather_transpose(csr_view(p));
  const std::vector<T> flat = flat_entries(plan_vals<T>(p));
  std::vector<T> tval(t.ttap.size(), T(0));
  for (size_t k = 0; k < t.tsrc.size(); ++k) tval[k] = flat[(size_t)t.tsrc[k]];
  ESCOIN_HIP_TRY(ga->trow.upload(t.trow, stream));
  ESCOIN_HIP_TRY(ga->ttap.upload(t.ttap, stream));
  ESCOIN_HIP_TRY(ga->tval.upload(tval, stream));
  ESCOIN_HIP_TRY(hipStreamSynchronize(stream));   // host vectors die at scope exit
  ga->tsrc = std::move(t.tsrc);
  return ESCOIN_OK;
}

static int stg_build(const escoin_plan *p, const StgPlan &sp, StagedWgrad *st, hipStream_t stream) {
  st->icb = sp.icb;
  st->nblk = sp.nblk;
  st->rows = sp.rows_max;
  st->lds_bytes = sp.lds_bytes;
  st->osplit = sp.osplit;
  const StagedTables t = staged_tables(csr_view(p), sp.icb, sp.nblk, sp.cs, p->g.d.W + 2 * p->g.d.pad_w);
  ESCOIN_HIP_TRY(st->blk.upload(t.blk, stream));
  ESCOIN_HIP_TRY(st->off.upload(t.off, stream));
  ESCOIN_HIP_TRY(hipStreamSynchronize(stream));   // host vectors die at scope exit
  return ESCOIN_OK;
}

template <typename T> static int bwd_build(escoin_plan *p, hipStream_t stream);

// The plan's backward state, built where this alignment has none yet; a refused or failed build leaves none behind.
template <typename T>
static int ensure_state(escoin_plan *p, hipStream_t stream) {
  if (p->bwd) return ESCOIN_OK;
  const int rc = bwd_build<T>(p, stream);
  if (rc != ESCOIN_OK) p->bwd.reset();
  return rc;
}

// The data gradient's side of the state.
template <typename T>
static int build_data(escoin_plan *p, BwdState *s, const BwdChoice &c, hipStream_t stream) {
  switch (c.data) {
    // the inner plan's backward state is built here, with this one: the update list is rebuilt once for both, and no
    // later call allocates (dX' is the X' scratch)
    case kBwdInner: return ensure_state<float>(p->inner_plan()->plan.get(), stream);
    case kBwdTransposed: return build_transposed_plan(p, s, stream);
    case kBwdMfma: return dgm_build(p, c.dgm, &s->dgm, stream);
    case kBwdGather: break;
  }
  return build_gather<T>(p, &s->gather, stream);
}

// The rule decides (align_rules.h bwd_choice), this does the device work: uploads, allocations, the derived plans.
template <typename T>
static int bwd_build(escoin_plan *p, hipStream_t stream) {
  const auto t0 = std::chrono::steady_clock::now();
  // (after device-source weight updates the host CSR this state is built from is stale: the values come back first)
  if (const int rcs = sync_host_values(p)) return rcs;
  const Geometry &g = p->g;
  const long nnz = plan_nnz(p);
  const BwdOptions o{p->bwd_kernel, p->wgrad_kernel, p->wgrad_channel_block, p->inner_plan() != nullptr, p->wgrad_pointwise,
                     p->wgrad_pw_tile_entries};
  const BwdChoice c = bwd_choice(g, p->is_f64, nnz, o, tiled_device_cus());
  if (c.rc != ESCOIN_OK) return fail(c.rc, c.error);
  p->bwd.reset(new BwdState());
  BwdState *s = p->bwd.get();
  s->nnz = nnz; s->data = c.data; s->wgrad = c.wgrad; s->chunks_max = c.chunks_max;
  int rc = build_data<T>(p, s, c, stream);
  if (rc != ESCOIN_OK) return rc;
  const std::vector<int> wpos = dense_positions(csr_view(p), g.kdim);   // (lives until the synchronise below)
  ESCOIN_HIP_TRY(s->wpos.upload(wpos, stream));
  ESCOIN_HIP_TRY(s->slab.alloc(sizeof(T) * (size_t)s->chunks_max * (size_t)(nnz + g.d.M)));
  if (c.wgrad == ESCOIN_WGRAD_MFMA) rc = wgm_build(p, c.wgm, &s->wgm, stream);
  else if (c.wgrad == ESCOIN_WGRAD_STAGED) rc = stg_build(p, c.stg, &s->stg, stream);
  else if (c.wgrad == ESCOIN_WGRAD_POINTWISE) rc = pw_build(p, o, &s->pw, stream);
  if (rc != ESCOIN_OK) return rc;
  ESCOIN_HIP_TRY(hipStreamSynchronize(stream));
  s->align_ms = ms_since(t0);
  return ESCOIN_OK;
}

// ---- data gradient: one function per path ----------------------------------------------------------------------------
// option "s2d": dX' = the inner plan's data gradient of top_diff (the ReLU mask is its own), then depth-to-space
// option "s2b": G' = top_diff's residue classes (times [top > 0] on a fuse_relu plan), dX' = the inner plan's data
// gradient of G' (it has no ReLU and needs no top), then the classes interleaved into bottom_diff
static int dgrad_inner(escoin_plan *p, const float *top, const float *top_diff, float *bottom_diff, int n_images,
                       hipStream_t stream) {
  if (S2bState *sb = p->s2b_state.get()) {
    const int P = sb->sp.eh * sb->sp.ew;
    int rc = g_s2b_hooks.pack(p, top_diff, p->g.d.fuse_relu ? top : nullptr, sb->t.get<float>(), true, n_images, stream);
    if (rc != ESCOIN_OK) return rc;
    rc = escoin_backward(sb->inner.plan.get(), nullptr, nullptr, sb->t.get<const float>(), sb->x.get<float>(), nullptr, nullptr, n_images * P, stream);
    return rc != ESCOIN_OK ? rc : g_s2b_hooks.unpack(p, sb->x.get<const float>(), bottom_diff, false, false, n_images, stream);
  }
  S2dState *sd = p->s2d_state.get();
  const int rc = escoin_backward(sd->inner.plan.get(), nullptr, top, top_diff, sd->x.get<float>(), nullptr, nullptr, n_images, stream);
  return rc != ESCOIN_OK ? rc : g_s2d_hooks.unpack(p, sd->x.get<const float>(), bottom_diff, n_images, stream);
}

static int dgrad_transposed(escoin_plan *p, const float *top, const float *top_diff, float *bottom_diff, int n_images,
                            hipStream_t stream) {
  const Geometry &g = p->g;
  const BwdState *s = p->bwd.get();
  const float *src = top_diff;
  if (g.d.fuse_relu) {
    const size_t count = (size_t)n_images * g.d.M * g.OH * g.OW;
    const unsigned blocks = (unsigned)std::min<size_t>((count + 255) / 256, 8192);
    hipLaunchKernelGGL(escoin_sconv_bwd_relu_mask_kernel, dim3(blocks), dim3(256), 0, stream, top_diff, top, s->g.get<float>(), count);
    ESCOIN_HIP_TRY(hipGetLastError());
    src = s->g.get<const float>();
  }
  return escoin_forward(s->transposed.plan.get(), src, nullptr, bottom_diff, n_images, stream);
}

// One launch of a kernel that is compiled with and without the fuse_relu mask.
template <typename A>
static int launch_relu_pair(bool relu, void (*masked)(A), void (*plain)(A), dim3 grid, dim3 block, size_t lds, hipStream_t stream,
                            const A &a) {
  hipLaunchKernelGGL(relu ? masked : plain, grid, block, lds, stream, a);
  ESCOIN_HIP_TRY(hipGetLastError());
  return ESCOIN_OK;
}

template <typename T>
static int dgrad_gather(const escoin_plan *p, const T *top, const T *top_diff, T *bottom_diff, int n_images, hipStream_t stream) {
  const Geometry &g = p->g;
  const escoin_conv_desc &d = g.d;
  const GatherDgrad &ga = p->bwd->gather;
  BwdDataArgs<T> a;
  a.top_diff = top_diff; a.top = top; a.bottom_diff = bottom_diff;
  a.trow = ga.trow.get<int>(); a.ttap = ga.ttap.get<int>(); a.tval = ga.tval.get<T>();
  a.C = d.C; a.H = d.H; a.W = d.W; a.M = d.M; a.OH = g.OH; a.OW = g.OW;
  a.pad_h = d.pad_h; a.pad_w = d.pad_w; a.stride_h = d.stride_h; a.stride_w = d.stride_w;
  a.dil_h = d.dil_h; a.dil_w = d.dil_w; a.Cg = g.Cg; a.Mg = g.Mg;
  const dim3 grid((d.H * d.W + 63) / 64, (d.C + kBwdWaves - 1) / kBwdWaves, n_images), block(64, kBwdWaves);
  if constexpr (sizeof(T) == 8)
    return launch_relu_pair(d.fuse_relu, escoin_sconv_bwd_data_f64_kernel<true>, escoin_sconv_bwd_data_f64_kernel<false>, grid, block, 0, stream, a);
  else
    return launch_relu_pair(d.fuse_relu, escoin_sconv_bwd_data_kernel<true>, escoin_sconv_bwd_data_kernel<false>, grid, block, 0, stream, a);
}

template <typename T>
static int data_gradient(escoin_plan *p, const T *top, const T *top_diff, T *bottom_diff, int n_images, hipStream_t stream) {
  if constexpr (sizeof(T) == 4) {   // (a double plan's data gradient is the gather kernel's: bwd_choice)
    switch (p->bwd->data) {
      case kBwdInner: return dgrad_inner(p, top, top_diff, bottom_diff, n_images, stream);
      case kBwdTransposed: return dgrad_transposed(p, top, top_diff, bottom_diff, n_images, stream);
      case kBwdMfma: return launch_dgrad_mfma(p, p->bwd->dgm, top, top_diff, bottom_diff, n_images, stream);
      case kBwdGather: break;
    }
  }
  return dgrad_gather<T>(p, top, top_diff, bottom_diff, n_images, stream);
}

// ---- weight / bias gradient: stage 1 by one of four kernels, stage 2 by one of two sums -----------------------------
// One call's blobs, outputs (either may be null), slab and chunks.
template <typename T>
struct WgradCall {
  const T *bottom, *top, *top_diff;
  T *weight_diff, *bias_diff;
  T *slab_w, *slab_b;
  const int *wpos;       // null: compact output (escoin_backward_values), stage 2 writes entry e to weight_diff[e]
  int n_images, chunks;
  hipStream_t stream;
};

// Stage 1 by the entry kernel, for the weights and / or the bias.
template <typename T>
static int launch_partial(const escoin_plan *p, const WgradCall<T> &c, bool want_w, bool want_b) {
  const Geometry &g = p->g;
  const escoin_conv_desc &d = g.d;
  if (d.M > 65535) return fail(ESCOIN_EINVAL, "backward: more than 65535 output channels");
  WgradArgs<T> a;
  a.bottom = c.bottom; a.top_diff = c.top_diff; a.top = c.top;
  a.rowptr = p->gen.rowptr.get<int>(); a.taps = p->gen.taps.get<int>();
  a.slab_w = c.slab_w; a.slab_b = c.slab_b;
  a.total = (long)c.n_images * g.OH * g.OW; a.nnz = (int)p->bwd->nnz;
  a.C = d.C; a.H = d.H; a.W = d.W; a.M = d.M; a.OH = g.OH; a.OW = g.OW;
  a.pad_h = d.pad_h; a.pad_w = d.pad_w; a.stride_h = d.stride_h; a.stride_w = d.stride_w;
  a.dil_h = d.dil_h; a.dil_w = d.dil_w; a.Cg = g.Cg; a.Mg = g.Mg;
  a.want_w = want_w; a.want_b = want_b;
  const dim3 grid(c.chunks, d.M), block(64 * kBwdWaves);
  if constexpr (sizeof(T) == 8)
    return launch_relu_pair(d.fuse_relu, escoin_sconv_wgrad_partial_f64_kernel<true>, escoin_sconv_wgrad_partial_f64_kernel<false>, grid, block, 0, c.stream, a);
  else
    return launch_relu_pair(d.fuse_relu, escoin_sconv_wgrad_partial_kernel<true>, escoin_sconv_wgrad_partial_kernel<false>, grid, block, 0, c.stream, a);
}

// Stage 2, one lane per item: the slab's columns into weight_diff and / or bias_diff (a null one is left out).
template <typename T>
static int launch_sum(const escoin_plan *p, const WgradCall<T> &c, T *weight_diff, T *bias_diff) {
  const int nnz = (int)p->bwd->nnz, M = p->g.d.M;
  const long lanes = (weight_diff ? nnz : 0) + (bias_diff ? M : 0);
  if (lanes == 0) return ESCOIN_OK;
  const dim3 grid((unsigned)((lanes + 255) / 256));
  if constexpr (sizeof(T) == 8)
    hipLaunchKernelGGL(escoin_sconv_wgrad_sum_f64_kernel, grid, dim3(256), 0, c.stream, c.slab_w, c.slab_b, c.wpos, weight_diff,
                       bias_diff, nnz, M, c.chunks);
  else
    hipLaunchKernelGGL(escoin_sconv_wgrad_sum_kernel, grid, dim3(256), 0, c.stream, c.slab_w, c.slab_b, c.wpos, weight_diff,
                       bias_diff, nnz, M, c.chunks);
  ESCOIN_HIP_TRY(hipGetLastError());
  return ESCOIN_OK;
}

// Stage 2 of the staged and the MFMA kernel, 16 lanes per item.
static int launch_tree_sum(const escoin_plan *p, const WgradCall<float> &c, float *weight_diff, float *bias_diff) {
  const int nnz = (int)p->bwd->nnz, M = p->g.d.M;
  const long items = (weight_diff ? nnz : 0) + (bias_diff ? M : 0);
  if (items == 0) return ESCOIN_OK;
  hipLaunchKernelGGL(escoin_sconv_wgrad_tree_sum_kernel, dim3((unsigned)((items + 15) / 16)), dim3(256), 0, c.stream, c.slab_w,
                     c.slab_b, c.wpos, weight_diff, bias_diff, nnz, M, c.chunks);
  ESCOIN_HIP_TRY(hipGetLastError());
  return ESCOIN_OK;
}

template <typename T>
static int wgrad_entry(const escoin_plan *p, const WgradCall<T> &c) {
  const int rc = launch_partial<T>(p, c, c.weight_diff != nullptr, c.bias_diff != nullptr);
  return rc != ESCOIN_OK ? rc : launch_sum<T>(p, c, c.weight_diff, c.bias_diff);
}

static int wgrad_staged(const escoin_plan *p, const WgradCall<float> &c) {
  const Geometry &g = p->g;
  const escoin_conv_desc &d = g.d;
  const BwdState *s = p->bwd.get();
  const StagedWgrad &st = s->stg;
  StagedArgs sa;
  sa.bottom = c.bottom; sa.top_diff = c.top_diff; sa.top = c.top;
  sa.blk = st.blk.get<int>(); sa.off = st.off.get<int>();
  sa.slab_w = c.slab_w; sa.slab_b = c.slab_b;
  sa.total = (long)c.n_images * g.OH * g.OW; sa.nnz = (int)s->nnz; sa.n_images = c.n_images;
  sa.C = d.C; sa.H = d.H; sa.W = d.W; sa.M = d.M; sa.OH = g.OH; sa.OW = g.OW;
  sa.pad_h = d.pad_h; sa.pad_w = d.pad_w; sa.span_h = d.dil_h * (d.KH - 1);
  sa.Cg = g.Cg; sa.Mg = g.Mg; sa.Hp = d.H + 2 * d.pad_h; sa.Wp = d.W + 2 * d.pad_w;
  sa.icb = st.icb; sa.nblk = st.nblk; sa.rows_max = st.rows; sa.cs = st.rows * sa.Wp;
  sa.osplit = st.osplit; sa.mper = (g.Mg + st.osplit - 1) / st.osplit;
  sa.want_w = c.weight_diff != nullptr; sa.want_b = c.bias_diff != nullptr;
  sa.inv_opix = 1.0f / (float)(g.OH * g.OW); sa.inv_ow = 1.0f / (float)g.OW;
  sa.inv_wp = 1.0f / (float)sa.Wp; sa.inv_hp = 1.0f / (float)sa.Hp;
  const dim3 grid(c.chunks, d.group * st.osplit, sa.want_w ? st.nblk : 1), block(64 * kStgWaves);
  const size_t lds = sa.want_w ? st.lds_bytes : 0;
  const int rc = launch_relu_pair(d.fuse_relu, escoin_sconv_wgrad_staged_kernel<true>, escoin_sconv_wgrad_staged_kernel<false>, grid, block, lds, c.stream, sa);
  return rc != ESCOIN_OK ? rc : launch_tree_sum(p, c, c.weight_diff, c.bias_diff);
}

// weights: the MFMA kernel's partials, then the tree sum; bias: the entry kernel's bias-only stage 1 and its serial
// stage 2 -- the entry kernel's bias bits
static int wgrad_mfma(const escoin_plan *p, const WgradCall<float> &c) {
  const BwdState *s = p->bwd.get();
  int rc = ESCOIN_OK;
  if (c.weight_diff) {
    rc = launch_wgrad_mfma(p, s->wgm, s->nnz, c.bottom, c.top, c.top_diff, c.slab_w, c.n_images, c.chunks, c.stream);
    if (rc == ESCOIN_OK) rc = launch_tree_sum(p, c, c.weight_diff, nullptr);
  }
  if (rc == ESCOIN_OK && c.bias_diff) {
    rc = launch_partial<float>(p, c, false, true);
    if (rc == ESCOIN_OK) rc = launch_sum<float>(p, c, nullptr, c.bias_diff);
  }
  return rc;
}

// option "wgrad_pointwise": weights and bias by the pointwise kernel (wgrad_pointwise.hip), then the tree sum
static int wgrad_pointwise(const escoin_plan *p, const WgradCall<float> &c) {
  const BwdState *s = p->bwd.get();
  const int rc = launch_wgrad_pointwise(p, s->pw, s->nnz, c.bottom, c.top, c.top_diff, c.weight_diff ? c.slab_w : nullptr,
                                        c.bias_diff ? c.slab_b : nullptr, c.n_images, c.chunks, c.stream);
  return rc != ESCOIN_OK ? rc : launch_tree_sum(p, c, c.weight_diff, c.bias_diff);
}

template <typename T>
static int weight_gradient(escoin_plan *p, const T *bottom, const T *top, const T *top_diff, T *weight_diff, T *bias_diff,
                           int n_images, hipStream_t stream, bool compact) {
  BwdState *s = p->bwd.get();
  const long total = (long)n_images * p->g.OH * p->g.OW;
  T *slab_w = s->slab.get<T>();
  const WgradCall<T> c{bottom, top, top_diff, weight_diff, bias_diff, slab_w, slab_w + (size_t)s->chunks_max * (size_t)s->nnz,
                       compact ? nullptr : s->wpos.get<int>(), n_images, (int)((total + kChunkPixels - 1) / kChunkPixels), stream};
  s->last_chunks = c.chunks;
  s->last_wgrad = s->wgrad;
  if constexpr (sizeof(T) == 4) {   // (a double plan's weight gradient is the entry kernel's: bwd_choice)
    if (s->wgrad == ESCOIN_WGRAD_STAGED) return wgrad_staged(p, c);
    if (s->wgrad == ESCOIN_WGRAD_MFMA) return wgrad_mfma(p, c);
    if (s->wgrad == ESCOIN_WGRAD_POINTWISE) return wgrad_pointwise(p, c);
  }
  return wgrad_entry<T>(p, c);
}

// option "b2s": the whole backward is the inner plan's, on X' (the bottom transposed: the weight gradient's operand) and G'
// (top_diff transposed, times [top > 0] on a fuse_relu plan; the inner plan has no ReLU and needs no top).  weight_diff,
// values_diff and bias_diff have one layout on both plans: the caller's pointers go straight through.  dX' has a scratch of
// its own (X' is read by the same inner call) and is transposed into bottom_diff.  The plan builds no state of its own.
static int backward_b2s(escoin_plan *p, const float *bottom, const float *top, const float *top_diff, float *bottom_diff,
                        float *weight_diff, float *bias_diff, int n_images, hipStream_t stream, bool compact) {
  B2sState *bs = p->b2s_state.get();
  escoin_plan *ip = bs->inner.plan.get();
  // (after device-source updates of THIS plan the inner plan's host CSR, which its backward state is built from, is stale:
  //  the values come back first, into every host mirror of the walk)
  if (!ip->bwd)
    if (const int rcs = sync_host_values(p)) return rcs;
  if (const int rc = ensure_state<float>(ip, stream)) return rc;
  if (n_images == 0 || (!bottom_diff && !weight_diff && !bias_diff)) return ESCOIN_OK;
  const int n_inner = (n_images + bs->bp.B - 1) / bs->bp.B;
  int rc = ESCOIN_OK;
  if (weight_diff) rc = g_b2s_hooks.pack(p, bottom, nullptr, bs->x.get<float>(), false, n_images, stream);
  if (rc == ESCOIN_OK) rc = g_b2s_hooks.pack(p, top_diff, p->g.d.fuse_relu ? top : nullptr, bs->t.get<float>(), true, n_images, stream);
  if (rc != ESCOIN_OK) return rc;
  rc = (compact ? escoin_backward_values : escoin_backward)(ip, weight_diff ? bs->x.get<const float>() : nullptr, nullptr,
                                                            bs->t.get<const float>(), bottom_diff ? bs->dx.get<float>() : nullptr,
                                                            weight_diff, bias_diff, n_inner, stream);
  if (rc != ESCOIN_OK || !bottom_diff) return rc;
  return g_b2s_hooks.unpack(p, bs->dx.get<const float>(), bottom_diff, false, false, n_images, stream);
}

// option "deconv": the whole backward is the inner plan's, on the caller's bottom (the weight gradient's operand) and G' (top_diff
// split into its output phases by the pack kernel, times [top > 0] on a fuse_relu plan, +0 outside the top).  The inner data
// gradient IS bottom_diff: the caller's pointer goes straight through.  The inner compact weight gradient and the inner
// bias gradient (M * P phases) land in two scratches, zeroed first (the inner plan accumulates), and are added to the
// caller's blobs by the carry and bias-sum kernels: through the entry map into values_diff, through the entries' positions
// in blobs_[0] (C x Mg x KH x KW) into weight_diff.  No atomics, nothing allocated after the inner state is built.
static int backward_d2s(escoin_plan *p, const float *bottom, const float *top, const float *top_diff, float *bottom_diff,
                        float *weight_diff, float *bias_diff, int n_images, hipStream_t stream, bool compact) {
  D2sState *ds = p->d2s_state.get();
  escoin_plan *ip = ds->inner.plan.get();
  // (after device-source updates of THIS plan the inner plan's host CSR, which its backward state is built from, is stale)
  if (!ip->bwd)
    if (const int rcs = sync_host_values(p)) return rcs;
  if (const int rc = ensure_state<float>(ip, stream)) return rc;
  if (n_images == 0 || (!bottom_diff && !weight_diff && !bias_diff)) return ESCOIN_OK;
  const long nnz = plan_nnz(p);
  int rc = g_d2s_hooks.pack(p, top_diff, p->g.d.fuse_relu ? top : nullptr, ds->t.get<float>(), n_images, stream);
  if (rc != ESCOIN_OK) return rc;
  const bool want_w = weight_diff && nnz > 0;
  if (want_w) ESCOIN_HIP_TRY(hipMemsetAsync(ds->wv.get<void>(), 0, sizeof(float) * (size_t)nnz, stream));
  if (bias_diff) ESCOIN_HIP_TRY(hipMemsetAsync(ds->bv.get<void>(), 0, ds->bv.bytes(), stream));
  rc = escoin_backward_values(ip, want_w ? bottom : nullptr, nullptr, ds->t.get<const float>(), bottom_diff,
                              want_w ? ds->wv.get<float>() : nullptr, bias_diff ? ds->bv.get<float>() : nullptr, n_images, stream);
  if (rc != ESCOIN_OK) return rc;
  if (want_w) {
    rc = g_d2s_hooks.carry(ds->wv.get<const float>(), compact ? ds->src.get<const int>() : ds->wpos.get<const int>(), weight_diff, nnz, stream);
    if (rc != ESCOIN_OK) return rc;
  }
  if (bias_diff) rc = g_d2s_hooks.bias_sum(ds->bv.get<const float>(), bias_diff, p->user_desc.M, ds->dp.P, stream);
  return rc;
}

// The driver: the checks, the state where this alignment has none yet, then the two gradients.  With the state built a
// call allocates nothing and synchronises nothing.
template <typename T>
static int backward_gpu(escoin_plan *p, const T *bottom, const T *top, const T *top_diff, T *bottom_diff,
                        T *weight_diff, T *bias_diff, int n_images, void *stream_v, bool compact) {
  if (!p) return fail(ESCOIN_EINVAL, "null plan");
  if (!p->aligned) return fail(ESCOIN_ESTATE, "backward called before weight_align / set_csr");
  if (p->is_f64 != (sizeof(T) == 8))
    return fail(ESCOIN_ESTATE, p->is_f64 ? "backward: the plan holds double weights (use the _f64 entry point)"
                                         : "backward_f64: the plan holds float weights");
  if (const int rc = check_plan_device(p, "backward")) return rc;
  if (!top_diff) return fail(ESCOIN_EINVAL, "backward: top_diff is required");
  if (p->g.d.fuse_relu && !top) return fail(ESCOIN_EINVAL, "backward: a fuse_relu plan needs the forward's top");
  if (weight_diff && !bottom) return fail(ESCOIN_EINVAL, "backward: the weight gradient needs bottom");
  if (const int rc = check_n_images(p, n_images)) return rc;
  hipStream_t stream = (hipStream_t)stream_v;
  if constexpr (sizeof(T) == 4)
    if (p->b2s_state) return backward_b2s(p, bottom, top, top_diff, bottom_diff, weight_diff, bias_diff, n_images, stream, compact);
  if constexpr (sizeof(T) == 4)
    if (p->d2s_state) return backward_d2s(p, bottom, top, top_diff, bottom_diff, weight_diff, bias_diff, n_images, stream, compact);
  if (const int rc = ensure_state<T>(p, stream)) return rc;
  if (n_images == 0) return ESCOIN_OK;
  if (bottom_diff) {
    const int rc = data_gradient<T>(p, top, top_diff, bottom_diff, n_images, stream);
    if (rc != ESCOIN_OK) return rc;
  }
  if (weight_diff || bias_diff) return weight_gradient<T>(p, bottom, top, top_diff, weight_diff, bias_diff, n_images, stream, compact);
  return ESCOIN_OK;
}

}  // namespace escoin

using namespace escoin;

extern "C" {

int escoin_backward(escoin_plan *plan, const float *bottom_dev, const float *top_dev, const float *top_diff_dev,
                    float *bottom_diff_dev, float *weight_diff_dev, float *bias_diff_dev, int n_images, void *stream) {
  return guarded([&]() -> int {
    return backward_gpu<float>(plan, bottom_dev, top_dev, top_diff_dev, bottom_diff_dev, weight_diff_dev, bias_diff_dev,
                               n_images, stream, false);
  });
}

int escoin_backward_f64(escoin_plan *plan, const double *bottom_dev, const double *top_dev, const double *top_diff_dev,
                        double *bottom_diff_dev, double *weight_diff_dev, double *bias_diff_dev, int n_images,
                        void *stream) {
  return guarded([&]() -> int {
    return backward_gpu<double>(plan, bottom_dev, top_dev, top_diff_dev, bottom_diff_dev, weight_diff_dev,
                                bias_diff_dev, n_images, stream, false);
  });
}

int escoin_backward_values(escoin_plan *plan, const float *bottom_dev, const float *top_dev, const float *top_diff_dev,
                           float *bottom_diff_dev, float *values_diff_dev, float *bias_diff_dev, int n_images,
                           void *stream) {
  return guarded([&]() -> int {
    return backward_gpu<float>(plan, bottom_dev, top_dev, top_diff_dev, bottom_diff_dev, values_diff_dev, bias_diff_dev,
                               n_images, stream, true);
  });
}

int escoin_backward_values_f64(escoin_plan *plan, const double *bottom_dev, const double *top_dev,
                               const double *top_diff_dev, double *bottom_diff_dev, double *values_diff_dev,
                               double *bias_diff_dev, int n_images, void *stream) {
  return guarded([&]() -> int {
    return backward_gpu<double>(plan, bottom_dev, top_dev, top_diff_dev, bottom_diff_dev, values_diff_dev,
                                bias_diff_dev, n_images, stream, true);
  });
}

}  // extern "C"
