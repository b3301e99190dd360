// depthwise.hip -- the kernel pair of plan option "depthwise": layers with one input channel per conv group (Cg == 1; Mg is
// the channel multiplier).  Such a layer does 2 x taps flops per output element and moves 8 bytes per element: it is bound by
// HBM, and the kernels' job is to read every bottom (top_diff) element once, keep the plane in LDS and write every top
// (bottom_diff) element once.  The plan: align_rules.h dw_plan (DwPlan); the weights: the generic kernel's device CSR
// (gen.rowptr / taps / vals), which every in-place update writes -- no copy of the values of its own.
//
// Work split (both kernels): a workgroup has kDwWaves waves and every wave takes one work unit with a PRIVATE LDS region.
// The waves of a workgroup never wait for each other -- there is no workgroup barrier -- and everything derived from the
// unit (the CSR row, its taps and values) is wave-uniform and comes in through scalar loads.
//
//   escoin_depthwise_kernel<RELU, P>        unit = (image, conv group, band of output rows).  The wave copies the band's
//       input window into its region once -- coalesced, 16 bytes per lane where the row allows it, the halo and the padding
//       written as +0 in the same pass -- and then, for each of the group's Mg output channels, every lane keeps up to
//       kDwLaneItems runs of P consecutive output pixels in registers and walks the channel's CSR row in order: sum =
//       fmaf(v, x, sum) from +0, one LDS read per tap and pixel; then the bias once, the optional ReLU, one store per run.
//       That is the loop nest of escoin_sconv_generic_kernel (a padded tap is multiplied as a zero there too): the top blob
//       is bit-identical to KERNEL_GENERIC's, whatever the banding.
//   escoin_depthwise_dgrad_kernel<RELU, P, S1>   unit = (image, input channel, band of bottom rows).  For ocl = 0 .. Mg - 1
//       in turn the wave stages the top_diff rows the band receives from (0 where top <= 0 under fuse_relu) and walks that
//       output channel's CSR row; the lanes keep their bottom pixels' sums in registers across ocl.  Entry (kr, kc) contributes
//       to pixel (h, w) when h + pad_h - kr * dil_h is a non-negative multiple of stride_h with a quotient below OH, and
//       likewise in w; another entry is skipped (a per-lane predicate), not multiplied by a zero.  Per bottom pixel that is
//       the gather kernel's chain -- ascending (ocl, kr, kc), one fmaf per contributing entry from +0 -- so bottom_diff is
//       bit-identical to backward_kernel = GENERIC's.  S1: stride_w == 1, where a tap's column offset is wave-uniform.
//
//   escoin_depthwise_wgrad_kernel<RELU, P>   (plan option "wgrad_depthwise": stage 1 of the weight / bias gradient; align_rules.h
//       DwwPlan)  unit = (row segment, slice): up to kDwwSegEntries consecutive CSR entries of one output channel's row, and a
//       contiguous run of the call's (image, band of output rows) pairs, bands being the forward's.  Per pair the wave stages
//       the band's input window as the forward does, every lane loads top_diff for its runs of P output pixels from global
//       memory into registers (the forward's item / run mapping; 0 where top <= 0 under fuse_relu), and the segment's entries
//       are walked: acc[k] = fmaf(g, win[base + at_k], acc[k]) per owned pixel, items and pixels ascending -- one LDS read
//       per fma, the forward's addresses.  The accumulators are statically indexed registers that live across the slice; the
//       unit ends with one 64-lane butterfly per entry and lane 0's store of one partial per (slice, entry) into the slab of
//       sconv_backward.hip, whose tree sum is stage 2 over the slices.  A row's first segment also sums the lane's g: the bias.
//       A padded tap is multiplied as a zero; a dead lane or a dead pixel of a run is left out by a select, so a non-finite
//       bottom element reaches only the entries whose tap reads it.  A bias-only call has one unit per (output channel,
//       slice) and stages nothing.
//
// LDS layout (align_rules.h): a row is de-interleaved by P -- column x lies at (x % P) * (pitch / P) + x / P -- so that for
// one tap the lanes of a wave, whose runs start P columns apart, read consecutive words.  Blob bases are 64-bit; offsets
// inside a plane fit 32 bits (dw_plan).  No atomics; a launch allocates and synchronises nothing.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>
#include <vector>

#include "align_rules.h"
#include "csr_tables.h"
#include "escoin_plan.h"

namespace escoin {

namespace {

constexpr int kDwThreads = 64 * kDwWaves;

struct DwArgs {
  const float *__restrict__ src;     // forward: bottom; data gradient: top_diff
  const float *__restrict__ mask;    // data gradient under fuse_relu: top
  float *__restrict__ dst;           // forward: top; data gradient: bottom_diff
  const int *__restrict__ rowptr;
  const int *__restrict__ taps;
  const float *__restrict__ vals;
  const float *__restrict__ bias;    // forward only
  escoin_conv_desc d;
  int OH, OW, Mg;
  int band, nbands, padl, pitch, region;   // region: floats per wave
  int units;
  int vec_src, vec_dst;              // 16-byte loads of the staging pass / one store per run
  S2dDiv by_sh, by_sw;               // data gradient: the divisions by the strides
};

template <int P> __device__ inline int dw_pos(int x, int q_per_row) {
  constexpr int lg = P == 4 ? 2 : P == 2 ? 1 : 0;
  return (x & (P - 1)) * q_per_row + (x >> lg);
}

// Stages `rows` rows of `width` floats (row r at src + (size_t)r * width for first_row + r in [0, limit), +0 elsewhere) into the
// region, window column x = row column x - shift; every word of rows x pitch is written.
template <int P, bool MASK>
__device__ inline void dw_stage(float *win, const float *__restrict__ src, const float *__restrict__ mask, int first_row, int rows,
                                int limit, int width, int shift, int pitch, bool vec, int lane) {
  const int qpr = pitch >> 2, Q = pitch / P;
  for (int idx = lane; idx < rows * qpr; idx += 64) {
    const int r = idx / qpr, q = idx - r * qpr;
    const int ir = first_row + r, c0 = 4 * q - shift;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if ((unsigned)ir < (unsigned)limit) {
      const int off = ir * width + c0;
      if (vec && c0 >= 0 && c0 + 3 < width) {
        const float4 t = *reinterpret_cast<const float4 *>(src + off);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        if (MASK) {
          const float4 m = *reinterpret_cast<const float4 *>(mask + off);
          v[0] = m.x > 0.f ? v[0] : 0.f; v[1] = m.y > 0.f ? v[1] : 0.f;
          v[2] = m.z > 0.f ? v[2] : 0.f; v[3] = m.w > 0.f ? v[3] : 0.f;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if ((unsigned)(c0 + e) < (unsigned)width) {
            v[e] = src[off + e];
            if (MASK && !(mask[off + e] > 0.f)) v[e] = 0.f;
          }
      }
    }
    float *row = win + r * pitch;
#pragma unroll
    for (int e = 0; e < 4; ++e) row[dw_pos<P>(4 * q + e, Q)] = v[e];
  }
  // the wave's own writes, read below by other lanes of the same wave: LDS serves a wave's requests in order
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One run of P results: a single store where the launch allows it
template <int P>
__device__ inline void dw_store(float *__restrict__ out, const float (&s)[P], int col, int width, bool vec) {
  if (P == 4 && vec) {
    *reinterpret_cast<float4 *>(out) = make_float4(s[0], s[1], s[2], s[3]);
  } else if (P == 2 && vec) {
    *reinterpret_cast<float2 *>(out) = make_float2(s[0], s[1]);
  } else {
#pragma unroll
    for (int q = 0; q < P; ++q)
      if (col + q < width) out[q] = s[q];
  }
}

// One run of P values (P = 4 or 2) in a single aligned load
template <int P>
__device__ inline void dw_load(const float *__restrict__ in, float (&s)[P]) {
  if constexpr (P == 4) {
    const float4 t = *reinterpret_cast<const float4 *>(in);
    s[0] = t.x; s[1] = t.y; s[2] = t.z; s[3] = t.w;
  } else {
    const float2 t = *reinterpret_cast<const float2 *>(in);
    s[0] = t.x; s[1] = t.y;
  }
}

}  // namespace

template <bool RELU, int P>
__global__ void __launch_bounds__(kDwThreads)
escoin_depthwise_kernel(DwArgs a) {
  extern __shared__ float dw_lds[];
  const escoin_conv_desc &d = a.d;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int unit = __builtin_amdgcn_readfirstlane(blockIdx.x * kDwWaves + wave);
  if (unit >= a.units) return;
  float *win = dw_lds + wave * a.region;
  const int per_image = d.group * a.nbands;
  const int n = unit / per_image, rest = unit - n * per_image;
  const int grp = rest / a.nbands, b = rest - grp * a.nbands;
  const int o0 = b * a.band, o1 = min(a.OH, o0 + a.band);
  int first, rows;
  dw_window(d, o0, o1, &first, &rows);
  dw_stage<P, false>(win, a.src + ((size_t)n * d.C + grp) * ((size_t)d.H * d.W), nullptr, first, rows, d.H, d.W, a.padl, a.pitch,
                     a.vec_src != 0, lane);
  const int Q = a.pitch / P;
  const int runs = (a.OW + P - 1) / P, items = (o1 - o0) * runs;
  const int col0 = a.padl - d.pad_w;
  const size_t opix = (size_t)a.OH * a.OW;
  for (int ocl = 0; ocl < a.Mg; ++ocl) {
    const int oc = grp * a.Mg + ocl;
    const int jb = a.rowptr[oc], je = a.rowptr[oc + 1];
    float *__restrict__ out = a.dst + ((size_t)n * d.M + oc) * opix;
    for (int it0 = 0; it0 < items; it0 += 64 * kDwLaneItems) {
      const int ni = min(kDwLaneItems, (items - it0 + 63) >> 6);   // wave-uniform
      float acc[kDwLaneItems][P];
      int base[kDwLaneItems], opos[kDwLaneItems], ocol[kDwLaneItems];
#pragma unroll
      for (int i = 0; i < kDwLaneItems; ++i) {
        const int it = it0 + i * 64 + lane;
        const int itc = it < items ? it : 0;       // (a dead lane reads item 0's window and stores nothing)
        const int row = itc / runs, run = itc - row * runs;
        base[i] = row * d.stride_h * a.pitch + run * d.stride_w;
        ocol[i] = it < items ? run * P : a.OW;
        opos[i] = (o0 + row) * a.OW + run * P;
#pragma unroll
        for (int q = 0; q < P; ++q) acc[i][q] = 0.f;
      }
      for (int j = jb; j < je; ++j) {
        const int tap = a.taps[j];
        const float v = a.vals[j];
        const int kr = (tap >> 8) & 0xff, kc = tap & 0xff;
        int at[P];
#pragma unroll
        for (int q = 0; q < P; ++q) at[q] = kr * d.dil_h * a.pitch + dw_pos<P>(q * d.stride_w + kc * d.dil_w + col0, Q);
#pragma unroll
        for (int i = 0; i < kDwLaneItems; ++i)
          if (i < ni) {
#pragma unroll
            for (int q = 0; q < P; ++q) acc[i][q] = fmaf(v, win[base[i] + at[q]], acc[i][q]);
          }
      }
#pragma unroll
      for (int i = 0; i < kDwLaneItems; ++i)
        if (i < ni && ocol[i] < a.OW) {
          float s[P];
#pragma unroll
          for (int q = 0; q < P; ++q) {
            s[q] = acc[i][q];
            if (a.bias) s[q] += a.bias[oc];
            if (RELU) s[q] = s[q] > 0.f ? s[q] : 0.f;
          }
          dw_store<P>(out + opos[i], s, ocol[i], a.OW, a.vec_dst != 0);
        }
    }
  }
}

template <bool RELU, int P, bool S1>
__global__ void __launch_bounds__(kDwThreads)
escoin_depthwise_dgrad_kernel(DwArgs a) {
  extern __shared__ float dw_lds[];
  const escoin_conv_desc &d = a.d;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int unit = __builtin_amdgcn_readfirstlane(blockIdx.x * kDwWaves + wave);
  if (unit >= a.units) return;
  float *win = dw_lds + wave * a.region;
  const int per_image = d.C * a.nbands;
  const int n = unit / per_image, rest = unit - n * per_image;
  const int c = rest / a.nbands, b = rest - c * a.nbands;
  const int h0 = b * a.band, h1 = min(d.H, h0 + a.band);
  int tfirst, trows;
  dw_top_rows(d, a.OH, h0, h1, &tfirst, &trows);
  const int Q = a.pitch / P;
  const int runs = (d.W + P - 1) / P, items = (h1 - h0) * runs;
  const size_t opix = (size_t)a.OH * a.OW;
  float *__restrict__ out = a.dst + ((size_t)n * d.C + c) * ((size_t)d.H * d.W);
  for (int it0 = 0; it0 < items; it0 += 64 * kDwLaneItems) {
    const int ni = min(kDwLaneItems, (items - it0 + 63) >> 6);   // wave-uniform
    float acc[kDwLaneItems][P];
    int hrow[kDwLaneItems], wcol[kDwLaneItems], ocol[kDwLaneItems];
#pragma unroll
    for (int i = 0; i < kDwLaneItems; ++i) {
      const int it = it0 + i * 64 + lane;
      const int itc = it < items ? it : 0;
      const int row = itc / runs, run = itc - row * runs;
      hrow[i] = h0 + row + d.pad_h;
      wcol[i] = run * P;
      ocol[i] = it < items ? run * P : d.W;
#pragma unroll
      for (int q = 0; q < P; ++q) acc[i][q] = 0.f;
    }
    for (int ocl = 0; ocl < a.Mg && trows > 0; ++ocl) {
      const int oc = c * a.Mg + ocl;           // (Cg == 1: the conv group is the input channel)
      const size_t plane = ((size_t)n * d.M + oc) * opix;
      dw_stage<P, RELU>(win, a.src + plane, RELU ? a.mask + plane : nullptr, tfirst, trows, a.OH, a.OW, 0, a.pitch, a.vec_src != 0,
                        lane);
      const int jb = a.rowptr[oc], je = a.rowptr[oc + 1];
      for (int j = jb; j < je; ++j) {
        const int tap = a.taps[j];
        const float v = a.vals[j];
        const int kr = (tap >> 8) & 0xff, kc = tap & 0xff;
        const int dh = kr * d.dil_h, dw = d.pad_w - kc * d.dil_w;
#pragma unroll
        for (int i = 0; i < kDwLaneItems; ++i)
          if (i < ni) {
            const int th = hrow[i] - dh;
            const int oh = d.stride_h == 1 ? th : (int)s2d_div((unsigned)max(th, 0), a.by_sh);
            const bool okh = th >= 0 && oh * d.stride_h == th && oh < a.OH;
            const int lrow = (oh - tfirst) * a.pitch;
#pragma unroll
            for (int q = 0; q < P; ++q) {
              bool ok;
              int at;
              if (S1) {
                // ow = wcol + (q + dw): the run's start is a multiple of P, the rest wave-uniform
                ok = okh && (unsigned)(wcol[i] + q + dw) < (unsigned)a.OW;
                at = lrow + (wcol[i] / P) + dw_pos<P>(q + dw, Q);
              } else {
                const int tw = wcol[i] + q + dw;
                const int ow = (int)s2d_div((unsigned)max(tw, 0), a.by_sw);
                ok = okh && tw >= 0 && ow * d.stride_w == tw && ow < a.OW;
                at = lrow + dw_pos<P>(ow, Q);
              }
              const float g = win[ok ? at : 0];
              acc[i][q] = ok ? fmaf(v, g, acc[i][q]) : acc[i][q];
            }
          }
      }
      // the next output channel's rows overwrite the region: the reads above were issued before those writes
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int i = 0; i < kDwLaneItems; ++i)
      if (i < ni && ocol[i] < d.W)
        dw_store<P>(out + (hrow[i] - d.pad_h) * d.W + ocol[i], acc[i], ocol[i], d.W, a.vec_dst != 0);
  }
}

struct DwwArgs {
  const float *__restrict__ bottom;
  const float *__restrict__ top_diff;
  const float *__restrict__ top;     // fuse_relu only
  const int *__restrict__ rowptr;
  const int *__restrict__ taps;
  const int *__restrict__ seg;       // [nseg][kDwwSegWords]; unread by a bias-only call
  float *__restrict__ slab_w;        // [slices][nnz]; null: a bias-only call, whose segments are the output channels
  float *__restrict__ slab_b;        // [slices][M]; null: no bias
  escoin_conv_desc d;
  int OH, OW, Mg;
  int band, nbands, padl, pitch, region;
  int nseg, slices, per, pairs;      // units = nseg * slices; pairs = n_images * nbands
  int nnz;
  int vec_src, vec_g;                // 16-byte loads of the staging pass / one load per run of top_diff
};

template <bool RELU, int P>
__global__ void __launch_bounds__(kDwThreads)
escoin_depthwise_wgrad_kernel(DwwArgs a) {
  extern __shared__ float dw_lds[];
  const escoin_conv_desc &d = a.d;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int unit = __builtin_amdgcn_readfirstlane(blockIdx.x * kDwWaves + wave);
  if (unit >= a.nseg * a.slices) return;
  float *win = dw_lds + wave * a.region;
  const int slice = unit / a.nseg, sg = unit - slice * a.nseg;
  const bool bias_only = a.slab_w == nullptr;
  const int oc = bias_only ? sg : a.seg[kDwwSegWords * sg];
  const int first = bias_only ? 0 : a.seg[kDwwSegWords * sg + 1];
  const int cnt = bias_only ? 0 : a.seg[kDwwSegWords * sg + 2];
  const bool bias = a.slab_b != nullptr && (bias_only || first == a.rowptr[oc]);   // a row's first segment owns its bias
  const int grp = oc / a.Mg;
  const int Q = a.pitch / P;
  const int runs = (a.OW + P - 1) / P;
  const int col0 = a.padl - d.pad_w;
  const size_t opix = (size_t)a.OH * a.OW;
  float acc[kDwwSegEntries];
#pragma unroll
  for (int k = 0; k < kDwwSegEntries; ++k) acc[k] = 0.f;
  float accb = 0.f;
  const int p0 = slice * a.per, p1 = min(a.pairs, p0 + a.per);
  for (int pr = p0; pr < p1; ++pr) {
    const int n = pr / a.nbands, b = pr - n * a.nbands;
    const int o0 = b * a.band, o1 = min(a.OH, o0 + a.band);
    const int items = (o1 - o0) * runs;
    if (cnt > 0) {
      int wfirst, wrows;
      dw_window(d, o0, o1, &wfirst, &wrows);
      dw_stage<P, false>(win, a.bottom + ((size_t)n * d.C + grp) * ((size_t)d.H * d.W), nullptr, wfirst, wrows, d.H, d.W, a.padl, a.pitch,
                         a.vec_src != 0, lane);
    }
    const size_t plane = ((size_t)n * d.M + oc) * opix;
    const float *__restrict__ gsrc = a.top_diff + plane;
    const float *__restrict__ msrc = RELU ? a.top + plane : nullptr;
    for (int it0 = 0; it0 < items; it0 += 64 * kDwLaneItems) {
      const int ni = min(kDwLaneItems, (items - it0 + 63) >> 6);   // wave-uniform
      float g[kDwLaneItems][P];
      int base[kDwLaneItems], nlive[kDwLaneItems];   // nlive: the run's live pixels, 0 on a dead lane
#pragma unroll
      for (int i = 0; i < kDwLaneItems; ++i) {
        const int it = it0 + i * 64 + lane;
        const bool on = i < ni && it < items;
        const int itc = on ? it : 0;               // (a dead lane reads item 0's window and contributes nothing)
        const int row = itc / runs, run = itc - row * runs;
        base[i] = row * d.stride_h * a.pitch + run * d.stride_w;
        const int col = run * P, opos = (o0 + row) * a.OW + col;
        nlive[i] = on ? min(P, a.OW - col) : 0;
#pragma unroll
        for (int q = 0; q < P; ++q) g[i][q] = 0.f;
        bool vec = false;
        if constexpr (P > 1) {
          vec = a.vec_g != 0;                      // (OW is a multiple of P: a live run has P live pixels)
          if (vec && on) {
            dw_load<P>(gsrc + opos, g[i]);
            if (RELU) {
              float m[P];
              dw_load<P>(msrc + opos, m);
#pragma unroll
              for (int q = 0; q < P; ++q) g[i][q] = m[q] > 0.f ? g[i][q] : 0.f;
            }
          }
        }
        if (!vec) {
#pragma unroll
          for (int q = 0; q < P; ++q)
            if (q < nlive[i]) {
              g[i][q] = gsrc[opos + q];
              if (RELU && !(msrc[opos + q] > 0.f)) g[i][q] = 0.f;
            }
        }
      }
      // every lane's every pixel of this pass is live (wave-uniform): no select
      const bool full = it0 + ni * 64 <= items && runs * P == a.OW;
      auto walk = [&](auto sel) __attribute__((always_inline)) {
        constexpr bool SEL = decltype(sel)::value;
        if (bias) {
#pragma unroll
          for (int i = 0; i < kDwLaneItems; ++i)
            if (i < ni) {
#pragma unroll
              for (int q = 0; q < P; ++q) accb = !SEL || q < nlive[i] ? accb + g[i][q] : accb;
            }
        }
#pragma unroll
        for (int k = 0; k < kDwwSegEntries; ++k)
          if (k < cnt) {                           // wave-uniform: acc[k] is a register
            const int tap = a.taps[first + k];
            const int kr = (tap >> 8) & 0xff, kc = tap & 0xff;
            int at[P];
#pragma unroll
            for (int q = 0; q < P; ++q) at[q] = kr * d.dil_h * a.pitch + dw_pos<P>(q * d.stride_w + kc * d.dil_w + col0, Q);
#pragma unroll
            for (int i = 0; i < kDwLaneItems; ++i)
              if (i < ni) {
#pragma unroll
                for (int q = 0; q < P; ++q) {
                  const float x = win[base[i] + at[q]];
                  acc[k] = !SEL || q < nlive[i] ? fmaf(g[i][q], x, acc[k]) : acc[k];
                }
              }
          }
      };
      if (full) walk(std::false_type());
      else walk(std::true_type());
    }
    // the next pair's window overwrites the region: the reads above were issued before those writes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  // the pairing of sconv_backward.hip's wave_sum: the same tree on every call
#pragma unroll
  for (int k = 0; k < kDwwSegEntries; ++k)
    if (k < cnt) {
      float v = acc[k];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
      if (lane == 0) a.slab_w[(size_t)slice * a.nnz + first + k] = v;
    }
  if (bias) {
    float v = accb;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) a.slab_b[(size_t)slice * d.M + oc] = v;
  }
}

namespace {

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

void fill_args(const escoin_plan *p, DwArgs *a) {
  const Geometry &g = p->g;
  a->rowptr = p->gen.rowptr.get<int>();
  a->taps = p->gen.taps.get<int>();
  a->vals = p->gen.vals.get<float>();
  a->d = g.d;
  a->OH = g.OH; a->OW = g.OW; a->Mg = g.Mg;
  a->by_sh = s2d_div_make((unsigned)g.d.stride_h);
  a->by_sw = s2d_div_make((unsigned)g.d.stride_w);
}

template <bool RELU>
void launch_fwd(int px, dim3 grid, size_t lds, hipStream_t stream, const DwArgs &a) {
  if (px == 4) hipLaunchKernelGGL((escoin_depthwise_kernel<RELU, 4>), grid, dim3(kDwThreads), lds, stream, a);
  else if (px == 2) hipLaunchKernelGGL((escoin_depthwise_kernel<RELU, 2>), grid, dim3(kDwThreads), lds, stream, a);
  else hipLaunchKernelGGL((escoin_depthwise_kernel<RELU, 1>), grid, dim3(kDwThreads), lds, stream, a);
}

template <bool RELU, bool S1>
void launch_bwd(int px, dim3 grid, size_t lds, hipStream_t stream, const DwArgs &a) {
  if (px == 4) hipLaunchKernelGGL((escoin_depthwise_dgrad_kernel<RELU, 4, S1>), grid, dim3(kDwThreads), lds, stream, a);
  else if (px == 2) hipLaunchKernelGGL((escoin_depthwise_dgrad_kernel<RELU, 2, S1>), grid, dim3(kDwThreads), lds, stream, a);
  else hipLaunchKernelGGL((escoin_depthwise_dgrad_kernel<RELU, 1, S1>), grid, dim3(kDwThreads), lds, stream, a);
}

}  // namespace

static int launch_depthwise(const escoin_plan *p, const DwPlan &dp, const float *bottom, const float *bias, float *top, int n_images,
                     hipStream_t stream) {
  const Geometry &g = p->g;
  DwArgs a = {};
  fill_args(p, &a);
  a.src = bottom; a.dst = top; a.bias = bias;
  a.band = dp.band; a.nbands = dp.nbands; a.padl = dp.padl; a.pitch = dp.pitch; a.region = dp.rows * dp.pitch;
  a.units = (int)((long)n_images * g.d.group * dp.nbands);      // (within kDwMaxUnits: dw_plan)
  a.vec_src = aligned16(bottom) && g.d.W % 4 == 0;
  a.vec_dst = aligned16(top) && g.OW % dp.px == 0;
  const dim3 grid((unsigned)((a.units + kDwWaves - 1) / kDwWaves));
  if (g.d.fuse_relu) launch_fwd<true>(dp.px, grid, dp.lds_bytes, stream, a);
  else launch_fwd<false>(dp.px, grid, dp.lds_bytes, stream, a);
  ESCOIN_HIP_TRY(hipGetLastError());
  return ESCOIN_OK;
}

static int launch_depthwise_dgrad(const escoin_plan *p, const DwPlan &dp, const float *top, const float *top_diff, float *bottom_diff,
                           int n_images, hipStream_t stream) {
  const Geometry &g = p->g;
  DwArgs a = {};
  fill_args(p, &a);
  a.src = top_diff; a.mask = top; a.dst = bottom_diff;
  a.band = dp.dband; a.nbands = dp.dnbands; a.padl = 0; a.pitch = dp.dpitch; a.region = (dp.drows > 0 ? dp.drows : 1) * dp.dpitch;
  a.units = (int)((long)n_images * g.d.C * dp.dnbands);
  a.vec_src = aligned16(top_diff) && (!g.d.fuse_relu || aligned16(top)) && g.OW % 4 == 0;
  a.vec_dst = aligned16(bottom_diff) && g.d.W % dp.dpx == 0;
  const dim3 grid((unsigned)((a.units + kDwWaves - 1) / kDwWaves));
  const bool s1 = g.d.stride_w == 1;
  if (g.d.fuse_relu) {
    if (s1) launch_bwd<true, true>(dp.dpx, grid, dp.dlds_bytes, stream, a);
    else launch_bwd<true, false>(dp.dpx, grid, dp.dlds_bytes, stream, a);
  } else {
    if (s1) launch_bwd<false, true>(dp.dpx, grid, dp.dlds_bytes, stream, a);
    else launch_bwd<false, false>(dp.dpx, grid, dp.dlds_bytes, stream, a);
  }
  ESCOIN_HIP_TRY(hipGetLastError());
  return ESCOIN_OK;
}

// option "wgrad_depthwise": the segments of the plan's CSR, the rule on their count with the options bwd_choice read
static int dww_build(const escoin_plan *p, const BwdOptions &o, DwWgrad *w, hipStream_t stream) {
  w->host_seg = dww_segments(csr_view(p));
  const long nseg = (long)(w->host_seg.size() / kDwwSegWords);
  if (!dww_plan(p->g, p->is_f64, plan_nnz(p), nseg, o.dw_band_rows, o.dww_slices, tiled_device_cus(), &w->plan))
    return fail(ESCOIN_ESTATE, "depthwise weight-gradient kernel: the rule does not serve this plan");
  w->nseg = (int)nseg;
  ESCOIN_HIP_TRY(w->seg.upload(w->host_seg, stream));   // (bwd_build synchronises)
  return ESCOIN_OK;
}

template <bool RELU>
static void launch_dww(int px, dim3 grid, size_t lds, hipStream_t stream, const DwwArgs &a) {
  if (px == 4) hipLaunchKernelGGL((escoin_depthwise_wgrad_kernel<RELU, 4>), grid, dim3(kDwThreads), lds, stream, a);
  else if (px == 2) hipLaunchKernelGGL((escoin_depthwise_wgrad_kernel<RELU, 2>), grid, dim3(kDwThreads), lds, stream, a);
  else hipLaunchKernelGGL((escoin_depthwise_wgrad_kernel<RELU, 1>), grid, dim3(kDwThreads), lds, stream, a);
}

static int launch_depthwise_wgrad(const escoin_plan *p, DwWgrad *w, long nnz, const float *bottom, const float *top, const float *top_diff,
                                  float *slab_w, float *slab_b, int n_images, int *slices, hipStream_t stream) {
  const Geometry &g = p->g;
  const DwwPlan &wp = w->plan;
  *slices = w->last_slices = 0;
  const bool want_w = slab_w != nullptr && nnz > 0, want_b = slab_b != nullptr;
  if ((!want_w && !want_b) || n_images <= 0) return ESCOIN_OK;     // nothing to produce: no launch
  if (!w->seg.get<void>() || wp.per <= 0) return fail(ESCOIN_ESTATE, "depthwise weight-gradient kernel: the backward state has no segments for it");
  DwwArgs a = {};
  a.bottom = bottom; a.top_diff = top_diff; a.top = top;
  a.rowptr = p->gen.rowptr.get<int>(); a.taps = p->gen.taps.get<int>(); a.seg = w->seg.get<const int>();
  a.slab_w = want_w ? slab_w : nullptr; a.slab_b = slab_b;
  a.d = g.d;
  a.OH = g.OH; a.OW = g.OW; a.Mg = g.Mg;
  a.band = wp.band; a.nbands = wp.nbands; a.padl = wp.padl; a.pitch = wp.pitch; a.region = wp.rows * wp.pitch;
  a.pairs = n_images * wp.nbands;                       // (n_images <= N: within kDwMaxUnits, dw_plan)
  a.slices = wp.slices(n_images);                       // (<= S: the slab's rows)
  a.per = wp.per;
  a.nseg = want_w ? w->nseg : g.d.M;                    // the bias alone: one unit per (output channel, slice), nothing staged
  a.nnz = (int)nnz;
  a.vec_src = aligned16(bottom) && g.d.W % 4 == 0;
  a.vec_g = aligned16(top_diff) && (!g.d.fuse_relu || aligned16(top)) && g.OW % wp.px == 0;
  const long units = (long)a.nseg * a.slices;           // (within kDwMaxUnits: dww_plan)
  const dim3 grid((unsigned)((units + kDwWaves - 1) / kDwWaves));
  const size_t lds = want_w ? wp.lds_bytes : 0;
  if (g.d.fuse_relu) launch_dww<true>(wp.px, grid, lds, stream, a);
  else launch_dww<false>(wp.px, grid, lds, stream, a);
  ESCOIN_HIP_TRY(hipGetLastError());
  *slices = w->last_slices = a.slices;
  return ESCOIN_OK;
}

// (the plan's core -- escoin_capi.hip, sconv_backward.hip -- reaches these through g_dw_hooks: escoin_plan.h)
namespace {
__attribute__((used)) const bool g_registered =
    (g_dw_hooks = DwHooks{launch_depthwise, launch_depthwise_dgrad, {"escoin_depthwise_kernel<false>", "escoin_depthwise_kernel<true>"},
                          dww_build, launch_depthwise_wgrad}, true);
}  // namespace

}  // namespace escoin
