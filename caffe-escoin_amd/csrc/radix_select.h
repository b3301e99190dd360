// radix_select.h -- the device-side select that prune_select.hip and rewire_select.hip share: a radix select of the
// take-th largest key among a source's candidates, then per-tile counts of N flags and their exclusive scan over the
// tiles, from which an apply kernel ranks every flagged index (tile_ranks).  Header-only, internal linkage: each of the
// two translation units instantiates the kernels over its own source.  Not part of the C ABI.
//
// A source is a small trivially-copyable struct passed by value to the kernels.  For an index i in [0, n):
//   bool candidate(long i), K key(long i)     whether i takes part in the select, and then its key (the histogram)
//   unsigned flags(long i, K T, unsigned ge)  its N flag bits under the boundary (T, ge) (count and apply)
// Every comparison is an integer comparison on key(s) = the bits of s without the sign bit (prune_rules.h).
//
// What keeps these kernels, and the apply kernels built on tile_ranks, from hanging a machine: plain C++ (no inline
// assembly); integer atomics only, whose result does not depend on their order (no float atomics); NO WORKGROUP EVER WAITS
// FOR ANOTHER WORKGROUP -- no decoupled look-back, no spin loop, no cooperative launch: a value one workgroup needs from
// another crosses a kernel boundary; every loop is bounded by n (grid strides over indices or tiles, 256 bins,
// ceil(tiles / 256) scan steps); grids are capped (prune_rules.h kMaxGrid).  Every workgroup is 256 lanes, four full waves
// of 64: no lane leaves before the last ballot or barrier of its kernel, predicates are folded into the flags.
//
//   select_init_kernel     zeroes the histograms, writes the selection state
//   select_hist_kernel     one launch per key byte, top byte first: the digit's histogram over the candidates' keys that
//                          match the prefix chosen so far -- 256 LDS bins, then one global atomic per non-empty bin
//   select_choose_kernel   one workgroup: the digit whose suffix sum reaches the remaining count; after the last pass the
//                          state holds the boundary key T and how many key == T candidates still fit
//   select_count_kernel    per tile of 1024 indices: how many carry each of the N flags
//   select_scan_kernel     one workgroup: exclusive scan of the N counts over the tiles, looping 256 tiles a step
// No host round trip between them (launch_select); a boundary known on the host skips the select.
#ifndef ESCOIN_RADIX_SELECT_H_
#define ESCOIN_RADIX_SELECT_H_

#include <hip/hip_runtime.h>

#include "prune_rules.h"

namespace escoin {
namespace {

using prune::kItems;
using prune::kThreads;
using prune::kTileEntries;

// The head of the workspace (kStateBytes).  During the select: prefix = the key bytes chosen so far, remaining = candidates
// still to take among the keys that match it.  Afterwards: prefix = T, remaining = the ties that fit.
struct SelState {
  unsigned long long prefix, remaining;
  unsigned ge, pad;
};
static_assert(sizeof(SelState) <= prune::kStateBytes, "selection state outgrew its slot");

// ws (launch_plan(n, sizeof(K), N).ws_bytes of device memory) carved into the state, one histogram per pass, N counts per tile
struct SelectWorkspace {
  SelState *st;
  unsigned *hist, *tile_cnt;
  SelectWorkspace(void *ws, const prune::LaunchPlan &lp)
      : st(static_cast<SelState *>(ws)), hist(reinterpret_cast<unsigned *>(static_cast<char *>(ws) + prune::kStateBytes)),
        tile_cnt(hist + (size_t)lp.passes * 256) {}
};

template <typename K> __device__ inline K key_mask() { return (K)(~(K)0 >> 1); }

__global__ void __launch_bounds__(256) select_init_kernel(SelState *st, unsigned *hist, int hist_words, unsigned long long prefix,
                                                           unsigned long long remaining, unsigned ge) {
  for (int i = threadIdx.x; i < hist_words; i += 256) hist[i] = 0u;
  if (threadIdx.x == 0) {
    st->prefix = prefix;
    st->remaining = remaining;
    st->ge = ge;
    st->pad = 0u;
  }
}

template <typename K, typename Src>
__global__ void __launch_bounds__(256) select_hist_kernel(const Src src, long n, int pass, int passes,
                                                           const SelState *__restrict__ st, unsigned *hist) {
  __shared__ unsigned bins[256];
  bins[threadIdx.x] = 0u;
  __syncthreads();
  const int shift = 8 * (passes - 1 - pass);
  const K prefix = (K)st->prefix;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    if (!src.candidate(i)) continue;
    const K k = src.key(i);
    if (pass == 0 || (k >> (shift + 8)) == prefix) atomicAdd(&bins[(unsigned)(k >> shift) & 0xffu], 1u);
  }
  __syncthreads();
  const unsigned c = bins[threadIdx.x];
  if (c) atomicAdd(&hist[threadIdx.x], c);
}

__global__ void __launch_bounds__(64) select_choose_kernel(SelState *st, const unsigned *__restrict__ hist) {
  if (threadIdx.x != 0) return;
  const unsigned long long remaining = st->remaining;
  unsigned long long above = 0;
  int digit = 0;
  for (int b = 255; b >= 0; --b) {
    const unsigned long long h = hist[b];
    if (above + h >= remaining) {
      digit = b;
      break;
    }
    above += h;
  }
  // (the host launches the select only for 0 < take < candidates, where the matching keys number at least `remaining`: a
  //  digit is always found; were it not, digit 0 and a clamped count keep the later kernels' arithmetic in range)
  st->remaining = remaining > above ? remaining - above : 0ull;
  st->prefix = (st->prefix << 8) | (unsigned long long)digit;
}

// the flags of item `item` of a tile for this lane; an index past n carries none
template <typename K, typename Src>
__device__ inline unsigned tile_flags(const Src &src, long tile, int item, long n, K T, unsigned ge) {
  const long i = tile * kTileEntries + item * kThreads + threadIdx.x;
  return i < n ? src.flags(i, T, ge) : 0u;
}

template <int N, typename K, typename Src>
__global__ void __launch_bounds__(256) select_count_kernel(const Src src, long n, long tiles, const SelState *__restrict__ st,
                                                            unsigned *tile_cnt) {
  __shared__ unsigned cnt[N];
  const K T = (K)st->prefix;
  const unsigned ge = st->ge;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    if (threadIdx.x < N) cnt[threadIdx.x] = 0u;
    __syncthreads();
    unsigned c[N] = {};
    for (int i = 0; i < kItems; ++i) {
      const unsigned f = tile_flags<K>(src, tile, i, n, T, ge);
      for (int k = 0; k < N; ++k) c[k] += __popcll(__ballot(f & (1u << k)));
    }
    if ((threadIdx.x & 63) == 0)
      for (int k = 0; k < N; ++k) atomicAdd(&cnt[k], c[k]);
    __syncthreads();
    if (threadIdx.x < N) tile_cnt[tile * N + threadIdx.x] = cnt[threadIdx.x];
    __syncthreads();
  }
}

// In place: tile_cnt[N t + k] becomes the number of flag-k indices in the tiles before t.
template <int N>
__global__ void __launch_bounds__(256) select_scan_kernel(long tiles, unsigned *tile_cnt) {
  __shared__ unsigned wsum[4][N];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long carry[N] = {};
  for (long base = 0; base < tiles; base += 256) {
    const long t = base + threadIdx.x;
    unsigned c[N], s[N];
    for (int k = 0; k < N; ++k) s[k] = c[k] = t < tiles ? tile_cnt[t * N + k] : 0u;
    for (int d = 1; d < 64; d <<= 1)      // inclusive scan inside the wave
      for (int k = 0; k < N; ++k) {
        const unsigned u = __shfl_up(s[k], d, 64);
        if (lane >= d) s[k] += u;
      }
    if (lane == 63)
      for (int k = 0; k < N; ++k) wsum[wave][k] = s[k];
    __syncthreads();
    for (int k = 0; k < N; ++k) {
      unsigned before = 0, all = 0;
      for (int w = 0; w < 4; ++w) {
        if (w < wave) before += wsum[w][k];
        all += wsum[w][k];
      }
      if (t < tiles) tile_cnt[t * N + k] = (unsigned)(carry[k] + before + s[k] - c[k]);
      carry[k] += all;
    }
    __syncthreads();   // wsum is rewritten by the next step
  }
}

// One tile of an apply kernel, called by all 256 lanes: visit(i, f, r) for each of this lane's kItems indices i below n,
// f its flags and r[k] the number of flag-k indices before i -- ballot / popcount ranks inside the tile plus the tile's
// scanned offsets.  A tile's order is item-major: index (item, lane) follows every index of earlier items and of earlier
// waves of its item.  The visitor only stores; it captures by value, which keeps the kernel's registers where they were
// (by-reference captures cost the apply kernels up to seven VGPRs).
template <int N, typename K, typename Src, typename Visit>
__device__ inline void tile_ranks(const Src &src, long n, long tile, K T, unsigned ge, const unsigned *__restrict__ tile_off,
                                  Visit &&visit) {
  __shared__ unsigned wsum[kItems][4][N];
  const int wave = threadIdx.x >> 6;
  unsigned f[kItems], in[kItems][N];   // flags; flag-k indices before this lane in its wave
  for (int i = 0; i < kItems; ++i) {
    f[i] = tile_flags<K>(src, tile, i, n, T, ge);
    for (int k = 0; k < N; ++k) {
      const unsigned long long b = __ballot(f[i] & (1u << k));
      in[i][k] = __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
      if ((threadIdx.x & 63) == 0) wsum[i][wave][k] = __popcll(b);
    }
  }
  __syncthreads();
  unsigned long long run[N];
  for (int k = 0; k < N; ++k) run[k] = tile_off[tile * N + k];
  for (int i = 0; i < kItems; ++i) {
    unsigned before[N] = {}, all[N] = {};
    for (int k = 0; k < N; ++k)
      for (int w = 0; w < 4; ++w) {
        if (w < wave) before[k] += wsum[i][w][k];
        all[k] += wsum[i][w][k];
      }
    const long at = tile * kTileEntries + i * kThreads + threadIdx.x;
    if (at < n) {   // (after the last ballot and barrier that read this lane's flags: only the stores are skipped)
      unsigned long long r[N];
      for (int k = 0; k < N; ++k) r[k] = run[k] + before[k] + in[i][k];
      visit(at, f[i], r);
    }
    for (int k = 0; k < N; ++k) run[k] += all[k];
  }
  __syncthreads();   // wsum is rewritten by the next tile
}

// The launches on `stream` that leave the boundary in w.st and the scanned tile offsets in w.tile_cnt: init, (take > 0: a
// select of the take-th largest candidate key, one histogram and one choose launch per key byte; take == 0: the boundary
// `b` as given), count, scan.  0 <= take < candidates; lp: launch_plan(n, sizeof(K), N).  Asynchronous.
template <int N, typename K, typename Src>
inline void launch_select(const Src &src, long n, const prune::LaunchPlan &lp, const SelectWorkspace &w, const prune::Boundary<K> &b,
                          long take, hipStream_t stream) {
  const dim3 block(kThreads);
  hipLaunchKernelGGL(select_init_kernel, dim3(1), block, 0, stream, w.st, w.hist, lp.passes * 256, (unsigned long long)(take ? 0 : b.T),
                     (unsigned long long)take, (unsigned)(take ? 0 : b.ge));
  for (int pass = 0; take && pass < lp.passes; ++pass) {
    hipLaunchKernelGGL((select_hist_kernel<K, Src>), dim3(lp.hist_grid), block, 0, stream, src, n, pass, lp.passes, (const SelState *)w.st,
                       w.hist + (size_t)pass * 256);
    hipLaunchKernelGGL(select_choose_kernel, dim3(1), dim3(64), 0, stream, w.st, (const unsigned *)(w.hist + (size_t)pass * 256));
  }
  hipLaunchKernelGGL((select_count_kernel<N, K, Src>), dim3(lp.tile_grid), block, 0, stream, src, n, lp.tiles, (const SelState *)w.st,
                     w.tile_cnt);
  hipLaunchKernelGGL((select_scan_kernel<N>), dim3(1), block, 0, stream, lp.tiles, w.tile_cnt);
}

}  // namespace
}  // namespace escoin
#endif
