// prune_select.hip -- magnitude pruning of an aligned plan on the device (include/escoin.h, "Pruning"): the selection
// kernels, the entry map, escoin_compact_entries, and the entry points that re-align the plan on the kept entries.
//
// The rule is prune_rules.h's: key(s) = the bits of s without the sign bit, an unsigned integer; KEEP keeps the first
// min(keep, nnz) entries by (key descending, entry index ascending), THRESHOLD the entries with key >= key(threshold).
// Every comparison below is an integer comparison.
//
// What keeps these kernels from hanging a machine: plain C++ (no inline assembly); integer atomics only, whose result does
// not depend on their order (no float atomics); NO WORKGROUP EVER WAITS FOR ANOTHER WORKGROUP -- no decoupled look-back, no
// spin loop, no cooperative launch: a value one workgroup needs from another crosses a kernel boundary; every loop is
// bounded by nnz (grid strides over entries or tiles, 256 bins, ceil(tiles / 256) scan steps); grids are capped
// (prune_rules.h kMaxGrid; the compact kernel's is ceil(nnz / 256)).  Every workgroup is 256 lanes, four full waves of
// 64: no lane leaves before the last ballot or barrier of its kernel, predicates are folded into the flags.
//
//   escoin_prune_init_kernel      zeroes the histograms, writes the selection state
//   escoin_prune_hist_kernel      one launch per key byte, top byte first: the digit's histogram over the keys that match
//                                 the prefix chosen so far -- 256 LDS bins, then one global atomic per non-empty bin
//   escoin_prune_choose_kernel    one workgroup: the digit whose suffix sum reaches the remaining count; after the last
//                                 pass the state holds the boundary key T and how many key == T entries still fit
//   escoin_prune_count_kernel     per tile of 1024 entries: how many are kept strictly (key > T) and how many tie
//   escoin_prune_scan_kernel      one workgroup: exclusive scan of both counts over the tiles, looping 256 tiles a step
//   escoin_prune_apply_kernel     per tile: ballot / popcount ranks inside the tile, plus the tile's offsets ->
//                                 entry_map[e] = kept-strictly before e + min(ties before e, ties that fit), or -1
//   escoin_compact_kernel         dst[entry_map[e]] = src[e], one lane per old entry, one plain store
// No host round trip between them; THRESHOLD mode and the trivial KEEP cases skip the select.
// The launch sequence, the descriptor check and the host form of the map are shared with rewire_select.hip (prune_select.h).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "escoin_plan.h"
#include "prune_rules.h"
#include "prune_select.h"

namespace escoin {
namespace {

using prune::kItems;
using prune::kThreads;
using prune::kTileEntries;
using prune::SelState;   // the head of the workspace (prune_select.h)

template <typename K> __device__ inline K key_mask() { return (K)(~(K)0 >> 1); }

__global__ void __launch_bounds__(256) escoin_prune_init_kernel(SelState *st, unsigned *hist, int hist_words,
                                                                 unsigned long long prefix, unsigned long long remaining,
                                                                 unsigned ge) {
  for (int i = threadIdx.x; i < hist_words; i += 256) hist[i] = 0u;
  if (threadIdx.x == 0) {
    st->prefix = prefix;
    st->remaining = remaining;
    st->ge = ge;
    st->pad = 0u;
    st->total_gt = st->total_eq = 0ull;
  }
}

template <typename K>
__global__ void __launch_bounds__(256) escoin_prune_hist_kernel(const K *__restrict__ keys, long n, int pass, int passes,
                                                                 const SelState *__restrict__ st, unsigned *hist) {
  __shared__ unsigned bins[256];
  bins[threadIdx.x] = 0u;
  __syncthreads();
  const int shift = 8 * (passes - 1 - pass);
  const K prefix = (K)st->prefix;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
    const K k = keys[e] & key_mask<K>();
    if (pass == 0 || (k >> (shift + 8)) == prefix) atomicAdd(&bins[(unsigned)(k >> shift) & 0xffu], 1u);
  }
  __syncthreads();
  const unsigned c = bins[threadIdx.x];
  if (c) atomicAdd(&hist[threadIdx.x], c);
}

__global__ void __launch_bounds__(64) escoin_prune_choose_kernel(SelState *st, const unsigned *__restrict__ hist) {
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
  // (the host launches the select only for 0 < keep < nnz, where the matching keys number at least `remaining`: a digit
  //  is always found; were it not, digit 0 and a clamped count keep the later kernels' arithmetic in range)
  st->remaining = remaining > above ? remaining - above : 0ull;
  st->prefix = (st->prefix << 8) | (unsigned long long)digit;
}

// the two flags of entry e under the state's rule: bit 0 kept strictly, bit 1 a tie
template <typename K>
__device__ inline unsigned entry_flags(const K *__restrict__ keys, long e, long n, K T, unsigned ge) {
  if (e >= n) return 0u;
  const K k = keys[e] & key_mask<K>();
  if (ge) return k >= T ? 1u : 0u;
  return (k > T ? 1u : 0u) | (k == T ? 2u : 0u);
}

template <typename K>
__global__ void __launch_bounds__(256) escoin_prune_count_kernel(const K *__restrict__ keys, long n, long tiles,
                                                                  const SelState *__restrict__ st, unsigned *tile_cnt) {
  __shared__ unsigned cnt[2];
  const K T = (K)st->prefix;
  const unsigned ge = st->ge;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0u;
    __syncthreads();
    unsigned gt = 0, eq = 0;
    for (int i = 0; i < kItems; ++i) {
      const unsigned f = entry_flags<K>(keys, tile * kTileEntries + i * kThreads + threadIdx.x, n, T, ge);
      gt += __popcll(__ballot(f & 1u));
      eq += __popcll(__ballot(f & 2u));
    }
    if ((threadIdx.x & 63) == 0) {
      atomicAdd(&cnt[0], gt);
      atomicAdd(&cnt[1], eq);
    }
    __syncthreads();
    if (threadIdx.x < 2) tile_cnt[tile * 2 + threadIdx.x] = cnt[threadIdx.x];
    __syncthreads();
  }
}

// In place: tile_cnt[2 t + {0, 1}] becomes the number of strictly-kept / tied entries in the tiles before t.
__global__ void __launch_bounds__(256) escoin_prune_scan_kernel(long tiles, SelState *st, unsigned *tile_cnt) {
  __shared__ unsigned wsum[4][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long carry0 = 0, carry1 = 0;
  for (long base = 0; base < tiles; base += 256) {
    const long t = base + threadIdx.x;
    const unsigned c0 = t < tiles ? tile_cnt[t * 2] : 0u, c1 = t < tiles ? tile_cnt[t * 2 + 1] : 0u;
    unsigned s0 = c0, s1 = c1;   // inclusive scan inside the wave
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned u0 = __shfl_up(s0, d, 64), u1 = __shfl_up(s1, d, 64);
      if (lane >= d) s0 += u0, s1 += u1;
    }
    if (lane == 63) wsum[wave][0] = s0, wsum[wave][1] = s1;
    __syncthreads();
    unsigned before0 = 0, before1 = 0, all0 = 0, all1 = 0;
    for (int w = 0; w < 4; ++w) {
      if (w < wave) before0 += wsum[w][0], before1 += wsum[w][1];
      all0 += wsum[w][0], all1 += wsum[w][1];
    }
    if (t < tiles) {
      tile_cnt[t * 2] = (unsigned)(carry0 + before0 + s0 - c0);
      tile_cnt[t * 2 + 1] = (unsigned)(carry1 + before1 + s1 - c1);
    }
    carry0 += all0, carry1 += all1;
    __syncthreads();   // wsum is rewritten by the next step
  }
  if (threadIdx.x == 0) st->total_gt = carry0, st->total_eq = carry1;
}

template <typename K>
__global__ void __launch_bounds__(256) escoin_prune_apply_kernel(const K *__restrict__ keys, long n, long tiles,
                                                                  const SelState *__restrict__ st,
                                                                  const unsigned *__restrict__ tile_off, int *entry_map) {
  __shared__ unsigned wsum[kItems][4][2];
  const K T = (K)st->prefix;
  const unsigned ge = st->ge;
  const unsigned long long ties = st->remaining;
  const int wave = threadIdx.x >> 6;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    unsigned f[kItems], in0[kItems], in1[kItems];   // flags; strictly-kept / tied entries before this lane in its wave
    for (int i = 0; i < kItems; ++i) {
      f[i] = entry_flags<K>(keys, tile * kTileEntries + i * kThreads + threadIdx.x, n, T, ge);
      const unsigned long long b0 = __ballot(f[i] & 1u), b1 = __ballot(f[i] & 2u);
      in0[i] = __builtin_amdgcn_mbcnt_hi((unsigned)(b0 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b0, 0u));
      in1[i] = __builtin_amdgcn_mbcnt_hi((unsigned)(b1 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b1, 0u));
      if ((threadIdx.x & 63) == 0) wsum[i][wave][0] = __popcll(b0), wsum[i][wave][1] = __popcll(b1);
    }
    __syncthreads();
    // a tile's order is item-major: entry (i, lane) follows every entry of items < i and of earlier waves of item i
    unsigned long long run0 = tile_off[tile * 2], run1 = tile_off[tile * 2 + 1];
    for (int i = 0; i < kItems; ++i) {
      unsigned before0 = 0, before1 = 0, all0 = 0, all1 = 0;
      for (int w = 0; w < 4; ++w) {
        if (w < wave) before0 += wsum[i][w][0], before1 += wsum[i][w][1];
        all0 += wsum[i][w][0], all1 += wsum[i][w][1];
      }
      const long e = tile * kTileEntries + i * kThreads + threadIdx.x;
      if (e < n) {
        const unsigned long long r0 = run0 + before0 + in0[i], r1 = run1 + before1 + in1[i];
        const bool kept = (f[i] & 1u) || ((f[i] & 2u) && r1 < ties);
        entry_map[e] = kept ? (int)(r0 + (r1 < ties ? r1 : ties)) : -1;
      }
      run0 += all0, run1 += all1;
    }
    __syncthreads();   // wsum is rewritten by the next tile
  }
}

template <typename W>
__global__ void __launch_bounds__(256) escoin_compact_kernel(const int *__restrict__ entry_map, long n,
                                                              const W *__restrict__ src, W *__restrict__ dst) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int to = entry_map[e];
  if (to >= 0) dst[to] = src[e];
}

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

namespace prune {

// What every entry point checks of the descriptor; thr_key: key(threshold) in the plan's Dtype.
template <typename T>
int check_desc(const escoin_prune_desc *d, typename KeyOf<T>::type *thr_key) {
  if (!d) return fail(ESCOIN_EINVAL, "prune: null descriptor");
  if (d->mode != ESCOIN_PRUNE_KEEP && d->mode != ESCOIN_PRUNE_THRESHOLD) return fail(ESCOIN_EINVAL, "prune: unknown mode");
  if (d->mode == ESCOIN_PRUNE_KEEP && d->keep < 0) return fail(ESCOIN_EINVAL, "prune: keep must be >= 0");
  *thr_key = 0;
  if (d->mode == ESCOIN_PRUNE_THRESHOLD) {
    if (std::isnan(d->threshold) || std::signbit(d->threshold)) return fail(ESCOIN_EINVAL, "prune: threshold must be >= 0 and not NaN");
    *thr_key = key_bits((T)d->threshold);
  }
  return ESCOIN_OK;
}
template int check_desc<float>(const escoin_prune_desc *, uint32_t *);
template int check_desc<double>(const escoin_prune_desc *, uint64_t *);

void launch_select_init(SelState *st, unsigned *hist, int hist_words, unsigned long long prefix, unsigned long long remaining,
                        unsigned ge, hipStream_t stream) {
  hipLaunchKernelGGL(escoin_prune_init_kernel, dim3(1), dim3(kThreads), 0, stream, st, hist, hist_words, prefix, remaining, ge);
}

void launch_select_choose(SelState *st, const unsigned *hist, hipStream_t stream) {
  hipLaunchKernelGGL(escoin_prune_choose_kernel, dim3(1), dim3(64), 0, stream, st, hist);
}

template <typename K>
int launch_selection(const K *keys, long nnz, const LaunchPlan &lp, const escoin_prune_desc *d, K thr_key, void *ws,
                     int *entry_map_dev, hipStream_t stream) {
  SelState *st = static_cast<SelState *>(ws);
  unsigned *hist = reinterpret_cast<unsigned *>(static_cast<char *>(ws) + kStateBytes);
  unsigned *tile_cnt = hist + (size_t)lp.passes * 256;
  const bool select = d->mode == ESCOIN_PRUNE_KEEP && d->keep > 0 && d->keep < nnz;
  Boundary<K> b{0, 0, 1};                                  // keep >= nnz: everything stays
  if (d->mode == ESCOIN_PRUNE_THRESHOLD) b = select_threshold<K>(thr_key);
  else if (d->keep == 0) b = Boundary<K>{std::numeric_limits<K>::max(), 0, 0};
  const dim3 block(kThreads);
  launch_select_init(st, hist, lp.passes * 256, (unsigned long long)(select ? 0 : b.T), (unsigned long long)(select ? d->keep : 0),
                     (unsigned)(select ? 0 : b.ge), stream);
  if (select) {
    for (int pass = 0; pass < lp.passes; ++pass) {
      hipLaunchKernelGGL((escoin_prune_hist_kernel<K>), dim3(lp.hist_grid), block, 0, stream, keys, nnz, pass, lp.passes,
                         (const SelState *)st, hist + (size_t)pass * 256);
      launch_select_choose(st, hist + (size_t)pass * 256, stream);
    }
  }
  hipLaunchKernelGGL((escoin_prune_count_kernel<K>), dim3(lp.tile_grid), block, 0, stream, keys, nnz, lp.tiles, (const SelState *)st, tile_cnt);
  hipLaunchKernelGGL(escoin_prune_scan_kernel, dim3(1), block, 0, stream, lp.tiles, st, tile_cnt);
  hipLaunchKernelGGL((escoin_prune_apply_kernel<K>), dim3(lp.tile_grid), block, 0, stream, keys, nnz, lp.tiles, (const SelState *)st,
                     (const unsigned *)tile_cnt, entry_map_dev);
  ESCOIN_HIP_TRY(hipGetLastError());
  return ESCOIN_OK;
}
template int launch_selection<uint32_t>(const uint32_t *, long, const LaunchPlan &, const escoin_prune_desc *, uint32_t, void *, int *, hipStream_t);
template int launch_selection<uint64_t>(const uint64_t *, long, const LaunchPlan &, const escoin_prune_desc *, uint64_t, void *, int *, hipStream_t);

template <typename T>
long host_entry_map(escoin_plan *p, const escoin_prune_desc *d, typename KeyOf<T>::type thr_key, int *map) {
  typedef typename KeyOf<T>::type K;
  const long nnz = plan_nnz(p);
  std::vector<T> flat;
  const T *score = static_cast<const T *>(d->score);
  if (!score) {
    flat = flat_entries(plan_vals<T>(p));
    score = flat.data();
  }
  const std::vector<K> keys = keys_of<T>(score, nnz);
  const Boundary<K> b = d->mode == ESCOIN_PRUNE_KEEP ? select_keep<K>(keys.data(), nnz, d->keep) : select_threshold<K>(thr_key);
  return build_map<K>(keys.data(), nnz, b, map);
}
template long host_entry_map<float>(escoin_plan *, const escoin_prune_desc *, uint32_t, int *);
template long host_entry_map<double>(escoin_plan *, const escoin_prune_desc *, uint64_t, int *);

}  // namespace prune

namespace {

using prune::check_desc;

// The plan re-aligned on the kept entries of `map` (host, old nnz elements): a new host CSR through set_csr's own checks,
// then -- for a device-aligned plan -- the device side rebuilt from it, as escoin_plan_set_csr does.
template <typename T>
int realign_kept(escoin_plan *p, const int *map, long old_nnz, bool device, hipStream_t stream) {
  const auto t0 = std::chrono::steady_clock::now();
  prune::FlatCsr<T> csr;
  if (!prune::apply_entry_map<T>(p->g.Mg, p->rowptr, p->colidx, plan_vals<T>(p), map, old_nnz, &csr))
    return fail(ESCOIN_EINVAL, "prune: the entry map does not match the plan's CSR");
  const int rc = set_csr_host<T>(p, csr.rowptr.data(), csr.colidx.data(), csr.values.data(), csr.nnz_per_group.data());
  if (rc != ESCOIN_OK) return rc;
  const double ms_csr = ms_since(t0);
  const int rc2 = device ? realign_from_host_csr(p, stream) : ESCOIN_OK;
  if (getenv("ESCOIN_VERBOSE"))
    fprintf(stderr, "[escoin] prune: %ld -> %zu entries: new host CSR %.2f ms, device side rebuilt in %.2f ms\n", old_nnz,
            csr.colidx.size(), ms_csr, ms_since(t0) - ms_csr);
  return rc2;
}

template <typename T>
int prune_device(escoin_plan *p, const escoin_prune_desc *d, int *entry_map_dev, long *new_nnz, hipStream_t stream) {
  typedef typename prune::KeyOf<T>::type K;
  const auto t_start = std::chrono::steady_clock::now();
  K thr_key = 0;
  if (const int rc = check_desc<T>(d, &thr_key)) return rc;
  const long nnz = plan_nnz(p);
  if (nnz > 0) {
    // the values a device-source update or solver step left are ranked where they are: behind that update's stream
    if (p->dev_authoritative && p->upd_stream != stream) ESCOIN_HIP_TRY(hipStreamSynchronize(p->upd_stream));
    if (p->gen.vals.bytes() < sizeof(T) * (size_t)nnz) return fail(ESCOIN_EINVAL, "prune: the plan's value array is shorter than its CSR");
  }
  std::vector<int> map((size_t)nnz);
  p->prune_kernels_ms = 0.0;
  if (nnz > 0) {
    const K *keys = d->score ? static_cast<const K *>(d->score) : p->gen.vals.get<const K>();
    const prune::LaunchPlan lp = prune::launch_plan(nnz, (int)sizeof(T));
    DeviceBuffer ws, own_map;
    ESCOIN_HIP_TRY(ws.alloc(lp.ws_bytes));
    if (!entry_map_dev) {
      ESCOIN_HIP_TRY(own_map.alloc(sizeof(int) * (size_t)nnz));
      entry_map_dev = own_map.get<int>();
    }
    // (events around the launches: stat "prune_kernels_us"; this call synchronises and allocates anyway)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    ESCOIN_HIP_TRY(hipEventCreate(&ev0));
    if (hipEventCreate(&ev1) != hipSuccess) {
      (void)hipEventDestroy(ev0);
      return fail(ESCOIN_EHIP, "prune: hipEventCreate failed");
    }
    struct EventGuard {
      hipEvent_t a, b;
      ~EventGuard() { (void)hipEventDestroy(a), (void)hipEventDestroy(b); }
    } guard{ev0, ev1};
    ESCOIN_HIP_TRY(hipEventRecord(ev0, stream));
    if (const int rc = prune::launch_selection<K>(keys, nnz, lp, d, thr_key, ws.get<void>(), entry_map_dev, stream)) return rc;
    ESCOIN_HIP_TRY(hipEventRecord(ev1, stream));
    // the plan is about to re-align, which synchronises anyway: the map comes to the host here
    ESCOIN_HIP_TRY(hipMemcpyAsync(map.data(), entry_map_dev, sizeof(int) * (size_t)nnz, hipMemcpyDeviceToHost, stream));
    ESCOIN_HIP_TRY(hipStreamSynchronize(stream));
    float kernels_ms = 0.f;
    ESCOIN_HIP_TRY(hipEventElapsedTime(&kernels_ms, ev0, ev1));
    p->prune_kernels_ms = kernels_ms;
  }
  p->prune_map_ms = ms_since(t_start);
  long kept = 0;
  for (long e = 0; e < nnz; ++e) kept += map[(size_t)e] >= 0 ? 1 : 0;
  ++p->prune_count;
  p->prune_last_dropped = nnz - kept;
  if (new_nnz) *new_nnz = kept;
  p->prune_realign_ms = 0.0;
  if (kept == nnz) return ESCOIN_OK;           // nothing dropped: the plan, its backward and update states stay
  if (const int rc = sync_host_values(p)) return rc;
  if (getenv("ESCOIN_VERBOSE"))
    fprintf(stderr, "[escoin] prune: map on the host after %.2f ms, values read back after %.2f ms\n", p->prune_map_ms, ms_since(t_start));
  const int rc = realign_kept<T>(p, map.data(), nnz, true, stream);
  p->align_ms = ms_since(t_start);
  p->prune_realign_ms = p->align_ms - p->prune_map_ms;
  return rc;
}

template <typename T>
int prune_host(escoin_plan *p, const escoin_prune_desc *d, int *entry_map, long *new_nnz) {
  typedef typename prune::KeyOf<T>::type K;
  const auto t_start = std::chrono::steady_clock::now();
  K thr_key = 0;
  if (const int rc = check_desc<T>(d, &thr_key)) return rc;
  const long nnz = plan_nnz(p);
  std::vector<int> own_map;
  if (!entry_map) {
    own_map.resize((size_t)nnz);
    entry_map = own_map.data();
  }
  const long kept = prune::host_entry_map<T>(p, d, thr_key, entry_map);
  ++p->prune_count;
  p->prune_last_dropped = nnz - kept;
  if (new_nnz) *new_nnz = kept;
  if (kept == nnz) return ESCOIN_OK;
  const int rc = realign_kept<T>(p, entry_map, nnz, false, nullptr);
  p->align_ms = ms_since(t_start);
  return rc;
}

}  // namespace
}  // namespace escoin

using namespace escoin;

extern "C" {

int escoin_plan_prune(escoin_plan *p, const escoin_prune_desc *desc, int *entry_map_dev, long *new_nnz, void *stream) {
  return guarded([&]() -> int {
    if (!p) return fail(ESCOIN_EINVAL, "prune: null plan");
    if (!desc) return fail(ESCOIN_EINVAL, "prune: null descriptor");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
      return fail(ESCOIN_ENODEVICE, "prune: no HIP device (a plan aligned by escoin_weight_align_cpu is pruned by escoin_plan_prune_cpu)");
    if (!p->aligned)
      return fail(ESCOIN_ESTATE, p->host_aligned ? "prune: the plan is aligned on the host only (use escoin_plan_prune_cpu)"
                                                 : "prune called before weight_align / set_csr");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != p->device)
      return fail(ESCOIN_ESTATE, "prune: the current device is not the device the plan was aligned on");
    return p->is_f64 ? prune_device<double>(p, desc, entry_map_dev, new_nnz, (hipStream_t)stream)
                     : prune_device<float>(p, desc, entry_map_dev, new_nnz, (hipStream_t)stream);
  });
}

int escoin_plan_prune_cpu(escoin_plan *p, const escoin_prune_desc *desc, int *entry_map, long *new_nnz) {
  return guarded([&]() -> int {
    if (!p) return fail(ESCOIN_EINVAL, "prune_cpu: null plan");
    if (!desc) return fail(ESCOIN_EINVAL, "prune: null descriptor");
    if (!p->host_aligned) return fail(ESCOIN_ESTATE, "prune_cpu called before weight_align_cpu");
    if (p->aligned)
      return fail(ESCOIN_ESTATE, "prune_cpu: the plan has a device side, which this entry point would leave behind; escoin_plan_prune prunes both sides");
    return p->is_f64 ? prune_host<double>(p, desc, entry_map, new_nnz) : prune_host<float>(p, desc, entry_map, new_nnz);
  });
}

int escoin_compact_entries(const int *entry_map, long old_nnz, int elem_bytes, const void *src, void *dst, int on_device,
                           void *stream) {
  if (elem_bytes != 4 && elem_bytes != 8) return fail(ESCOIN_EINVAL, "compact_entries: elem_bytes must be 4 or 8");
  if (old_nnz < 0) return fail(ESCOIN_EINVAL, "compact_entries: old_nnz must be >= 0");
  if (old_nnz > 0 && (!entry_map || !src || !dst)) return fail(ESCOIN_EINVAL, "compact_entries: null argument");
  if (old_nnz > 0 && src == dst) return fail(ESCOIN_EINVAL, "compact_entries: src and dst must not overlap");
  if (!on_device) {
    // a plain host loop, no HIP call
    if (elem_bytes == 4) {
      const uint32_t *s = static_cast<const uint32_t *>(src);
      uint32_t *t = static_cast<uint32_t *>(dst);
      for (long e = 0; e < old_nnz; ++e)
        if (entry_map[e] >= 0) t[entry_map[e]] = s[e];
    } else {
      const uint64_t *s = static_cast<const uint64_t *>(src);
      uint64_t *t = static_cast<uint64_t *>(dst);
      for (long e = 0; e < old_nnz; ++e)
        if (entry_map[e] >= 0) t[entry_map[e]] = s[e];
    }
    return ESCOIN_OK;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(ESCOIN_ENODEVICE, "compact_entries: no HIP device");
  if (old_nnz == 0) return ESCOIN_OK;
  const dim3 grid((unsigned)((old_nnz + 255) / 256)), block(256);
  if (elem_bytes == 4)
    hipLaunchKernelGGL((escoin_compact_kernel<uint32_t>), grid, block, 0, (hipStream_t)stream, entry_map, old_nnz,
                       static_cast<const uint32_t *>(src), static_cast<uint32_t *>(dst));
  else
    hipLaunchKernelGGL((escoin_compact_kernel<uint64_t>), grid, block, 0, (hipStream_t)stream, entry_map, old_nnz,
                       static_cast<const uint64_t *>(src), static_cast<uint64_t *>(dst));
  ESCOIN_HIP_TRY(hipGetLastError());
  return ESCOIN_OK;
}

}  // extern "C"
