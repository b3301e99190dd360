// prune_select.hip -- magnitude pruning of an aligned plan on the device (include/escoin.h, "Pruning"): the source and
// the apply kernel of the selection, the entry map, escoin_compact_entries, and the entry points that re-align the plan on
// the kept entries.
//
// The rule is prune_rules.h's: key(s) = the bits of s without the sign bit, an unsigned integer; KEEP keeps the first
// min(keep, nnz) entries by (key descending, entry index ascending), THRESHOLD the entries with key >= key(threshold).
// Every comparison below is an integer comparison.
//
// The select, count and scan kernels and the rank arithmetic are radix_select.h's, over KeySource with two counts per
// tile; the contract that keeps these kernels from hanging a machine is written there and holds for the two kernels here:
//   escoin_prune_apply_kernel     per tile: tile_ranks -> entry_map[e] = kept-strictly before e + min(ties before e,
//                                 ties that fit), or -1
//   escoin_compact_kernel         dst[entry_map[e]] = src[e], one lane per old entry, one plain store; its grid is
//                                 ceil(nnz / 256)
// THRESHOLD mode and the trivial KEEP cases skip the select.  The launch sequence, the descriptor check, the host form of
// the map and the host orchestration are shared with rewire_select.hip (prune_select.h).
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
#include "radix_select.h"

namespace escoin {
namespace {

// The entries' keys; every entry is a candidate.  Flags: bit 0 kept strictly, bit 1 a tie.
template <typename K>
struct KeySource {
  const K *__restrict__ keys;
  __device__ bool candidate(long) const { return true; }
  __device__ K key(long e) const { return keys[e] & key_mask<K>(); }
  __device__ unsigned flags(long e, K T, unsigned ge) const {
    const K k = key(e);
    if (ge) return k >= T ? 1u : 0u;
    return (k > T ? 1u : 0u) | (k == T ? 2u : 0u);
  }
};

template <typename K>
__global__ void __launch_bounds__(256) escoin_prune_apply_kernel(const KeySource<K> src, long n, long tiles,
                                                                  const SelState *__restrict__ st,
                                                                  const unsigned *__restrict__ tile_off, int *entry_map) {
  const K T = (K)st->prefix;
  const unsigned ge = st->ge;
  const unsigned long long ties = st->remaining;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x)
    tile_ranks<2>(src, n, tile, T, ge, tile_off, [=](long e, unsigned f, const unsigned long long (&r)[2]) {
      const bool kept = (f & 1u) || ((f & 2u) && r[1] < ties);
      entry_map[e] = kept ? (int)(r[0] + (r[1] < ties ? r[1] : ties)) : -1;
    });
}

template <typename W>
__global__ void __launch_bounds__(256) escoin_compact_kernel(const int *__restrict__ entry_map, long n,
                                                              const W *__restrict__ src, W *__restrict__ dst) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int to = entry_map[e];
  if (to >= 0) dst[to] = src[e];
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

template <typename K>
int launch_selection(const K *keys, long nnz, const LaunchPlan &lp, const escoin_prune_desc *d, K thr_key, void *ws,
                     int *entry_map_dev, hipStream_t stream) {
  const SelectWorkspace w(ws, lp);
  const KeySource<K> src{keys};
  const bool select = d->mode == ESCOIN_PRUNE_KEEP && d->keep > 0 && d->keep < nnz;
  Boundary<K> b{0, 0, 1};                                  // keep >= nnz: everything stays
  if (d->mode == ESCOIN_PRUNE_THRESHOLD) b = select_threshold<K>(thr_key);
  else if (d->keep == 0) b = Boundary<K>{std::numeric_limits<K>::max(), 0, 0};
  launch_select<2>(src, nnz, lp, w, b, select ? d->keep : 0, stream);
  hipLaunchKernelGGL((escoin_prune_apply_kernel<K>), dim3(lp.tile_grid), dim3(kThreads), 0, stream, src, nnz, lp.tiles,
                     (const SelState *)w.st, (const unsigned *)w.tile_cnt, entry_map_dev);
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

int check_device_plan(const escoin_plan *p, const char *name) {
  const std::string n(name);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail(ESCOIN_ENODEVICE, n + ": no HIP device (a plan aligned by escoin_weight_align_cpu is " + n + "d by escoin_plan_" + n + "_cpu)");
  if (!p->aligned)
    return fail(ESCOIN_ESTATE, p->host_aligned ? n + ": the plan is aligned on the host only (use escoin_plan_" + n + "_cpu)"
                                               : n + " called before weight_align / set_csr");
  return check_plan_device(p, n);
}

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
  return prune::realign_on<T>(p, csr, device, stream, t0,
                              "prune: " + std::to_string(old_nnz) + " -> " + std::to_string(csr.colidx.size()) + " entries");
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
    prune::EventTimer timer;   // stat "prune_kernels_us"
    if (const int rc = timer.start("prune", stream)) return rc;
    if (const int rc = prune::launch_selection<K>(keys, nnz, lp, d, thr_key, ws.get<void>(), entry_map_dev, stream)) return rc;
    if (const int rc = timer.stop(stream)) return rc;
    // the plan is about to re-align, which synchronises anyway: the map comes to the host here
    ESCOIN_HIP_TRY(hipMemcpyAsync(map.data(), entry_map_dev, sizeof(int) * (size_t)nnz, hipMemcpyDeviceToHost, stream));
    ESCOIN_HIP_TRY(hipStreamSynchronize(stream));
    if (const int rc = timer.elapsed_ms(&p->prune_kernels_ms)) return rc;
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
    if (const int rc = refuse_deconv(p, "escoin_plan_prune")) return rc;
    if (const int rc = prune::check_device_plan(p, "prune")) return rc;
    return p->is_f64 ? prune_device<double>(p, desc, entry_map_dev, new_nnz, (hipStream_t)stream)
                     : prune_device<float>(p, desc, entry_map_dev, new_nnz, (hipStream_t)stream);
  });
}

int escoin_plan_prune_cpu(escoin_plan *p, const escoin_prune_desc *desc, int *entry_map, long *new_nnz) {
  return guarded([&]() -> int {
    if (!p) return fail(ESCOIN_EINVAL, "prune_cpu: null plan");
    if (!desc) return fail(ESCOIN_EINVAL, "prune: null descriptor");
    if (const int rc = refuse_deconv(p, "escoin_plan_prune_cpu")) return rc;
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
  if (old_nnz > 0 && (!entry_map || !src)) return fail(ESCOIN_EINVAL, "compact_entries: null argument");
  if (old_nnz > 0 && !dst) {
    // a NULL dst is a destination of 0 elements (the new nnz is 0; an empty tensor's pointer): nothing is stored, nothing
    // launched.  The host route can see a map that keeps an entry all the same, and refuses it.
    if (!on_device)
      for (long e = 0; e < old_nnz; ++e)
        if (entry_map[e] >= 0) return fail(ESCOIN_EINVAL, "compact_entries: the map keeps an entry but dst is NULL");
    return ESCOIN_OK;
  }
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
