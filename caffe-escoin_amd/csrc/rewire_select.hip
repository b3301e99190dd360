// rewire_select.hip -- drop-and-grow rewiring of an aligned plan on the device (include/escoin.h, "Rewiring"): the
// kernels over the D = M * kdim dense positions, and the entry points that re-align the plan ONCE on kept + grown.
//
// The rule is rewire_rules.h's.  The drop is escoin_plan_prune's selection over the plan's entries, by its own launch
// sequence (prune_select.h launch_selection).  The grow ranks the positions outside the pattern by (key(score[p])
// descending, p ascending) and takes the first n_grown.  Every comparison below is an integer comparison.  What tells a
// candidate from a position of the pattern is slot[p], an int per position built from the host CSR's entry positions --
// never a value of the key itself, so a zero score (key 0) and a NaN with every mantissa bit set (the largest key) are
// ordinary candidates.
//
// The select, count and scan kernels and the rank arithmetic are radix_select.h's, over SlotSource with kCounts counts per
// tile; the contract that keeps these kernels from hanging a machine is written there and holds for the two kernels here,
// whose loops are bounded by D or nnz.  Every store is bounds-checked against the length of the array it goes to.
//
//   (hipMemsetAsync)              slot[p] = -1 for every position: a candidate
//   escoin_rewire_mark_kernel     per entry e at position pos[e]: slot = e if the drop keeps it, -2 if not (and then
//                                 entry_map[e] = -1)
//   (launch_select)               the boundary key T among the candidates; per tile of 1024 positions the kept entries,
//                                 the candidates above T and the ties, scanned over the tiles
//   escoin_rewire_apply_kernel    per tile: tile_ranks gives every flagged position its new entry index = kept before +
//                                 grown before.  <0>: entry_map through slot[p]; <1>: grown, the grown positions and the
//                                 grown values
// No host round trip between them; the trivial grow counts (0, every candidate) skip the select.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "escoin_plan.h"
#include "prune_rules.h"
#include "prune_select.h"
#include "radix_select.h"
#include "rewire_rules.h"

namespace escoin {
namespace {

using rewire::kCounts;
using rewire::kSlotCandidate;
using rewire::kSlotDropped;

__global__ void __launch_bounds__(256) escoin_rewire_mark_kernel(const int *__restrict__ pos, const int *__restrict__ drop_map,
                                                                  long nnz, long D, int *slot, int *entry_map) {
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < nnz; e += (long)gridDim.x * 256) {
    const bool kept = !drop_map || drop_map[e] >= 0;
    const long p = pos[e];
    if (p >= 0 && p < D) slot[p] = kept ? (int)e : kSlotDropped;
    if (!kept) entry_map[e] = -1;
  }
}

// The D positions; the candidates are those slot[p] marks as outside the pattern.  Flags: bit 0 a kept entry, bit 1 a
// candidate grown strictly, bit 2 a candidate that ties; score == NULL (nothing is grown): no candidate is flagged and no
// score is read.
template <typename K>
struct SlotSource {
  const K *__restrict__ score;
  const int *__restrict__ slot;
  __device__ bool candidate(long p) const { return slot[p] == kSlotCandidate; }
  __device__ K key(long p) const { return score[p] & key_mask<K>(); }
  __device__ unsigned flags(long p, K T, unsigned ge) const {
    const int s = slot[p];
    if (s >= 0) return 1u;
    if (s != kSlotCandidate || !score) return 0u;
    const K k = key(p);
    if (ge) return k >= T ? 2u : 0u;
    return (k > T ? 2u : 0u) | (k == T ? 4u : 0u);
  }
};

// WHAT == 0: entry_map[slot[p]] = the new index of every kept entry.  WHAT == 1: for the i-th grown position (ascending):
// grown[i] = its new index, grown_pos[i] = p, grown_val[i] = the bits of init[p], or +0.0.
template <typename K, int WHAT>
__global__ void __launch_bounds__(256) escoin_rewire_apply_kernel(const SlotSource<K> src, long D, long tiles,
                                                                   const SelState *__restrict__ st,
                                                                   const unsigned *__restrict__ tile_off, long nnz, int *entry_map,
                                                                   long n_grown, int *grown, int *grown_pos, K *grown_val,
                                                                   const K *__restrict__ init) {
  const K T = (K)st->prefix;
  const unsigned ge = st->ge;
  const unsigned long long ties = st->remaining;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x)
    tile_ranks<kCounts>(src, D, tile, T, ge, tile_off, [=](long p, unsigned f, const unsigned long long (&r)[kCounts]) {
      const unsigned long long grown_before = r[1] + (r[2] < ties ? r[2] : ties);
      const unsigned long long index = r[0] + grown_before;
      if (WHAT == 0) {
        if (f & 1u) {
          const long e = src.slot[p];
          if (e >= 0 && e < nnz) entry_map[e] = (int)index;
        }
      } else {
        const bool is_grown = (f & 2u) || ((f & 4u) && r[2] < ties);
        if (is_grown && grown_before < (unsigned long long)n_grown) {
          grown[grown_before] = (int)index;
          grown_pos[grown_before] = (int)p;
          grown_val[grown_before] = init ? init[p] : (K)0;
        }
      }
    });
}

// What both entry points check of the descriptor beyond the plan's state.
template <typename T>
int check_rewire(const escoin_plan *p, const escoin_rewire_desc *d, typename prune::KeyOf<T>::type *thr_key, long *D) {
  *thr_key = 0;
  if (d->drop)
    if (const int rc = prune::check_desc<T>(d->drop, thr_key)) return rc;
  *D = (long)p->g.d.M * p->g.kdim;
  return ESCOIN_OK;
}

// The plan re-aligned on the kept entries of `keep_map` and the grown positions: one new host CSR through set_csr's own
// checks, then -- for a device-aligned plan -- the device side rebuilt from it, as escoin_plan_set_csr does.  entry_map /
// grown: the merge's outputs (host), either may be NULL.  expect_map: NULL, or the device's entry map -- the host's merge is
// the rule's restatement, so a device map that differs is refused before the plan is touched.
template <typename T>
int realign_rewired(escoin_plan *p, const int *keep_map, const std::vector<int> &grown_pos, const T *grown_val, int *entry_map,
                    int *grown, const int *expect_map, bool device, hipStream_t stream) {
  const auto t0 = std::chrono::steady_clock::now();
  prune::FlatCsr<T> csr;
  if (!rewire::merge<T>(p->g.Mg, p->g.kdim, p->rowptr, p->colidx, plan_vals<T>(p), keep_map, grown_pos.data(), grown_val,
                        (long)grown_pos.size(), &csr, entry_map, grown))
    return fail(ESCOIN_EINVAL, "rewire: the grown positions do not fit the plan's CSR");
  if (expect_map && entry_map && std::memcmp(expect_map, entry_map, sizeof(int) * (size_t)plan_nnz(p)) != 0)
    return fail(ESCOIN_EINVAL, "rewire: the device's entry map is not the merged CSR's");
  return prune::realign_on<T>(p, csr, device, stream, t0,
                              "rewire: " + std::to_string(csr.colidx.size()) + " entries, " + std::to_string(grown_pos.size()) + " of them grown");
}

void note_stats(escoin_plan *p, long dropped, long grown) {
  ++p->rewire_count;
  p->rewire_last_dropped = dropped;
  p->rewire_last_grown = grown;
}

template <typename T>
int rewire_device(escoin_plan *p, const escoin_rewire_desc *d, int *entry_map_dev, int *grown_dev, long *new_nnz, long *n_grown_out,
                  hipStream_t stream) {
  typedef typename prune::KeyOf<T>::type K;
  const auto t_start = std::chrono::steady_clock::now();
  K thr_key = 0;
  long D = 0;
  if (const int rc = check_rewire<T>(p, d, &thr_key, &D)) return rc;
  const long nnz = plan_nnz(p), n_cand = D - nnz, n_grown = d->grow < n_cand ? d->grow : n_cand;
  p->rewire_kernels_ms = p->rewire_realign_ms = 0.0;
  std::vector<int> map((size_t)nnz), gpos((size_t)n_grown);
  std::vector<T> gval((size_t)n_grown);
  if (!d->drop && n_grown == 0) {
    // nothing can change: the identity map, no launch
    for (long e = 0; e < nnz; ++e) map[(size_t)e] = (int)e;
    if (entry_map_dev && nnz > 0) {
      ESCOIN_HIP_TRY(hipMemcpyAsync(entry_map_dev, map.data(), sizeof(int) * (size_t)nnz, hipMemcpyHostToDevice, stream));
      ESCOIN_HIP_TRY(hipStreamSynchronize(stream));
    }
  } else {
    if (nnz > 0 && d->drop) {
      // the values a device-source update or solver step left are ranked where they are: behind that update's stream
      if (p->dev_authoritative && p->upd_stream != stream) ESCOIN_HIP_TRY(hipStreamSynchronize(p->upd_stream));
      if (p->gen.vals.bytes() < sizeof(T) * (size_t)nnz) return fail(ESCOIN_EINVAL, "rewire: the plan's value array is shorter than its CSR");
    }
    const rewire::LaunchPlan lp = rewire::launch_plan(D, nnz, (int)sizeof(T));
    const std::vector<int> pos = rewire::entry_positions(p->g.Mg, p->g.kdim, p->rowptr, p->colidx);
    if ((long)pos.size() != nnz) return fail(ESCOIN_EINVAL, "rewire: the plan's CSR is inconsistent");
    DeviceBuffer ws, ws_drop, drop_map, pos_dev, slot, own_map, own_grown, gpos_dev, gval_dev;
    ESCOIN_HIP_TRY(ws.alloc(lp.ws_bytes));
    ESCOIN_HIP_TRY(slot.alloc(lp.slot_bytes));
    if (nnz > 0) {
      ESCOIN_HIP_TRY(pos_dev.upload(pos, stream));
      if (!entry_map_dev) {
        ESCOIN_HIP_TRY(own_map.alloc(sizeof(int) * (size_t)nnz));
        entry_map_dev = own_map.get<int>();
      }
    }
    if (n_grown > 0) {
      if (!grown_dev) {
        ESCOIN_HIP_TRY(own_grown.alloc(sizeof(int) * (size_t)n_grown));
        grown_dev = own_grown.get<int>();
      }
      ESCOIN_HIP_TRY(gpos_dev.alloc(sizeof(int) * (size_t)n_grown));
      ESCOIN_HIP_TRY(gval_dev.alloc(sizeof(T) * (size_t)n_grown));
    }
    const dim3 block(kThreads);
    prune::EventTimer timer;   // stat "rewire_kernels_us"
    if (const int rc = timer.start("rewire", stream)) return rc;
    if (nnz > 0 && d->drop) {
      const K *keys = d->drop->score ? static_cast<const K *>(d->drop->score) : p->gen.vals.get<const K>();
      const prune::LaunchPlan dlp = prune::launch_plan(nnz, (int)sizeof(T));
      ESCOIN_HIP_TRY(ws_drop.alloc(dlp.ws_bytes));
      ESCOIN_HIP_TRY(drop_map.alloc(sizeof(int) * (size_t)nnz));
      if (const int rc = prune::launch_selection<K>(keys, nnz, dlp, d->drop, thr_key, ws_drop.get<void>(), drop_map.get<int>(), stream)) return rc;
    }
    ESCOIN_HIP_TRY(hipMemsetAsync(slot.get<void>(), 0xff, lp.slot_bytes, stream));
    if (nnz > 0)
      hipLaunchKernelGGL(escoin_rewire_mark_kernel, dim3(lp.mark_grid), block, 0, stream, pos_dev.get<const int>(),
                         (const int *)drop_map.get<int>(), nnz, D, slot.get<int>(), entry_map_dev);
    const SelectWorkspace w(ws.get<void>(), lp);
    const SlotSource<K> src{n_grown > 0 ? static_cast<const K *>(d->score) : nullptr, slot.get<const int>()};
    // n_grown == n_cand: every candidate (key >= 0); n_grown == 0: none (no key exceeds or equals the largest K)
    const prune::Boundary<K> b = n_grown > 0 ? prune::Boundary<K>{0, 0, 1} : prune::Boundary<K>{std::numeric_limits<K>::max(), 0, 0};
    launch_select<kCounts>(src, D, lp, w, b, n_grown < n_cand ? n_grown : 0, stream);
    if (nnz > 0)
      hipLaunchKernelGGL((escoin_rewire_apply_kernel<K, 0>), dim3(lp.tile_grid), block, 0, stream, src, D, lp.tiles, (const SelState *)w.st,
                         (const unsigned *)w.tile_cnt, nnz, entry_map_dev, n_grown, (int *)nullptr, (int *)nullptr, (K *)nullptr,
                         (const K *)nullptr);
    if (n_grown > 0)
      hipLaunchKernelGGL((escoin_rewire_apply_kernel<K, 1>), dim3(lp.tile_grid), block, 0, stream, src, D, lp.tiles, (const SelState *)w.st,
                         (const unsigned *)w.tile_cnt, nnz, (int *)nullptr, n_grown, grown_dev, gpos_dev.get<int>(), gval_dev.get<K>(),
                         static_cast<const K *>(d->init));
    ESCOIN_HIP_TRY(hipGetLastError());
    if (const int rc = timer.stop(stream)) return rc;
    // the plan is about to re-align, which synchronises anyway: the map and the grown list come to the host here
    if (nnz > 0) ESCOIN_HIP_TRY(hipMemcpyAsync(map.data(), entry_map_dev, sizeof(int) * (size_t)nnz, hipMemcpyDeviceToHost, stream));
    if (n_grown > 0) {
      ESCOIN_HIP_TRY(hipMemcpyAsync(gpos.data(), gpos_dev.get<int>(), sizeof(int) * (size_t)n_grown, hipMemcpyDeviceToHost, stream));
      ESCOIN_HIP_TRY(hipMemcpyAsync(gval.data(), gval_dev.get<T>(), sizeof(T) * (size_t)n_grown, hipMemcpyDeviceToHost, stream));
    }
    ESCOIN_HIP_TRY(hipStreamSynchronize(stream));
    if (const int rc = timer.elapsed_ms(&p->rewire_kernels_ms)) return rc;
  }
  p->rewire_map_ms = ms_since(t_start);
  long kept = 0;
  for (long e = 0; e < nnz; ++e) kept += map[(size_t)e] >= 0 ? 1 : 0;
  note_stats(p, nnz - kept, n_grown);
  if (new_nnz) *new_nnz = kept + n_grown;
  if (n_grown_out) *n_grown_out = n_grown;
  if (kept == nnz && n_grown == 0) return ESCOIN_OK;   // nothing dropped or grown: the plan, its backward and update states stay
  if (const int rc = sync_host_values(p)) return rc;
  std::vector<int> host_map((size_t)nnz);
  const int rc = realign_rewired<T>(p, map.data(), gpos, gval.data(), host_map.data(), nullptr, map.data(), true, stream);
  p->align_ms = ms_since(t_start);
  p->rewire_realign_ms = p->align_ms - p->rewire_map_ms;
  return rc;
}

template <typename T>
int rewire_host(escoin_plan *p, const escoin_rewire_desc *d, int *entry_map, int *grown, long *new_nnz, long *n_grown_out) {
  typedef typename prune::KeyOf<T>::type K;
  const auto t_start = std::chrono::steady_clock::now();
  K thr_key = 0;
  long D = 0;
  if (const int rc = check_rewire<T>(p, d, &thr_key, &D)) return rc;
  const long nnz = plan_nnz(p);
  std::vector<int> own_map;
  if (!entry_map) {
    own_map.resize((size_t)nnz);
    entry_map = own_map.data();
  }
  std::vector<int> keep_map((size_t)nnz);
  long kept = nnz;
  if (d->drop) kept = prune::host_entry_map<T>(p, d->drop, thr_key, keep_map.data());
  std::vector<int> gpos;
  if (d->grow > 0 && nnz < D) {
    std::vector<unsigned char> in_pattern((size_t)D, 0);
    for (const int at : rewire::entry_positions(p->g.Mg, p->g.kdim, p->rowptr, p->colidx)) in_pattern[(size_t)at] = 1;
    gpos = rewire::select_grow<T>(static_cast<const T *>(d->score), in_pattern.data(), D, d->grow);
  }
  const long n_grown = (long)gpos.size();
  std::vector<T> gval((size_t)n_grown, (T)0);
  if (d->init)
    for (long i = 0; i < n_grown; ++i) std::memcpy(&gval[(size_t)i], static_cast<const T *>(d->init) + gpos[(size_t)i], sizeof(T));
  note_stats(p, nnz - kept, n_grown);
  if (new_nnz) *new_nnz = kept + n_grown;
  if (n_grown_out) *n_grown_out = n_grown;
  if (kept == nnz && n_grown == 0) {
    for (long e = 0; e < nnz; ++e) entry_map[e] = (int)e;
    return ESCOIN_OK;
  }
  const int rc = realign_rewired<T>(p, d->drop ? keep_map.data() : nullptr, gpos, gval.data(), entry_map, grown, nullptr, false, nullptr);
  p->align_ms = ms_since(t_start);
  return rc;
}

int check_args(const escoin_plan *p, const escoin_rewire_desc *d) {
  if (!p) return fail(ESCOIN_EINVAL, "rewire: null plan");
  if (!d) return fail(ESCOIN_EINVAL, "rewire: null descriptor");
  if (d->grow < 0) return fail(ESCOIN_EINVAL, "rewire: grow must be >= 0");
  if (d->grow > 0 && !d->score) return fail(ESCOIN_EINVAL, "rewire: grow > 0 needs a score");
  if ((long)p->g.d.M * p->g.kdim >= (1l << 31)) return fail(ESCOIN_EINVAL, "rewire: M * Cg * KH * KW must be below 2^31");
  return ESCOIN_OK;
}

}  // namespace
}  // namespace escoin

using namespace escoin;

extern "C" {

int escoin_plan_rewire(escoin_plan *p, const escoin_rewire_desc *desc, int *entry_map_dev, int *grown_dev, long *new_nnz,
                       long *n_grown, void *stream) {
  return guarded([&]() -> int {
    if (const int rc = check_args(p, desc)) return rc;
    if (const int rc = refuse_deconv(p, "escoin_plan_rewire")) return rc;
    if (const int rc = prune::check_device_plan(p, "rewire")) return rc;
    return p->is_f64 ? rewire_device<double>(p, desc, entry_map_dev, grown_dev, new_nnz, n_grown, (hipStream_t)stream)
                     : rewire_device<float>(p, desc, entry_map_dev, grown_dev, new_nnz, n_grown, (hipStream_t)stream);
  });
}

int escoin_plan_rewire_cpu(escoin_plan *p, const escoin_rewire_desc *desc, int *entry_map, int *grown, long *new_nnz,
                           long *n_grown) {
  return guarded([&]() -> int {
    if (const int rc = check_args(p, desc)) return rc;
    if (const int rc = refuse_deconv(p, "escoin_plan_rewire_cpu")) return rc;
    if (!p->host_aligned) return fail(ESCOIN_ESTATE, "rewire_cpu called before weight_align_cpu");
    if (p->aligned)
      return fail(ESCOIN_ESTATE, "rewire_cpu: the plan has a device side, which this entry point would leave behind; escoin_plan_rewire rewires both sides");
    return p->is_f64 ? rewire_host<double>(p, desc, entry_map, grown, new_nnz, n_grown)
                     : rewire_host<float>(p, desc, entry_map, grown, new_nnz, n_grown);
  });
}

}  // extern "C"
