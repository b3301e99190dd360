// prune_select.h -- what prune_select.hip shares with rewire_select.hip on the host: the descriptor check, the launch
// sequence of the drop selection, the host form of the drop's entry map, and the orchestration both device entry points
// run around their launches (the device preconditions, the event timer, the tail of the re-align).  The device side they
// share is radix_select.h.  Not part of the C ABI.
#ifndef ESCOIN_PRUNE_SELECT_H_
#define ESCOIN_PRUNE_SELECT_H_

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "escoin_plan.h"
#include "prune_rules.h"

namespace escoin {
namespace prune {

// What every entry point checks of a prune descriptor; thr_key: key(threshold) in the plan's Dtype.  T = float | double.
template <typename T> int check_desc(const escoin_prune_desc *d, typename KeyOf<T>::type *thr_key);

// The drop selection's launches on `stream`: init, (KEEP with 0 < keep < nnz: one histogram and one choose launch per key
// byte), count, scan, apply -> entry_map_dev[nnz].  ws: launch_plan(nnz, sizeof(K)).ws_bytes of device memory.  nnz > 0,
// `d` checked.  Asynchronous; K = uint32_t | uint64_t.
template <typename K>
int launch_selection(const K *keys, long nnz, const LaunchPlan &lp, const escoin_prune_desc *d, K thr_key, void *ws,
                     int *entry_map_dev, hipStream_t stream);

// The drop's entry map as plain host code (prune_rules), on d->score or the plan's host values; map: nnz elements.
// Returns the number kept.  T = float | double.
template <typename T>
long host_entry_map(escoin_plan *p, const escoin_prune_desc *d, typename KeyOf<T>::type thr_key, int *map);

// What escoin_plan_prune / escoin_plan_rewire (`name`: "prune" / "rewire") need of the device: one is present, the plan is
// aligned on it, and it is the current one.
int check_device_plan(const escoin_plan *p, const char *name);

// Two events around a call's launches on one stream (stats "prune_kernels_us" / "rewire_kernels_us"; the call synchronises
// and allocates anyway).  `name` prefixes the failure message.
class EventTimer {
 public:
  EventTimer() = default;
  EventTimer(const EventTimer &) = delete;
  EventTimer &operator=(const EventTimer &) = delete;
  ~EventTimer() {
    if (a_) (void)hipEventDestroy(a_);
    if (b_) (void)hipEventDestroy(b_);
  }
  int start(const char *name, hipStream_t stream) {
    if (hipEventCreate(&a_) != hipSuccess || hipEventCreate(&b_) != hipSuccess)
      return fail(ESCOIN_EHIP, std::string(name) + ": hipEventCreate failed");
    ESCOIN_HIP_TRY(hipEventRecord(a_, stream));
    return ESCOIN_OK;
  }
  int stop(hipStream_t stream) {
    ESCOIN_HIP_TRY(hipEventRecord(b_, stream));
    return ESCOIN_OK;
  }
  // once the stream is synchronised
  int elapsed_ms(double *ms) const {
    float f = 0.f;
    ESCOIN_HIP_TRY(hipEventElapsedTime(&f, a_, b_));
    *ms = f;
    return ESCOIN_OK;
  }

 private:
  hipEvent_t a_ = nullptr, b_ = nullptr;
};

// The tail of a prune's or a rewire's re-align: the new host CSR through set_csr's own checks, then -- for a device-aligned
// plan -- the device side rebuilt from it, as escoin_plan_set_csr does.  t0: when the caller began to build `csr`; what:
// the head of the verbose line.
template <typename T>
int realign_on(escoin_plan *p, const FlatCsr<T> &csr, bool device, hipStream_t stream, std::chrono::steady_clock::time_point t0,
               const std::string &what) {
  const int rc = set_csr_host<T>(p, csr.rowptr.data(), csr.colidx.data(), csr.values.data(), csr.nnz_per_group.data());
  if (rc != ESCOIN_OK) return rc;
  const double ms_csr = ms_since(t0);
  const int rc2 = device ? realign_from_host_csr(p, stream) : ESCOIN_OK;
  if (getenv("ESCOIN_VERBOSE"))
    fprintf(stderr, "[escoin] %s: new host CSR %.2f ms, device side rebuilt in %.2f ms\n", what.c_str(), ms_csr, ms_since(t0) - ms_csr);
  return rc2;
}

}  // namespace prune
}  // namespace escoin
#endif
