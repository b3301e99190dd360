// prune_select.h -- what prune_select.hip shares with rewire_select.hip: the selection state at the head of a select's
// workspace, the descriptor check, the launch sequence of the drop selection, the two launches of a radix select that do
// not read keys (init, choose), and the host form of the drop's entry map.  Not part of the C ABI.
#ifndef ESCOIN_PRUNE_SELECT_H_
#define ESCOIN_PRUNE_SELECT_H_

#include "escoin_plan.h"
#include "prune_rules.h"

namespace escoin {
namespace prune {

// The head of the workspace (kStateBytes).  During the select: prefix = the key bytes chosen so far, remaining = entries
// still to take among the keys that match it.  Afterwards: prefix = T, remaining = the ties that fit.
struct SelState {
  unsigned long long prefix, remaining;
  unsigned ge, pad;
  unsigned long long total_gt, total_eq;
};
static_assert(sizeof(SelState) <= kStateBytes, "selection state outgrew its slot");

// What every entry point checks of a prune descriptor; thr_key: key(threshold) in the plan's Dtype.  T = float | double.
template <typename T> int check_desc(const escoin_prune_desc *d, typename KeyOf<T>::type *thr_key);

// The drop selection's launches on `stream`: init, (KEEP with 0 < keep < nnz: one histogram and one choose launch per key
// byte), count, scan, apply -> entry_map_dev[nnz].  ws: launch_plan(nnz, sizeof(K)).ws_bytes of device memory.  nnz > 0,
// `d` checked.  Asynchronous; K = uint32_t | uint64_t.
template <typename K>
int launch_selection(const K *keys, long nnz, const LaunchPlan &lp, const escoin_prune_desc *d, K thr_key, void *ws,
                     int *entry_map_dev, hipStream_t stream);

// escoin_prune_init_kernel / escoin_prune_choose_kernel for a select over other keys (rewire_select.hip's candidates)
void launch_select_init(SelState *st, unsigned *hist, int hist_words, unsigned long long prefix, unsigned long long remaining,
                        unsigned ge, hipStream_t stream);
void launch_select_choose(SelState *st, const unsigned *hist, hipStream_t stream);

// The drop's entry map as plain host code (prune_rules), on d->score or the plan's host values; map: nnz elements.
// Returns the number kept.  T = float | double.
template <typename T>
long host_entry_map(escoin_plan *p, const escoin_prune_desc *d, typename KeyOf<T>::type thr_key, int *map);

}  // namespace prune
}  // namespace escoin
#endif
