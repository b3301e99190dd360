// rewire_rules.h -- the host-only half of drop-and-grow rewiring (include/escoin.h, "Rewiring"): the grow selection as
// plain host code, the merge of a host CSR with a kept map and a grown position list into set_csr's flat form, and the
// launch plan of the device kernels (rewire_select.hip).  No HIP header: this unit runs and is tested without a GPU,
// like prune_rules, whose key function and selection it is built on.
#ifndef ESCOIN_REWIRE_RULES_H_
#define ESCOIN_REWIRE_RULES_H_

#include <cstddef>
#include <vector>

#include "prune_rules.h"

namespace escoin {
namespace rewire {

// A position is p = oc * kdim + colidx (oc over all conv groups): an element of blobs_[0].  D = M * kdim < 2^31.
// The position of every entry of a host CSR (per conv group, as a plan holds it), in get_csr's order: ascending.
std::vector<int> entry_positions(int Mg, int kdim, const std::vector<std::vector<int>> &rowptr,
                                 const std::vector<std::vector<int>> &colidx);

// The grow selection.  The candidates are the positions p with in_pattern[p] == 0, ordered by (key(score[p]) descending,
// p ascending); the first min(grow, candidates) are grown and returned in ascending p.  score (D elements) is read at
// candidate positions only.  It is prune's KEEP rule over the candidates' keys (select_keep / build_map): NaN ranks highest,
// a zero score is an ordinary candidate.  grow >= 0.
template <typename T>
std::vector<int> select_grow(const T *score, const unsigned char *in_pattern, long D, long grow);

// The CSR that holds the kept entries of a host CSR and the grown positions, in the flat form escoin_plan_set_csr reads.
//   keep_map   old nnz elements, an entry is kept iff keep_map[e] >= 0 (a prune's entry map); NULL: every entry is kept
//   grown_pos  n_grown positions, strictly ascending, none of them in the old pattern (kept or dropped)
//   grown_val  the grown entries' values; NULL: +0.0
//   entry_map  out, old nnz elements: the entry's index in the new CSR, or -1; may be NULL
//   grown      out, n_grown elements: the new entry index of grown_pos[i]; may be NULL
// Returns false -- and leaves the outputs unspecified -- if the CSR is inconsistent or grown_pos breaks the above.
template <typename T>
bool merge(int Mg, int kdim, const std::vector<std::vector<int>> &rowptr, const std::vector<std::vector<int>> &colidx,
           const std::vector<std::vector<T>> &values, const int *keep_map, const int *grown_pos, const T *grown_val,
           long n_grown, prune::FlatCsr<T> *out, int *entry_map, int *grown);

// The launch plan of the device kernels, a function of D, nnz and the element size alone.  Workgroups, tiles and the
// grid cap are prune_rules.h's (kThreads, kItems, kTileEntries, kScanWidth, kMaxGrid); the tiles cover the D positions.
constexpr int kCounts = 3;                  // per tile: kept entries, candidates grown strictly, candidates that tie
constexpr int kSlotCandidate = -1;          // slot[p]: not in the pattern (what a byte fill of 0xff leaves)
constexpr int kSlotDropped = -2;            // slot[p]: an entry this call drops; slot[p] >= 0: the kept entry's old index
struct LaunchPlan : prune::LaunchPlan {   // prune's plan over the D positions with kCounts counts per tile, and
  int mark_grid;     // workgroups of the launch that marks the entries' positions (grid stride over the entries)
  size_t slot_bytes; // one int per position
};
LaunchPlan launch_plan(long D, long nnz, int elem_bytes);

}  // namespace rewire
}  // namespace escoin
#endif
