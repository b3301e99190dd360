// prune_rules.h -- the host-only half of magnitude pruning (include/escoin.h, "Pruning"): the key function, the selection
// rule as plain host code, the re-index of a host CSR through an entry map, and the launch plan of the device kernels
// (prune_select.hip).  No HIP header: this unit runs and is tested without a GPU, like align_rules / csr_tables.
#ifndef ESCOIN_PRUNE_RULES_H_
#define ESCOIN_PRUNE_RULES_H_

#include <cstdint>
#include <cstring>
#include <vector>

namespace escoin {
namespace prune {

// key(s): the bits of s with the sign bit cleared, compared as an unsigned integer.  -0.0 == +0.0, denormals rank
// exactly, inf ranks above every finite value and NaN above inf.  No floating-point comparison anywhere.
template <typename T> struct KeyOf;
template <> struct KeyOf<float> { typedef uint32_t type; };
template <> struct KeyOf<double> { typedef uint64_t type; };
inline uint32_t key_bits(float s) {
  uint32_t k;
  std::memcpy(&k, &s, 4);
  return k & 0x7fffffffu;
}
inline uint64_t key_bits(double s) {
  uint64_t k;
  std::memcpy(&k, &s, 8);
  return k & 0x7fffffffffffffffull;
}

// The keep rule in the form both sides evaluate per entry:
//   ge != 0:  kept iff key >= T                                       (THRESHOLD; KEEP with nothing to drop: T = 0)
//   ge == 0:  kept iff key > T, or key == T and fewer than `ties` entries with key == T precede it (by entry index)
// (KEEP with keep == 0: T = the largest key value, ties = 0.)
template <typename K>
struct Boundary {
  K T;
  long ties;
  int ge;
};

// KEEP: the boundary that keeps exactly min(keep, n) entries, the largest keys first, equal keys by ascending entry
// index.  A radix select from the top byte down, sizeof(K) histogram passes over the keys -- no sort -- which is the
// device's algorithm step for step (prune_select.hip).  keep >= 0.
template <typename K> Boundary<K> select_keep(const K *keys, long n, long keep);
// THRESHOLD: kept iff key >= key(threshold)
template <typename K> inline Boundary<K> select_threshold(K key_of_threshold) { return Boundary<K>{key_of_threshold, 0, 1}; }
// map[e] = the index of entry e among the kept entries, or -1; returns the number kept.  map may be NULL (count only).
template <typename K> long build_map(const K *keys, long n, const Boundary<K> &b, int *map);
// the keys of n scores
template <typename T> std::vector<typename KeyOf<T>::type> keys_of(const T *s, long n);

// A host CSR (per conv group, as a plan holds it) re-indexed through an entry map, in the flat form escoin_plan_set_csr
// reads: rowptr [group x (Mg + 1)], colidx / values [new nnz] with the groups concatenated, nnz_per_group [group].
template <typename T>
struct FlatCsr {
  std::vector<int> rowptr, colidx, nnz_per_group;
  std::vector<T> values;
};
// The map covers the entries of all groups concatenated (get_csr's order).  Returns false -- and leaves *out unspecified --
// if the map is not -1 / 0, 1, 2, ... ascending over the kept entries, or its length is not the CSR's nnz.
template <typename T>
bool apply_entry_map(int Mg, const std::vector<std::vector<int>> &rowptr, const std::vector<std::vector<int>> &colidx,
                     const std::vector<std::vector<T>> &values, const int *map, long map_len, FlatCsr<T> *out);

// The launch plan of the device kernels (radix_select.h), a function of the number of indices the select ranges over (a
// prune: nnz), the element size and the counts a tile carries alone.
constexpr int kThreads = 256;                       // lanes of every workgroup (four full waves of 64)
constexpr int kItems = 4;                           // entries per lane of a tile
constexpr int kTileEntries = kThreads * kItems;     // entries one workgroup of the count / apply kernels covers per step
constexpr int kScanWidth = kThreads;                // tiles the scanning workgroup takes per loop step
constexpr int kMaxGrid = 2048;                      // workgroups of a histogram / count / apply launch, at most
struct LaunchPlan {
  int passes;       // histogram passes of the radix select: one per key byte
  long tiles;       // ceil(nnz / kTileEntries)
  int hist_grid;    // workgroups of a histogram launch (grid stride over the entries)
  int tile_grid;    // workgroups of the count / apply launches (grid stride over the tiles)
  int scan_steps;   // loop steps of the one scanning workgroup: ceil(tiles / kScanWidth)
  size_t ws_bytes;  // the device workspace: selection state, sizeof(K) histograms, `counts` counts per tile
};
constexpr size_t kStateBytes = 64;                  // the selection state at the head of the workspace
LaunchPlan launch_plan(long nnz, int elem_bytes, int counts = 2);   // (a prune's two: kept strictly, tie)

}  // namespace prune
}  // namespace escoin
#endif
