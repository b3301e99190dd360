// prune_rules.cpp -- see prune_rules.h.  Host-only: no HIP header, no plan.
#include "prune_rules.h"

#include <algorithm>
#include <limits>

namespace escoin {
namespace prune {

template <typename K>
Boundary<K> select_keep(const K *keys, long n, long keep) {
  if (keep >= n) return Boundary<K>{0, 0, 1};
  if (keep <= 0) return Boundary<K>{std::numeric_limits<K>::max(), 0, 0};
  // 0 < keep < n: in every pass the entries that match the prefix number at least `remaining` >= 1, so a digit is found
  const int passes = (int)sizeof(K);
  K prefix = 0;
  long remaining = keep;
  for (int d = 0; d < passes; ++d) {
    const int shift = 8 * (passes - 1 - d);
    long hist[256] = {0};
    for (long e = 0; e < n; ++e)
      if (d == 0 || (keys[e] >> (shift + 8)) == prefix) ++hist[(keys[e] >> shift) & 0xff];
    long above = 0;   // matching entries whose digit is larger than the one looked at
    int digit = 0;
    for (int b = 255; b >= 0; --b) {
      if (above + hist[b] >= remaining) {
        digit = b;
        break;
      }
      above += hist[b];
    }
    remaining -= above;
    prefix = (K)((prefix << 8) | (K)digit);
  }
  return Boundary<K>{prefix, remaining, 0};
}

template <typename K>
long build_map(const K *keys, long n, const Boundary<K> &b, int *map) {
  long kept = 0, ties_seen = 0;
  for (long e = 0; e < n; ++e) {
    bool keep;
    if (b.ge) {
      keep = keys[e] >= b.T;
    } else if (keys[e] == b.T) {
      keep = ties_seen < b.ties;
      ++ties_seen;
    } else {
      keep = keys[e] > b.T;
    }
    if (map) map[e] = keep ? (int)kept : -1;
    kept += keep ? 1 : 0;
  }
  return kept;
}

template <typename T>
std::vector<typename KeyOf<T>::type> keys_of(const T *s, long n) {
  std::vector<typename KeyOf<T>::type> k((size_t)std::max<long>(n, 0));
  for (long e = 0; e < n; ++e) k[(size_t)e] = key_bits(s[e]);
  return k;
}

template <typename T>
bool apply_entry_map(int Mg, const std::vector<std::vector<int>> &rowptr, const std::vector<std::vector<int>> &colidx,
                     const std::vector<std::vector<T>> &values, const int *map, long map_len, FlatCsr<T> *out) {
  const size_t G = rowptr.size();
  long nnz = 0;
  for (size_t grp = 0; grp < G; ++grp) nnz += (long)colidx[grp].size();
  if (nnz != map_len || colidx.size() != G || values.size() != G) return false;
  out->rowptr.assign(G * (size_t)(Mg + 1), 0);
  out->nnz_per_group.assign(G, 0);
  out->colidx.clear();
  out->values.clear();
  long e = 0, next = 0;
  for (size_t grp = 0; grp < G; ++grp) {
    if ((int)rowptr[grp].size() != Mg + 1 || values[grp].size() != colidx[grp].size()) return false;
    int *rp = out->rowptr.data() + grp * (size_t)(Mg + 1);
    int n_g = 0;
    for (int m = 0; m < Mg; ++m) {
      for (int j = rowptr[grp][m]; j < rowptr[grp][m + 1]; ++j, ++e) {
        if (e >= map_len) return false;
        if (map[e] < 0) continue;
        if (map[e] != next) return false;
        ++next;
        out->colidx.push_back(colidx[grp][(size_t)j]);
        out->values.push_back(values[grp][(size_t)j]);
        ++n_g;
      }
      rp[m + 1] = n_g;
    }
    out->nnz_per_group[grp] = n_g;
  }
  return e == map_len;
}

LaunchPlan launch_plan(long nnz, int elem_bytes, int counts) {
  LaunchPlan lp;
  const long n = std::max<long>(nnz, 0);
  lp.passes = elem_bytes == 8 ? 8 : 4;
  lp.tiles = (n + kTileEntries - 1) / kTileEntries;
  lp.hist_grid = (int)std::max<long>(1, std::min<long>((n + kThreads - 1) / kThreads, kMaxGrid));
  lp.tile_grid = (int)std::max<long>(1, std::min<long>(lp.tiles, kMaxGrid));
  lp.scan_steps = (int)((lp.tiles + kScanWidth - 1) / kScanWidth);
  lp.ws_bytes = kStateBytes + (size_t)lp.passes * 256 * sizeof(uint32_t) + (size_t)std::max<long>(lp.tiles, 1) * (size_t)counts * sizeof(uint32_t);
  return lp;
}

template Boundary<uint32_t> select_keep<uint32_t>(const uint32_t *, long, long);
template Boundary<uint64_t> select_keep<uint64_t>(const uint64_t *, long, long);
template long build_map<uint32_t>(const uint32_t *, long, const Boundary<uint32_t> &, int *);
template long build_map<uint64_t>(const uint64_t *, long, const Boundary<uint64_t> &, int *);
template std::vector<uint32_t> keys_of<float>(const float *, long);
template std::vector<uint64_t> keys_of<double>(const double *, long);
template bool apply_entry_map<float>(int, const std::vector<std::vector<int>> &, const std::vector<std::vector<int>> &,
                                     const std::vector<std::vector<float>> &, const int *, long, FlatCsr<float> *);
template bool apply_entry_map<double>(int, const std::vector<std::vector<int>> &, const std::vector<std::vector<int>> &,
                                      const std::vector<std::vector<double>> &, const int *, long, FlatCsr<double> *);

}  // namespace prune
}  // namespace escoin
