// rewire_rules.cpp -- see rewire_rules.h.  Host-only: no HIP header, no plan.
#include "rewire_rules.h"

#include <algorithm>
#include <cstdint>

namespace escoin {
namespace rewire {

std::vector<int> entry_positions(int Mg, int kdim, const std::vector<std::vector<int>> &rowptr,
                                 const std::vector<std::vector<int>> &colidx) {
  std::vector<int> pos;
  for (size_t grp = 0; grp < rowptr.size(); ++grp)
    for (int m = 0; m < Mg; ++m)
      for (int j = rowptr[grp][(size_t)m]; j < rowptr[grp][(size_t)m + 1]; ++j)
        pos.push_back((int)(((long)grp * Mg + m) * kdim + colidx[grp][(size_t)j]));
  return pos;
}

template <typename T>
std::vector<int> select_grow(const T *score, const unsigned char *in_pattern, long D, long grow) {
  typedef typename prune::KeyOf<T>::type K;
  std::vector<int> cand;
  std::vector<K> keys;
  for (long p = 0; p < D; ++p)
    if (!in_pattern[p]) {
      cand.push_back((int)p);
      keys.push_back(prune::key_bits(score[p]));
    }
  const long n = (long)cand.size();
  std::vector<int> map((size_t)n);
  const prune::Boundary<K> b = prune::select_keep<K>(keys.data(), n, grow);
  const long n_grown = prune::build_map<K>(keys.data(), n, b, map.data());
  std::vector<int> grown;
  grown.reserve((size_t)n_grown);
  for (long c = 0; c < n; ++c)
    if (map[(size_t)c] >= 0) grown.push_back(cand[(size_t)c]);
  return grown;
}

template <typename T>
bool merge(int Mg, int kdim, const std::vector<std::vector<int>> &rowptr, const std::vector<std::vector<int>> &colidx,
           const std::vector<std::vector<T>> &values, const int *keep_map, const int *grown_pos, const T *grown_val,
           long n_grown, prune::FlatCsr<T> *out, int *entry_map, int *grown) {
  const size_t G = rowptr.size();
  if (colidx.size() != G || values.size() != G || n_grown < 0) return false;
  out->rowptr.assign(G * (size_t)(Mg + 1), 0);
  out->nnz_per_group.assign(G, 0);
  out->colidx.clear();
  out->values.clear();
  long e = 0, gi = 0, next = 0;
  for (size_t grp = 0; grp < G; ++grp) {
    if ((int)rowptr[grp].size() != Mg + 1 || values[grp].size() != colidx[grp].size()) return false;
    int *rp = out->rowptr.data() + grp * (size_t)(Mg + 1);
    int n_g = 0;
    // the grown positions below `upto` that are still to come, which all lie in the row that starts at row0
    auto grow_upto = [&](long row0, long upto) -> bool {
      while (gi < n_grown && grown_pos[gi] < upto) {
        if (grown_pos[gi] < row0 || (gi > 0 && grown_pos[gi] <= grown_pos[gi - 1])) return false;
        out->colidx.push_back((int)(grown_pos[gi] - row0));
        out->values.push_back(grown_val ? grown_val[gi] : (T)0);
        if (grown) grown[gi] = (int)next;
        ++next, ++n_g, ++gi;
      }
      return true;
    };
    for (int m = 0; m < Mg; ++m) {
      const long row0 = ((long)grp * Mg + m) * kdim;
      if (rowptr[grp][(size_t)m] > rowptr[grp][(size_t)m + 1] || (size_t)rowptr[grp][(size_t)m + 1] > colidx[grp].size()) return false;
      for (int j = rowptr[grp][(size_t)m]; j < rowptr[grp][(size_t)m + 1]; ++j, ++e) {
        const int col = colidx[grp][(size_t)j];
        if (col < 0 || col >= kdim) return false;
        if (!grow_upto(row0, row0 + col)) return false;
        if (gi < n_grown && grown_pos[gi] == row0 + col) return false;   // a grown position inside the old pattern
        const bool kept = !keep_map || keep_map[e] >= 0;
        if (entry_map) entry_map[e] = kept ? (int)next : -1;
        if (!kept) continue;
        out->colidx.push_back(col);
        out->values.push_back(values[grp][(size_t)j]);
        ++next, ++n_g;
      }
      if (!grow_upto(row0, row0 + kdim)) return false;
      rp[m + 1] = n_g;
    }
    out->nnz_per_group[grp] = n_g;
  }
  return gi == n_grown;
}

LaunchPlan launch_plan(long D, long nnz, int elem_bytes) {
  LaunchPlan lp;
  static_cast<prune::LaunchPlan &>(lp) = prune::launch_plan(D, elem_bytes, kCounts);
  lp.mark_grid = prune::launch_plan(nnz, elem_bytes).hist_grid;   // a grid stride over the entries, as a prune's histogram
  lp.slot_bytes = (size_t)std::max<long>(D, 1) * sizeof(int);
  return lp;
}

template std::vector<int> select_grow<float>(const float *, const unsigned char *, long, long);
template std::vector<int> select_grow<double>(const double *, const unsigned char *, long, long);
template bool merge<float>(int, int, const std::vector<std::vector<int>> &, const std::vector<std::vector<int>> &,
                           const std::vector<std::vector<float>> &, const int *, const int *, const float *, long,
                           prune::FlatCsr<float> *, int *, int *);
template bool merge<double>(int, int, const std::vector<std::vector<int>> &, const std::vector<std::vector<int>> &,
                            const std::vector<std::vector<double>> &, const int *, const int *, const double *, long,
                            prune::FlatCsr<double> *, int *, int *);

}  // namespace rewire
}  // namespace escoin
