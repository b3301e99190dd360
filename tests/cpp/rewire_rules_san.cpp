// rewire_rules_san.cpp -- the host-only half of rewiring (csrc/rewire_rules.{h,cpp} on csrc/prune_rules.{h,cpp}) as a
// stand-alone program, built with plain g++ (no ROCm include path: the compile proves the unit is host-only) under the
// address and undefined-behaviour sanitizers by tests/test_rewire_rules_san.py.  Over the dense sizes of the rewiring
// tests: the sort-free grow selection against a stable sort on the candidates' keys, the merge of a CSR with a kept map
// and a grown list (and malformed lists refused), the entry positions, and the launch plan's bounds.  Prints one
// "OK ..." line per check; any mismatch exits non-zero.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "rewire_rules.h"

using namespace escoin;
using namespace escoin::rewire;

static void die(const std::string &what) {
  std::printf("FAIL %s\n", what.c_str());
  std::exit(1);
}

template <typename T>
static T from_bits(typename prune::KeyOf<T>::type b) {
  T v;
  std::memcpy(&v, &b, sizeof(T));
  return v;
}

// name -> n scores (the cases of tests/prune_common.py, restated); few: only "ties", "specials", "all_equal"
template <typename T>
static std::vector<std::pair<std::string, std::vector<T>>> score_cases(long n, unsigned seed, bool few) {
  typedef typename prune::KeyOf<T>::type U;
  std::mt19937_64 rng(seed);
  std::vector<std::pair<std::string, std::vector<T>>> out;
  const T mags[6] = {(T)0.125, (T)0.25, (T)0.5, (T)0.75, (T)1.0, (T)1.5};
  std::vector<T> v((size_t)n);
  for (auto &x : v) x = mags[rng() % 6] * ((rng() & 1) ? (T)1 : (T)-1);
  out.push_back({"ties", v});
  for (auto &x : v) x = (T)((double)(rng() % 2000001) / 1e6 - 1.0);
  const T tiny = std::numeric_limits<T>::min();
  // (a NaN with every mantissa bit set is the largest key there is; zeros are ordinary candidates)
  const T special[10] = {(T)0.0, (T)-0.0, std::numeric_limits<T>::quiet_NaN(), std::numeric_limits<T>::infinity(),
                         -std::numeric_limits<T>::infinity(), tiny / 2, -tiny / 4, tiny / 2, std::numeric_limits<T>::denorm_min(),
                         from_bits<T>((U)(~(U)0 >> 1))};
  for (long i = 0; i < std::min<long>(n, 10); ++i) v[(size_t)((i * 7919) % n)] = special[i];
  out.push_back({"specials", v});
  U base;
  const T one = (T)1.2345678901234567;
  std::memcpy(&base, &one, sizeof(T));
  for (int j = 0; j < (int)sizeof(T) && !few; ++j) {
    const int width = j == (int)sizeof(T) - 1 ? 7 : 8;
    for (auto &x : v) {
      const U digit = (U)(rng() % (1u << width));
      const U sign = (U)(rng() & 1) << (8 * sizeof(T) - 1);
      x = from_bits<T>((U)((base & ~((U)0xff << (8 * j))) | (digit << (8 * j)) | sign));
    }
    out.push_back({"byte" + std::to_string(j), v});
  }
  for (auto &x : v) x = (T)0.37 * ((rng() & 1) ? (T)1 : (T)-1);
  out.push_back({"all_equal", v});
  return out;
}

// the rule by a stable sort: the first `grow` candidates by descending key, ascending position
template <typename T>
static std::vector<int> sorted_grow(const std::vector<T> &score, const std::vector<unsigned char> &in_pattern, long grow) {
  std::vector<int> cand;
  for (size_t p = 0; p < score.size(); ++p)
    if (!in_pattern[p]) cand.push_back((int)p);
  std::stable_sort(cand.begin(), cand.end(), [&](int a, int b) { return prune::key_bits(score[(size_t)a]) > prune::key_bits(score[(size_t)b]); });
  cand.resize((size_t)std::min<long>(grow, (long)cand.size()));
  std::sort(cand.begin(), cand.end());
  return cand;
}

template <typename T>
static void check_grow(const char *tname) {
  const long T1 = prune::kTileEntries;
  // the dense sizes of tests/test_rewire_gpu.py: a partial and a whole wave, a tile edge, more tiles than the scanning
  // workgroup is wide, more tiles than the grid cap (at the last two: three score cases and one grow count)
  const long sizes[] = {63, 64, 65, T1 + 1, T1 + 128, (long)T1 * prune::kScanWidth + 512, (long)T1 * prune::kMaxGrid + 257536};
  for (long D : sizes) {
    const bool big = D > (long)T1 * prune::kScanWidth;
    std::mt19937_64 rng((unsigned)D);
    std::vector<unsigned char> in_pattern((size_t)D);
    long nnz = 0;
    for (auto &m : in_pattern) nnz += (m = (rng() % 10) < (D > (long)T1 * prune::kMaxGrid ? 1 : 3));
    const long n_cand = D - nnz;
    for (const auto &c : score_cases<T>(D, (unsigned)(D * 31 + sizeof(T)), big)) {
      std::vector<T> score = c.second;
      for (long p = 0; p < D; ++p)
        if (in_pattern[(size_t)p] && p % 3 == 0) score[(size_t)p] = std::numeric_limits<T>::quiet_NaN();   // never ranked
      std::vector<long> grows = {n_cand / 2};
      if (!big) grows.insert(grows.end(), {0L, 1L, n_cand / 2 + 1, n_cand - 1, n_cand, n_cand + 5});
      for (long grow : grows) {
        if (grow < 0) continue;
        const std::vector<int> got = select_grow<T>(score.data(), in_pattern.data(), D, grow);
        if ((long)got.size() != std::min(grow, n_cand)) die(std::string(tname) + " grown count " + c.first);
        if (got != sorted_grow<T>(score, in_pattern, grow))
          die(std::string(tname) + " grow " + c.first + " D=" + std::to_string(D) + " grow=" + std::to_string(grow));
      }
    }
    std::printf("OK %s grow D=%ld\n", tname, D);
  }
  // no candidate at all, and D = 0: nothing read
  const std::vector<unsigned char> full(64, 1);
  const std::vector<T> s(64, (T)1);
  if (!select_grow<T>(s.data(), full.data(), 64, 5).empty() || !select_grow<T>(nullptr, nullptr, 0, 5).empty()) die("no candidates");
  std::printf("OK %s grow without candidates\n", tname);
}

template <typename T>
static void check_merge(const char *tname) {
  // two conv groups of three rows of kdim 8; group 1's middle row is empty
  const int Mg = 3, kdim = 8;
  const std::vector<std::vector<int>> rowptr = {{0, 2, 5, 6}, {0, 3, 3, 4}};
  const std::vector<std::vector<int>> colidx = {{1, 4, 0, 2, 7, 3}, {0, 5, 6, 2}};
  std::vector<std::vector<T>> values(2);
  for (int g = 0; g < 2; ++g)
    for (size_t j = 0; j < colidx[(size_t)g].size(); ++j) values[(size_t)g].push_back((T)(10 * g + (int)j) + (T)0.5);
  if (entry_positions(Mg, kdim, rowptr, colidx) != std::vector<int>({1, 4, 8, 10, 15, 19, 24, 29, 30, 42})) die("entry_positions");
  const std::vector<int> keep = {0, -1, -1, 1, 2, -1, 3, -1, 4, 5};
  // grown: before the first entry, between two entries of a row, in the empty row, after the last entry of the last row
  const std::vector<int> gpos = {0, 9, 33, 47};
  const std::vector<T> gval = {(T)-1, (T)-2, (T)-3, (T)-4};
  prune::FlatCsr<T> out;
  std::vector<int> map(10, 777), grown(4, 777);
  if (!merge<T>(Mg, kdim, rowptr, colidx, values, keep.data(), gpos.data(), gval.data(), 4, &out, map.data(), grown.data()))
    die("merge refused a good list");
  if (out.rowptr != std::vector<int>({0, 2, 5, 5, 0, 2, 3, 5}) || out.colidx != std::vector<int>({0, 1, 1, 2, 7, 0, 6, 1, 2, 7}) ||
      out.nnz_per_group != std::vector<int>({5, 5}) ||
      out.values != std::vector<T>({(T)-1, (T)0.5, (T)-2, (T)3.5, (T)4.5, (T)10.5, (T)12.5, (T)-3, (T)13.5, (T)-4}))
    die(std::string(tname) + " merge result");
  if (map != std::vector<int>({1, -1, -1, 3, 4, -1, 5, -1, 6, 8}) || grown != std::vector<int>({0, 2, 7, 9})) die(std::string(tname) + " merge maps");
  // no drop, no values: every entry kept, grown entries +0.0; NULL outputs
  if (!merge<T>(Mg, kdim, rowptr, colidx, values, nullptr, gpos.data(), nullptr, 4, &out, nullptr, nullptr) || out.colidx.size() != 14 ||
      out.values[0] != (T)0 || std::signbit(out.values[0]) || out.nnz_per_group != std::vector<int>({8, 6}))
    die("merge without a drop");
  // nothing grown equals prune's re-index
  prune::FlatCsr<T> pruned;
  if (!merge<T>(Mg, kdim, rowptr, colidx, values, keep.data(), nullptr, nullptr, 0, &out, map.data(), nullptr) ||
      !prune::apply_entry_map<T>(Mg, rowptr, colidx, values, keep.data(), 10, &pruned) || out.rowptr != pruned.rowptr ||
      out.colidx != pruned.colidx || out.values != pruned.values || out.nnz_per_group != pruned.nnz_per_group || map != keep)
    die("merge without a grow is not apply_entry_map");
  // refused: a grown position inside the pattern (kept, and dropped), out of range, negative, not ascending
  for (const std::vector<int> &bad : {std::vector<int>{1}, std::vector<int>{4}, std::vector<int>{48}, std::vector<int>{-1},
                                      std::vector<int>{9, 9}, std::vector<int>{33, 9}})
    if (merge<T>(Mg, kdim, rowptr, colidx, values, keep.data(), bad.data(), nullptr, (long)bad.size(), &out, nullptr, nullptr))
      die("merge accepted a bad grown list starting at " + std::to_string(bad[0]));
  // an empty CSR grows
  const std::vector<std::vector<int>> rp0 = {{0, 0, 0, 0}, {0, 0, 0, 0}}, ci0 = {{}, {}};
  const std::vector<std::vector<T>> va0 = {{}, {}};
  if (!merge<T>(Mg, kdim, rp0, ci0, va0, nullptr, gpos.data(), gval.data(), 4, &out, nullptr, grown.data()) ||
      out.rowptr != std::vector<int>({0, 1, 2, 2, 0, 0, 1, 2}) || grown != std::vector<int>({0, 1, 2, 3}))
    die("merge into an empty CSR");
  std::printf("OK %s merge\n", tname);
}

static void check_launch_plan() {
  const long T1 = prune::kTileEntries;
  const long sizes[] = {0, 1, 63, 64, 65, 255, 256, 257, T1 - 1, T1, T1 + 1, (long)T1 * prune::kScanWidth + 512,
                        (long)T1 * prune::kMaxGrid + 257536, 2147483647L};
  for (int elem : {4, 8})
    for (long D : sizes)
      for (long nnz : {0L, D / 10, D}) {
        const LaunchPlan lp = launch_plan(D, nnz, elem);
        if (lp.passes != elem) die("passes");
        if (lp.tiles * T1 < D || (lp.tiles > 0 && (lp.tiles - 1) * T1 >= D)) die("tiles");
        for (int g : {lp.hist_grid, lp.tile_grid, lp.mark_grid})
          if (g < 1 || g > prune::kMaxGrid) die("grid cap");
        if ((long)lp.scan_steps * prune::kScanWidth < lp.tiles) die("scan steps");
        if (lp.ws_bytes < prune::kStateBytes + (size_t)elem * 1024 + (size_t)lp.tiles * kCounts * 4) die("workspace");
        if (lp.slot_bytes < (size_t)D * 4) die("slots");
      }
  if (kSlotCandidate != -1 || kSlotDropped >= 0 || kSlotDropped == kSlotCandidate) die("slot codes");
  std::printf("OK launch_plan\n");
}

int main() {
  check_grow<float>("float");
  check_grow<double>("double");
  check_merge<float>("float");
  check_merge<double>("double");
  check_launch_plan();
  return 0;
}
