// prune_rules_san.cpp -- the host-only half of pruning (csrc/prune_rules.{h,cpp}) as a stand-alone program, built with
// plain g++ (no ROCm include path: the compile proves the unit is host-only) under the address and undefined-behaviour
// sanitizers by tests/test_prune_rules_san.py.  Over the score cases and sizes of the pruning tests: the sort-free
// selection against a stable sort on the keys, the entry map's shape, a CSR re-indexed through the map (and malformed
// maps refused), and the launch plan's bounds.  Prints one "OK ..." line per check; any mismatch exits non-zero.
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

#include "prune_rules.h"

using namespace escoin::prune;

static void die(const std::string &what) {
  std::printf("FAIL %s\n", what.c_str());
  std::exit(1);
}

template <typename T> struct Bits;
template <> struct Bits<float> { typedef uint32_t type; };
template <> struct Bits<double> { typedef uint64_t type; };

template <typename T>
static T from_bits(typename Bits<T>::type b) {
  T v;
  std::memcpy(&v, &b, sizeof(T));
  return v;
}

// name -> n scores (the cases of tests/prune_common.py, restated)
template <typename T>
static std::vector<std::pair<std::string, std::vector<T>>> score_cases(long n, unsigned seed) {
  typedef typename Bits<T>::type U;
  std::mt19937_64 rng(seed);
  std::vector<std::pair<std::string, std::vector<T>>> out;
  const T mags[6] = {(T)0.125, (T)0.25, (T)0.5, (T)0.75, (T)1.0, (T)1.5};
  std::vector<T> v((size_t)n);
  for (auto &x : v) x = mags[rng() % 6] * ((rng() & 1) ? (T)1 : (T)-1);
  out.push_back({"ties", v});
  for (auto &x : v) x = (T)((double)(rng() % 2000001) / 1e6 - 1.0);
  const T tiny = std::numeric_limits<T>::min();
  const T special[9] = {(T)0.0, (T)-0.0, std::numeric_limits<T>::quiet_NaN(), std::numeric_limits<T>::infinity(),
                        -std::numeric_limits<T>::infinity(), tiny / 2, -tiny / 4, tiny / 2, std::numeric_limits<T>::denorm_min()};
  for (long i = 0; i < std::min<long>(n, 9); ++i) v[(size_t)((i * 7919) % n)] = special[i];
  out.push_back({"specials", v});
  U base;
  const T one = (T)1.2345678901234567;
  std::memcpy(&base, &one, sizeof(T));
  for (int j = 0; j < (int)sizeof(T); ++j) {
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

template <typename K>
static std::vector<int> sorted_map(const std::vector<K> &keys, long keep) {
  const long n = (long)keys.size();
  std::vector<long> order((size_t)n);
  std::iota(order.begin(), order.end(), 0L);
  std::stable_sort(order.begin(), order.end(), [&](long a, long b) { return keys[(size_t)a] > keys[(size_t)b]; });
  std::vector<char> kept((size_t)n, 0);
  for (long i = 0; i < std::min(keep, n); ++i) kept[(size_t)order[(size_t)i]] = 1;
  std::vector<int> map((size_t)n);
  int next = 0;
  for (long e = 0; e < n; ++e) map[(size_t)e] = kept[(size_t)e] ? next++ : -1;
  return map;
}

template <typename T>
static void check_selection(const char *tname) {
  typedef typename KeyOf<T>::type K;
  const long Tl = kTileEntries;
  const long sizes[] = {1, 2, 63, 64, 65, Tl - 1, Tl, Tl + 1, 3 * Tl + 1};
  for (long n : sizes) {
    for (const auto &c : score_cases<T>(n, (unsigned)(n * 31 + sizeof(T)))) {
      const std::vector<K> keys = keys_of<T>(c.second.data(), n);
      for (long e = 0; e < n; ++e)
        if (keys[(size_t)e] != key_bits(c.second[(size_t)e]) || (keys[(size_t)e] >> (8 * sizeof(K) - 1))) die("key");
      const long keeps[] = {0, 1, n / 2, n / 2 + 1, n - 1, n, n + 5};
      for (long keep : keeps) {
        if (keep < 0) continue;
        const Boundary<K> b = select_keep<K>(keys.data(), n, keep);
        std::vector<int> map((size_t)n, 12345);
        const long kept = build_map<K>(keys.data(), n, b, map.data());
        if (kept != std::min(keep, n) || kept != build_map<K>(keys.data(), n, b, nullptr)) die(std::string(tname) + " kept count " + c.first);
        if (map != sorted_map<K>(keys, keep)) die(std::string(tname) + " map " + c.first + " n=" + std::to_string(n) + " keep=" + std::to_string(keep));
      }
      // THRESHOLD at an existing key, one above it, 0 and the largest key value
      const K mid = keys[(size_t)(n / 2)];
      const K thr[] = {0, mid, (K)(mid + 1), std::numeric_limits<K>::max() >> 1};
      for (K t : thr) {
        std::vector<int> map((size_t)n);
        const long kept = build_map<K>(keys.data(), n, select_threshold<K>(t), map.data());
        long want = 0;
        for (long e = 0; e < n; ++e) {
          const bool k = keys[(size_t)e] >= t;
          if (map[(size_t)e] != (k ? (int)want : -1)) die(std::string(tname) + " threshold map " + c.first);
          want += k;
        }
        if (kept != want) die("threshold count");
      }
    }
    std::printf("OK %s selection n=%ld\n", tname, n);
  }
  // n = 0: nothing to select, nothing read
  const Boundary<K> b0 = select_keep<K>(nullptr, 0, 3);
  if (build_map<K>(nullptr, 0, b0, nullptr) != 0) die("empty");
  std::printf("OK %s selection n=0\n", tname);
}

template <typename T>
static void check_apply(const char *tname) {
  // two conv groups of three rows; group 1's middle row is empty
  const int Mg = 3;
  const std::vector<std::vector<int>> rowptr = {{0, 2, 5, 6}, {0, 3, 3, 4}};
  const std::vector<std::vector<int>> colidx = {{1, 4, 0, 2, 7, 3}, {0, 5, 6, 2}};
  std::vector<std::vector<T>> values(2);
  for (int g = 0; g < 2; ++g)
    for (size_t j = 0; j < colidx[(size_t)g].size(); ++j) values[(size_t)g].push_back((T)(10 * g + (int)j) + (T)0.5);
  const std::vector<int> map = {0, -1, -1, 1, 2, -1, 3, -1, 4, 5};
  FlatCsr<T> out;
  if (!apply_entry_map<T>(Mg, rowptr, colidx, values, map.data(), (long)map.size(), &out)) die("apply refused a good map");
  if (out.rowptr != std::vector<int>({0, 1, 3, 3, 0, 2, 2, 3}) || out.colidx != std::vector<int>({1, 2, 7, 0, 6, 2}) ||
      out.nnz_per_group != std::vector<int>({3, 3}) ||
      out.values != std::vector<T>({(T)0.5, (T)3.5, (T)4.5, (T)10.5, (T)12.5, (T)13.5}))
    die(std::string(tname) + " apply result");
  const std::vector<int> none(10, -1);
  if (!apply_entry_map<T>(Mg, rowptr, colidx, values, none.data(), 10, &out) || !out.colidx.empty() ||
      out.rowptr != std::vector<int>(8, 0) || out.nnz_per_group != std::vector<int>({0, 0}))
    die("apply: everything dropped");
  std::vector<int> bad = map;
  bad[3] = 2;                              // not ascending by one over the kept entries
  if (apply_entry_map<T>(Mg, rowptr, colidx, values, bad.data(), 10, &out)) die("apply accepted a gap");
  if (apply_entry_map<T>(Mg, rowptr, colidx, values, map.data(), 9, &out)) die("apply accepted a short map");
  if (apply_entry_map<T>(Mg, rowptr, colidx, values, map.data(), 11, &out)) die("apply accepted a long map");
  std::printf("OK %s apply_entry_map\n", tname);
}

static void check_launch_plan() {
  const long sizes[] = {0, 1, 255, 256, 257, kTileEntries - 1, kTileEntries, kTileEntries + 1, 3L * kTileEntries + 1,
                        512L * 512 * 9, (long)kTileEntries * kScanWidth + 1, 2147483647L};
  for (int elem : {4, 8})
    for (long n : sizes)
      for (int counts : {2, 3}) {
        const LaunchPlan lp = launch_plan(n, elem, counts);
        if (lp.passes != elem) die("passes");
        if (lp.tiles * kTileEntries < n || (lp.tiles > 0 && (lp.tiles - 1) * kTileEntries >= n)) die("tiles");
        if (lp.hist_grid < 1 || lp.hist_grid > kMaxGrid || lp.tile_grid < 1 || lp.tile_grid > kMaxGrid) die("grid cap");
        if ((long)lp.scan_steps * kScanWidth < lp.tiles) die("scan steps");
        if (lp.ws_bytes < kStateBytes + (size_t)elem * 1024 + (size_t)lp.tiles * counts * 4) die("workspace");
        if (counts == 2 && lp.ws_bytes != launch_plan(n, elem).ws_bytes) die("default counts");
      }
  if (kTileEntries % 64 != 0 || kThreads % 64 != 0) die("tile is not whole waves");
  std::printf("OK launch_plan\n");
}

int main() {
  check_selection<float>("float");
  check_selection<double>("double");
  check_apply<float>("float");
  check_apply<double>("double");
  check_launch_plan();
  return 0;
}
