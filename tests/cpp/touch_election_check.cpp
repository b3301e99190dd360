// tests/cpp/touch_election_check.cpp -- which workgroups of a tiled launch touch generated code with whole lines
// (csrc/align_rules.h touch_election / touch_workgroup / touch_lines), on the host alone (test code).
//
// Compiled with plain g++ against align_rules.cpp, stream_builder.cpp and jit_codegen.cpp: no HIP header, no device.
// Geometries: the rows of the manifest (tests/layout_cases.py BODY, tiled by the product's jit_layout for a batch of 256)
// and the table of tests/cpp/emulate_tiled.cpp with the tilings that file gives them.  Every geometry is launched at its
// own batch and at 256 images, on 256, 64 and 8 compute units, in launch order and grouped by XCD, and every linear
// workgroup id of every launch is enumerated: the sets that share an XCD and a grid row are built by sorting ids, with
// no use of the rank arithmetic under test.
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "align_rules.h"

using namespace escoin;

struct Case { int N, C, H, W, M, KH, KW, ph, pw, group; float sparsity; int waves; int lds; int ncu = 1; int product = 0; };

static int fail(const std::string &name, const char *what, long a = 0, long b = 0) {
  printf("%s: %s (%ld, %ld)\n", name.c_str(), what, a, b);
  return 1;
}

// One launch shape at every stride: 0 when everything holds.
static int check_launch(const std::string &name, const TiledLaunchShape &s, const Tiling &t, int n_cu, long *n_sets) {
  const int nwg = s.grid_x * s.grid_y;
  const int n_pref = 3;
  // the renumbering, built from its description: XCD x runs consecutive (row-major) workgroups, XCD 0's first
  std::vector<int> wg_of(nwg);
  if (s.xcd_q >= 0) {
    int next = 0;
    for (int x = 0; x < kTouchXcds; ++x)
      for (int orig = x; orig < nwg; orig += kTouchXcds) wg_of[orig] = next++;
    if (next != nwg) return fail(name, "renumbering is not a bijection", next, nwg);
  } else {
    for (int orig = 0; orig < nwg; ++orig) wg_of[orig] = orig;
  }
  // sets that share an L2 and code: (XCD = id % 8, grid row), members in ascending id = dispatch order
  std::map<std::pair<int, int>, std::vector<int>> sets;
  for (int orig = 0; orig < nwg; ++orig) sets[{orig % kTouchXcds, wg_of[orig] / s.grid_x}].push_back(orig);
  *n_sets += (long)sets.size();
  const int rule = touch_election(s, true, n_pref, n_cu, 0);
  // what the rule ships: kTouchRuleStride on a device of eight XCDs, 1 where it does not take the device for one
  if (rule != (n_cu == 8 ? 1 : kTouchRuleStride)) return fail(name, "the rule's stride is not the shipped one", rule, n_cu);
  for (int option : {0, 2, 65535}) {
    if (touch_election(s, false, n_pref, n_cu, option) != 1) return fail(name, "stream plans have no code to touch", option);
    if (touch_election(s, true, 0, n_cu, option) != 1) return fail(name, "plans without touches keep stride 1", option);
  }
  size_t largest = 1;
  for (const auto &kv : sets) largest = std::max(largest, kv.second.size());
  const int options[] = {0, 1, 2, 3, 4, 7, 8, 16, (int)largest, 65535, 1000000};
  for (int option : options) {
    const int T = touch_election(s, true, n_pref, n_cu, option);
    if (option >= 1 && T != std::min(option, kTouchMaxStride)) return fail(name, "a forced stride is not honoured", option, T);
    if (option == 0 && T != rule) return fail(name, "the rule is not a function of its arguments", T, rule);
    long touchers = 0, lines = 0;
    for (const auto &kv : sets) {
      int in_set = 0;
      for (size_t rank = 0; rank < kv.second.size(); ++rank) {
        const int orig = kv.second[rank];
        const TouchWorkgroup w = touch_workgroup(s, orig, T);
        if (w.xcd != kv.first.first || w.by != kv.first.second || w.bx != wg_of[orig] % s.grid_x)
          return fail(name, "touch_workgroup places a workgroup elsewhere", orig, T);
        const bool want = rank % (size_t)T == 0;
        if (w.toucher != want) return fail(name, "wrong election", orig, T);
        if (rank == 0 && !w.toucher) return fail(name, "rank 0 of a set does not touch", orig, T);
        if (T == 1 && !w.toucher) return fail(name, "T = 1 must mark every workgroup", orig);
        in_set += w.toucher;
        long walked = 0;
        for (int tile = w.bx; tile < s.tiles; tile += s.grid_x) ++walked;
        lines += (long)t.waves * n_pref * (1 + walked * t.n_icb) * (w.toucher ? 64 : 1);
      }
      if (in_set < 1) return fail(name, "a set without a toucher", kv.first.first, kv.first.second);
      if ((size_t)T >= kv.second.size() && in_set != 1) return fail(name, "a set smaller than T has more than its first member", in_set, T);
      touchers += in_set;
    }
    long got_touchers = -1;
    const long got = touch_lines(s, t, n_pref, T, &got_touchers);
    if (got != lines || got_touchers != touchers) return fail(name, "touch_lines differs from the enumerated count", got, lines);
  }
  return 0;
}

static int check_geometry(const std::string &name, const Geometry &g, const Tiling &t, long *n_launches, long *n_sets) {
  const int batches[] = {g.d.N, 256};
  const int cus[] = {256, 64, 8};
  for (int n_images : batches)
    for (int n_cu : cus)
      for (long code_bytes : {0l, 1l << 30}) {      // launch order / grouped by XCD wherever the launch has rows to group
        const TiledLaunchShape s = tiled_launch_shape(g, t, n_images, g.d.group, true, code_bytes, n_cu);
        if (s.grid_x < 1 || s.grid_y < 1) return fail(name, "empty launch");
        if (code_bytes == 0 && s.xcd_q >= 0) return fail(name, "launch order expected");
        if (code_bytes > 0 && s.grid_y > 1 && s.grid_x * s.grid_y >= 8 && s.xcd_q < 0) return fail(name, "grouped launch expected");
        if (check_launch(name, s, t, n_cu, n_sets)) return 1;
        ++*n_launches;
      }
  return 0;
}

static Geometry geometry(int N, int C, int H, int W, int M, int KH, int KW, int ph, int pw, int group) {
  Geometry G{};
  G.d = escoin_conv_desc{N, C, H, W, M, KH, KW, ph, pw, 1, 1, 1, 1, group, 1, 0};
  G.OH = H + 2 * ph - KH + 1;
  G.OW = W + 2 * pw - KW + 1;
  G.Cg = C / group;
  G.Mg = M / group;
  G.kdim = G.Cg * KH * KW;
  return G;
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: touch_election_check <manifest of layout rows>\n"); return 2; }
  // the multiplication of touch_elected against the remainder it replaces, over every rank and stride a launch can have
  for (unsigned T : {1u, 2u, 3u, 5u, 7u, 8u, 16u, 255u, 256u, 257u, 4097u, 65534u, 65535u})
    for (unsigned rank = 0; rank < 65536u; ++rank)
      if (touch_elected(rank, T, touch_mul((int)T)) != (rank % T == 0)) { printf("touch_elected(%u, %u) is wrong\n", rank, T); return 1; }
  int bad = 0, n_rows = 0, n_geoms = 0;
  long n_launches = 0, n_sets = 0;
  std::ifstream in(argv[1]);
  std::string name;
  int N, C, H, W, M, K, pad;
  float sparsity;
  while (in >> name >> N >> C >> H >> W >> M >> K >> pad >> sparsity) {
    const Geometry g = geometry(N, C, H, W, M, K, K, pad, pad, 1);
    const JitLayout lay = jit_layout(g, 1.0f - sparsity, 256, 256);
    if (!lay.ok) { bad += fail(name, "the layout rule refuses the row"); continue; }
    bad += check_geometry(name, g, lay.t, &n_launches, &n_sets);
    ++n_rows;
  }
  // tests/cpp/emulate_tiled.cpp's table
  const Case cases[] = {
      {3, 8, 7, 7, 40, 3, 3, 1, 1, 1, 0.9f, 8, 65536},
      {2, 16, 14, 14, 24, 3, 3, 1, 1, 1, 0.9f, 8, 65536},
      {2, 6, 28, 28, 20, 3, 3, 1, 1, 1, 0.8f, 8, 8192},
      {2, 5, 56, 56, 16, 3, 3, 1, 1, 1, 0.9f, 8, 65536},
      {2, 5, 56, 56, 70, 3, 3, 1, 1, 1, 0.9f, 8, 65536},
      {2, 8, 27, 27, 16, 5, 5, 2, 2, 2, 0.8f, 8, 65536},
      {3, 12, 13, 13, 20, 3, 3, 1, 1, 2, 0.8f, 8, 65536},
      {2, 20, 12, 12, 50, 5, 5, 0, 0, 1, 0.5f, 8, 65536},
      {2, 24, 28, 28, 33, 1, 1, 0, 0, 1, 0.95f, 8, 65536},
      {1, 3, 20, 20, 8, 3, 3, 2, 2, 1, 0.5f, 8, 65536},
      {2, 4, 9, 70, 8, 3, 3, 1, 1, 1, 0.6f, 8, 65536},
      {1, 4, 5, 200, 4, 3, 1, 1, 0, 1, 0.5f, 8, 65536},
      {2, 4, 6, 6, 4, 2, 2, 1, 1, 1, 0.3f, 8, 65536},
      {1, 2, 4, 4, 3, 3, 3, 1, 1, 1, 0.0f, 8, 65536},
      {1, 2, 4, 4, 3, 3, 3, 1, 1, 1, 1.0f, 8, 65536},
      {5, 64, 7, 7, 48, 3, 3, 1, 1, 1, 0.5f, 8, 65536},
      {7, 40, 14, 14, 16, 1, 1, 0, 0, 1, 0.9f, 8, 65536},
      {5, 30, 7, 7, 48, 1, 1, 0, 0, 1, 0.9f, 8, 65536},
      {300, 6, 7, 7, 12, 1, 1, 0, 0, 1, 0.8f, 8, 65536},
      {3, 6, 13, 13, 10, 1, 1, 0, 0, 2, 0.7f, 8, 65536},
      {3, 8, 21, 6, 7, 5, 5, 4, 4, 1, 0.9f, 8, 65536},
      {2, 4, 5, 7, 6, 3, 3, 2, 2, 1, 0.5f, 8, 65536},
      {2, 5, 56, 56, 70, 3, 3, 1, 1, 1, 0.9f, 8, 65536, 256},
      {5, 30, 7, 7, 48, 1, 1, 0, 0, 1, 0.9f, 8, 65536, 256},
      {40, 16, 7, 7, 64, 1, 1, 0, 0, 1, 0.9f, 8, 65536, 8},
      {1, 48, 56, 56, 64, 1, 1, 0, 0, 1, 0.97f, 8, 65536, 256},
      {32, 300, 14, 14, 256, 1, 1, 0, 0, 1, 0.95f, 8, 65536, 32},
      {16, 400, 7, 7, 384, 1, 1, 0, 0, 1, 0.97f, 8, 65536, 16},
      {16, 10, 4, 4, 300, 1, 1, 0, 0, 1, 0.8f, 8, 65536, 16},
      {2, 21, 14, 14, 16, 3, 3, 1, 1, 1, 0.8f, 8, 16384},
      {3, 24, 28, 28, 64, 3, 3, 1, 1, 1, 0.9f, 8, 16384},
      {5, 33, 14, 14, 32, 1, 1, 0, 0, 1, 0.9f, 8, 8192},
      {4, 45, 7, 7, 24, 3, 3, 1, 1, 1, 0.85f, 8, 8192},
      {3, 20, 56, 56, 8, 3, 3, 1, 1, 1, 0.9f, 8, 32768},
      {9, 37, 7, 7, 64, 1, 1, 0, 0, 1, 0.9f, 8, 4096, 256},
      {4, 48, 28, 28, 64, 1, 1, 0, 0, 1, 0.95f, 4, 32768, 4},
      {3, 40, 28, 28, 96, 1, 1, 0, 0, 1, 0.9f, 4, 8192, 2},
      {2, 21, 14, 14, 16, 3, 3, 1, 1, 1, 0.8f, 4, 16384},
      {3, 30, 28, 28, 128, 1, 1, 0, 0, 1, 0.9f, 4, 32768, 1},
      {2, 26, 28, 28, 176, 1, 1, 0, 0, 1, 0.93f, 4, 8192, 1},
      {2, 40, 14, 14, 80, 3, 3, 1, 1, 1, 0.9f, 8, 65536, 256, 1},
      {2, 5, 56, 56, 16, 3, 3, 1, 1, 1, 0.9f, 8, 65536, 256, 2},
      {3, 120, 14, 14, 24, 1, 1, 0, 0, 1, 0.95f, 8, 65536, 256, 3},
      {3, 24, 28, 28, 16, 1, 1, 0, 0, 1, 0.95f, 8, 65536, 256, 4},
  };
  for (const Case &cs : cases) {
    char nm[128];
    snprintf(nm, sizeof nm, "N%d C%d %dx%d M%d K%dx%d g%d waves%d lds%d ncu%d", cs.N, cs.C, cs.H, cs.W, cs.M, cs.KH, cs.KW, cs.group, cs.waves, cs.lds, cs.ncu);
    const Geometry G = geometry(cs.N, cs.C, cs.H, cs.W, cs.M, cs.KH, cs.KW, cs.ph, cs.pw, cs.group);
    Tiling t;
    if (cs.product) {
      const JitLayout lay = jit_layout(G, 1.0f - cs.sparsity, 256, 256);
      if (!lay.ok) { bad += fail(nm, "the layout rule refuses the case"); continue; }
      t = lay.t;
    } else {
      ConvGeom g{cs.N, cs.C, cs.H, cs.W, cs.M, cs.KH, cs.KW, cs.ph, cs.pw, cs.group, 0, 0, 0, 0};
      g.OH = G.OH; g.OW = G.OW; g.Cg = G.Cg; g.Mg = G.Mg;
      g.density = 1.0f - cs.sparsity;
      t = choose_tiling(g, cs.waves, cs.lds, cs.ncu, true);
      if (!t.ok) { bad += fail(nm, "tiling rejected"); continue; }
    }
    bad += check_geometry(nm, G, t, &n_launches, &n_sets);
    ++n_geoms;
  }
  printf("rows=%d geometries=%d launches=%ld sets=%ld\n", n_rows, n_geoms, n_launches, n_sets);
  printf(bad ? "FAILED %d case(s)\n" : "all cases OK\n", bad);
  return bad ? 1 : 0;
}
