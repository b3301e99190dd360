// tests/cpp/dense_wgrad_plan_check.cpp -- the host-only side of the dense weight gradient: align_rules.h dwg_plan (the
// serve predicate, the tiles and the split of the pixel axis) and csr_tables.h im2col_ktab (the column decode, which must
// equal the ktab of wgrad_mfma_tables element by element), printed for tests/test_dense_wgrad_host.py to compare with its
// numpy restatement.  Built with plain g++ against align_rules.cpp and csr_tables.cpp, no ROCm include path.
//
//   dense_wgrad_plan_check CASEFILE
// CASEFILE: lines of "N C H W M KH KW pad_h pad_w stride_h stride_w dil_h dil_w group is_f64 n_cu max_splits".
// Prints per line: "serves 0|1"; when served "plan mtiles ktiles chunks span splits positions slab_bytes lds_bytes",
// "cover min max" (how often the spans [s * span, min((s + 1) * span, chunks)) cover a chunk: the least and the most
// covered chunk), "empty n" (spans without a chunk) and "ktab_equal 0|1 len".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "align_rules.h"
#include "csr_tables.h"

using namespace escoin;

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  int v[17];
  for (;;) {
    int got = 0;
    for (; got < 17; ++got)
      if (fscanf(f, "%d", &v[got]) != 1) break;
    if (got == 0) break;
    if (got != 17) {
      fprintf(stderr, "short case line\n");
      return 2;
    }
    Geometry g = {};
    escoin_conv_desc &d = g.d;
    d.N = v[0]; d.C = v[1]; d.H = v[2]; d.W = v[3]; d.M = v[4]; d.KH = v[5]; d.KW = v[6]; d.pad_h = v[7]; d.pad_w = v[8];
    d.stride_h = v[9]; d.stride_w = v[10]; d.dil_h = v[11]; d.dil_w = v[12]; d.group = v[13];
    const bool is_f64 = v[14] != 0;
    const int n_cu = v[15], max_splits = v[16];
    g.OH = (d.H + 2 * d.pad_h - (d.dil_h * (d.KH - 1) + 1)) / d.stride_h + 1;
    g.OW = (d.W + 2 * d.pad_w - (d.dil_w * (d.KW - 1) + 1)) / d.stride_w + 1;
    g.Cg = d.C / d.group;
    g.Mg = d.M / d.group;
    g.kdim = g.Cg * d.KH * d.KW;
    DwgPlan dp;
    const bool serves = dwg_plan(g, is_f64, n_cu, max_splits, &dp);
    printf("serves %d\n", serves ? 1 : 0);
    if (!serves) continue;
    printf("plan %d %d %d %d %d %ld %zu %zu\n", dp.tile.mtiles, dp.tile.ktiles, dp.tile.chunks, dp.span, dp.splits,
           dp.positions, dp.slab_bytes, dp.tile.lds_bytes);
    std::vector<int> cover((size_t)dp.tile.chunks, 0);
    int empty = 0;
    for (int s = 0; s < dp.splits; ++s) {
      const long lo = (long)s * dp.span, hi = std::min<long>(lo + dp.span, dp.tile.chunks);
      if (lo >= hi) ++empty;
      for (long c = lo; c < hi; ++c) ++cover[(size_t)c];
    }
    printf("cover %d %d\n", *std::min_element(cover.begin(), cover.end()), *std::max_element(cover.begin(), cover.end()));
    printf("empty %d\n", empty);
    // the decode table against the one the sparse-position kernel's tables carry (an empty pattern: ktab does not read it)
    std::vector<std::vector<int>> rowptr(d.group, std::vector<int>((size_t)g.Mg + 1, 0)), colidx(d.group);
    const WgmTables t = wgrad_mfma_tables(CsrView{&g, &rowptr, &colidx}, dp.tile.tile_m, dp.tile.tile_k);
    const std::vector<int> ktab = im2col_ktab(g, dp.tile.tile_k);
    printf("ktab_equal %d %zu\n", ktab == t.ktab ? 1 : 0, ktab.size());
  }
  fclose(f);
  return 0;
}
