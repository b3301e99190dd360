// tests/cpp/wgrad_mfma_tables_check.cpp -- the host-only side of the MFMA weight-gradient kernel: align_rules.h wgm_plan
// (the serve predicate and the tile plan) and csr_tables.h wgrad_mfma_tables (the (row, column) -> entry table, the
// entries per tile, the im2col decode), printed for tests/test_wgrad_mfma_host.py to compare with its numpy
// restatement.  Built with plain g++ against align_rules.cpp and csr_tables.cpp, no ROCm include path.
//
//   wgrad_mfma_tables_check CASEFILE
// CASEFILE: "N C H W M KH KW pad_h pad_w stride_h stride_w dil_h dil_w group is_f64", then per conv group its rowptr
// (Mg + 1 ints) and its colidx (rowptr[Mg] ints), whitespace separated.
// Prints: "serves 0|1"; when served "plan tile_m tile_k mtiles ktiles kpad chunks lds_bytes lds_budget", "ent ...",
// "cnt ...", "ktab ...".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "align_rules.h"
#include "csr_tables.h"

using namespace escoin;

static int next_int(FILE *f) {
  int v = 0;
  if (fscanf(f, "%d", &v) != 1) {
    fprintf(stderr, "short case file\n");
    exit(2);
  }
  return v;
}

static void print_row(const char *name, const std::vector<int> &v) {
  printf("%s", name);
  for (int x : v) printf(" %d", x);
  printf("\n");
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  Geometry g = {};
  escoin_conv_desc &d = g.d;
  d.N = next_int(f); d.C = next_int(f); d.H = next_int(f); d.W = next_int(f); d.M = next_int(f);
  d.KH = next_int(f); d.KW = next_int(f); d.pad_h = next_int(f); d.pad_w = next_int(f);
  d.stride_h = next_int(f); d.stride_w = next_int(f); d.dil_h = next_int(f); d.dil_w = next_int(f);
  d.group = next_int(f);
  const bool is_f64 = next_int(f) != 0;
  g.OH = (d.H + 2 * d.pad_h - (d.dil_h * (d.KH - 1) + 1)) / d.stride_h + 1;
  g.OW = (d.W + 2 * d.pad_w - (d.dil_w * (d.KW - 1) + 1)) / d.stride_w + 1;
  g.Cg = d.C / d.group;
  g.Mg = d.M / d.group;
  g.kdim = g.Cg * d.KH * d.KW;
  std::vector<std::vector<int>> rowptr(d.group), colidx(d.group);
  for (int grp = 0; grp < d.group; ++grp) {
    for (int m = 0; m <= g.Mg; ++m) rowptr[grp].push_back(next_int(f));
    for (int j = 0; j < rowptr[grp][g.Mg]; ++j) colidx[grp].push_back(next_int(f));
  }
  fclose(f);
  WgmPlan wp;
  const bool serves = wgm_plan(g, is_f64, &wp);
  printf("serves %d\n", serves ? 1 : 0);
  if (!serves) return 0;
  printf("plan %d %d %d %d %d %d %zu %zu\n", wp.tile_m, wp.tile_k, wp.mtiles, wp.ktiles, wp.kpad, wp.chunks, wp.lds_bytes,
         kWgmLdsBudget);
  const WgmTables t = wgrad_mfma_tables(CsrView{&g, &rowptr, &colidx}, wp.tile_m, wp.tile_k);
  print_row("ent", t.ent);
  print_row("cnt", t.tile_cnt);
  print_row("ktab", t.ktab);
  return 0;
}
