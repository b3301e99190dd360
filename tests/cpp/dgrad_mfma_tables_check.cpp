// tests/cpp/dgrad_mfma_tables_check.cpp -- the host-only side of the MFMA data-gradient kernel: align_rules.h dgm_plan
// (the serve predicate and the tile plan) and csr_tables.h dgrad_mfma_tables (the phases, their taps, the column decode,
// each entry's place in the phase matrices, the live-step lists), printed for tests/test_dgrad_mfma_host.py to compare
// with its numpy restatement.  Built with plain g++ against align_rules.cpp and csr_tables.cpp, no ROCm include path.
//
//   dgrad_mfma_tables_check CASEFILE
// CASEFILE: "N C H W M KH KW pad_h pad_w stride_h stride_w dil_h dil_w group is_f64", then per conv group its rowptr
// (Mg + 1 ints) and its colidx (rowptr[Mg] ints), whitespace separated.
// Prints: "serves 0|1"; when served "plan tile_c tile_p step_k phases_h phases_w ctiles tiles_max cols_total mat_floats
// lds_bytes lds_budget", "tiles ..." (per phase, the full batch), "phase ...", "tap_ptr ...", "taps ...", "col ...",
// "pos ...", "live_ptr ...", "live ...".
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
  DgmPlan dp;
  const bool serves = dgm_plan(g, is_f64, &dp);
  printf("serves %d\n", serves ? 1 : 0);
  if (!serves) return 0;
  printf("plan %d %d %d %d %d %d %ld %ld %ld %zu %zu\n", dp.tile_c, dp.tile_p, dp.step_k, dp.phases_h, dp.phases_w, dp.ctiles,
         dp.tiles_max, dp.cols_total, dp.mat_floats, dp.lds_bytes, kDgmLdsBudget);
  printf("tiles");
  for (const DgmPhase &ph : dp.phase) printf(" %ld", ph.tiles);
  printf("\n");
  const DgmTables t = dgrad_mfma_tables(CsrView{&g, &rowptr, &colidx}, dp);
  print_row("phase", t.phase);
  print_row("tap_ptr", t.tap_ptr);
  print_row("taps", t.taps);
  print_row("col", t.col);
  print_row("pos", t.pos);
  print_row("live_ptr", t.live_ptr);
  print_row("live", t.live);
  return 0;
}
