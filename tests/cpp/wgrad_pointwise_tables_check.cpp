// tests/cpp/wgrad_pointwise_tables_check.cpp -- the host-only side of the pointwise weight-gradient kernel (test code):
// align_rules.h pw_plan (the serve predicate and the tiling), csr_tables.h pw_tables (tiles and items) and bwd_choice
// with option "wgrad_pointwise", printed for tests/test_wgrad_pointwise_host.py to compare with its numpy restatement.
// Built with plain g++ against align_rules.cpp and csr_tables.cpp, no ROCm include path.
//
//   wgrad_pointwise_tables_check tables CASEFILE
// CASEFILE: "N C H W M KH KW pad_h pad_w stride_h stride_w dil_h dil_w group is_f64 channel_block tile_entries n_cu nnz",
// then per conv group its rowptr (Mg + 1 ints) and its colidx (rowptr[Mg] ints), whitespace separated.  nnz < 0: the
// CSR's count; else the count the predicate is asked about (the CSR may then be empty: no tables are built).
// Prints "serves 0|1"; when served "plan step pitch cblk lane_entries tile_cap chunks rows_max chans_max lds_bytes
// lds_budget bias_tiles tiles", "bound ..." (the same line for the tiling that reads no pattern), "btiles ..." (that
// tiling's tiles, six ints each: group, first row, rows, first channel, channels, items), and with a CSR "tile ..." (eight
// ints per tile), "ent ...", "pk ...".
//
//   wgrad_pointwise_tables_check choice MANIFEST
// MANIFEST: tests/cpp/bwd_choice_check.cpp's lines with two more fields, wgrad_pointwise and tile_entries; prints that
// program's JSON lines.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "align_rules.h"
#include "csr_tables.h"

using namespace escoin;

static long next_int(FILE *f) {
  long v = 0;
  if (fscanf(f, "%ld", &v) != 1) {
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

static void derive(Geometry *g) {
  escoin_conv_desc &d = g->d;
  g->OH = (d.H + 2 * d.pad_h - (d.dil_h * (d.KH - 1) + 1)) / d.stride_h + 1;
  g->OW = (d.W + 2 * d.pad_w - (d.dil_w * (d.KW - 1) + 1)) / d.stride_w + 1;
  g->Cg = d.C / d.group;
  g->Mg = d.M / d.group;
  g->kdim = g->Cg * d.KH * d.KW;
}

static void print_plan(const char *name, const PwPlan &p) {
  printf("%s %d %d %d %d %d %d %d %d %zu %zu %d %zu\n", name, p.step, p.pitch, p.cblk, p.lane_entries, p.tile_cap, p.chunks,
         p.rows_max, p.chans_max, p.lds_bytes, kPwLdsBudget, p.bias_tiles, p.tiles.size());
}

static int tables(const char *path) {
  FILE *f = fopen(path, "r");
  if (!f) return 2;
  Geometry g = {};
  escoin_conv_desc &d = g.d;
  d.N = (int)next_int(f); d.C = (int)next_int(f); d.H = (int)next_int(f); d.W = (int)next_int(f); d.M = (int)next_int(f);
  d.KH = (int)next_int(f); d.KW = (int)next_int(f); d.pad_h = (int)next_int(f); d.pad_w = (int)next_int(f);
  d.stride_h = (int)next_int(f); d.stride_w = (int)next_int(f); d.dil_h = (int)next_int(f); d.dil_w = (int)next_int(f);
  d.group = (int)next_int(f);
  const bool is_f64 = next_int(f) != 0;
  const int block = (int)next_int(f), tile_entries = (int)next_int(f), n_cu = (int)next_int(f);
  const long nnz_asked = next_int(f);
  derive(&g);
  std::vector<std::vector<int>> rowptr(d.group), colidx(d.group);
  long nnz = 0;
  if (nnz_asked < 0) {
    for (int grp = 0; grp < d.group; ++grp) {
      for (int m = 0; m <= g.Mg; ++m) rowptr[grp].push_back((int)next_int(f));
      for (int j = 0; j < rowptr[grp][g.Mg]; ++j) colidx[grp].push_back((int)next_int(f));
      nnz += (long)colidx[grp].size();
    }
  }
  fclose(f);
  PwPlan bound, pp;
  const bool serves = pw_plan(g, is_f64, nnz_asked < 0 ? nnz : nnz_asked, nullptr, nullptr, block, tile_entries, n_cu, &bound);
  printf("serves %d\n", serves ? 1 : 0);
  if (!serves || nnz_asked >= 0) return 0;
  if (!pw_plan(g, is_f64, nnz, &rowptr, &colidx, block, tile_entries, n_cu, &pp)) return 3;   // the predicate reads no pattern
  print_plan("plan", pp);
  print_plan("bound", bound);
  std::vector<int> bt;
  for (const PwTile &t : bound.tiles) {
    const int w[6] = {t.grp, t.row0, t.rows, t.c0, t.chans, t.items};
    bt.insert(bt.end(), w, w + 6);
  }
  print_row("btiles", bt);
  const PwTables t = pw_tables(CsrView{&g, &rowptr, &colidx}, pp);
  // the plan's own item counts are the tables'
  for (size_t k = 0; k < pp.tiles.size(); ++k)
    if (t.tile[k * kPwTileWords + 6] != pp.tiles[k].items) return 4;
  print_row("tile", t.tile);
  print_row("ent", t.ent);
  print_row("pk", t.pk);
  return 0;
}

static int choice(const char *path) {
  std::ifstream in(path);
  static const char *const kPath[] = {"inner", "transposed", "gather", "mfma"};
  Geometry g;
  escoin_conv_desc &d = g.d;
  BwdOptions o;
  int s2d, is_f64, n_cu, n_cases = 0;
  long nnz;
  d.has_bias = d.fuse_relu = 0;
  while (in >> d.N >> d.C >> d.H >> d.W >> d.M >> d.KH >> d.KW >> d.pad_h >> d.pad_w >> d.stride_h >> d.stride_w >> d.dil_h >> d.dil_w >>
         d.group >> o.backward_kernel >> o.wgrad_kernel >> o.wgrad_channel_block >> s2d >> is_f64 >> nnz >> n_cu >> o.wgrad_pointwise >>
         o.pw_tile_entries) {
    derive(&g);
    o.s2d = s2d != 0;
    const BwdChoice c = bwd_choice(g, is_f64 != 0, nnz, o, n_cu);
    const bool ok = c.rc == ESCOIN_OK;
    const long wgrad_lds = !ok ? 0
                           : c.wgrad == ESCOIN_WGRAD_STAGED ? (long)c.stg.lds_bytes
                           : c.wgrad == ESCOIN_WGRAD_MFMA ? (long)c.wgm.lds_bytes
                           : c.wgrad == ESCOIN_WGRAD_POINTWISE ? (long)c.pw.lds_bytes : 0;
    printf("{\"case\": %d, \"rc\": %d, \"error\": \"%s\", \"data\": \"%s\", \"wgrad_kernel\": %d, \"wgrad_lds_bytes\": %ld, "
           "\"dgrad_lds_bytes\": %ld, \"chunks_max\": %d}\n",
           n_cases++, c.rc, c.error, ok ? kPath[c.data] : "", ok ? c.wgrad : 0, wgrad_lds,
           ok && c.data == kBwdMfma ? (long)c.dgm.lds_bytes : 0, ok ? c.chunks_max : 0);
  }
  return n_cases > 0 ? 0 : 2;
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  if (!strcmp(argv[1], "tables")) return tables(argv[2]);
  if (!strcmp(argv[1], "choice")) return choice(argv[2]);
  return 2;
}
