// tests/cpp/sp24_rule_check.cpp -- align_rules.h sp24_plan and csr_tables.h sp24_index, printed for tests/test_sp24_host.py
// (test code; plain g++, no ROCm include path).  Arguments: N C H W M KH KW pad_h pad_w stride_h stride_w dil_h dil_w group
// is_f64 n_images groups n_cu, then the CSR of every conv group in turn: Mg row lengths followed by the row's columns.
// Prints "plan rc bm n_ptiles n_mtiles ksteps tiles workgroups idx_rows idx_row_words idx_bytes", then "index ok" and the
// table's words.
#include <cstdio>
#include <cstdlib>

#include "align_rules.h"
#include "csr_tables.h"

using namespace escoin;

int main(int argc, char **argv) {
  if (argc < 19) return 2;
  int v[18];
  for (int i = 0; i < 18; ++i) v[i] = atoi(argv[i + 1]);
  Geometry g = {};
  escoin_conv_desc &d = g.d;
  d.N = v[0]; d.C = v[1]; d.H = v[2]; d.W = v[3]; d.M = v[4]; d.KH = v[5]; d.KW = v[6]; d.pad_h = v[7]; d.pad_w = v[8];
  d.stride_h = v[9]; d.stride_w = v[10]; d.dil_h = v[11]; d.dil_w = v[12]; d.group = v[13];
  g.OH = (d.H + 2 * d.pad_h - (d.dil_h * (d.KH - 1) + 1)) / d.stride_h + 1;
  g.OW = (d.W + 2 * d.pad_w - (d.dil_w * (d.KW - 1) + 1)) / d.stride_w + 1;
  g.Cg = d.C / d.group; g.Mg = d.M / d.group; g.kdim = g.Cg * d.KH * d.KW;
  Sp24Plan p;
  const LaunchVerdict r = sp24_plan(g, v[14] != 0, v[15], v[16], v[17], &p);
  printf("plan %d %d %d %d %d %ld %ld %d %d %llu\n", r.rc, p.t.bm, p.t.n_ptiles, p.t.n_mtiles, p.t.ksteps, p.t.tiles, p.t.workgroups,
         p.idx_rows, p.idx_row_words, p.idx_bytes);
  if (argc == 19 || !r.ok()) return 0;
  std::vector<std::vector<int>> rowptr(d.group), colidx(d.group);
  int at = 19;
  for (int grp = 0; grp < d.group; ++grp) {
    rowptr[grp].push_back(0);
    for (int m = 0; m < g.Mg; ++m) {
      if (at >= argc) return 2;
      const int n = atoi(argv[at++]);
      for (int j = 0; j < n && at < argc; ++j) colidx[grp].push_back(atoi(argv[at++]));
      rowptr[grp].push_back((int)colidx[grp].size());
    }
  }
  const Sp24Index t = sp24_index(CsrView{&g, &rowptr, &colidx}, p.idx_rows, p.idx_row_words * 16);
  printf("index %d", t.ok ? 1 : 0);
  for (unsigned short w : t.idx) printf(" %u", (unsigned)w);
  printf("\n");
  return 0;
}
