// tests/cpp/d2s_tables_check.cpp -- the host-only side of plan option "deconv": align_rules.h d2s_plan (the serve predicate
// with its refusals, the inner descriptor, the mirror convolution, the scratch and launch sizes) and csr_tables.h d2s_csr (the
// inner CSR and the entry map), printed for tests/test_d2s_host.py to compare with its numpy restatement.  Built with plain
// g++ against align_rules.cpp and csr_tables.cpp, no ROCm include path.
//
//   d2s_tables_check CASEFILE
// CASEFILE: the Deconvolution layer "N C H W M KH KW pad_h pad_w stride_h stride_w dil_h dil_w group has_bias fuse_relu is_f64
// with_csr"; with_csr = 1: then per conv group the layer's rowptr (Cg + 1 ints: the rows are the bottom's channels) and its
// colidx (rowptr[Cg] ints), whitespace separated.
// Prints: "serves 0|1"; when refused "error <message>"; when served "top OH OW", "phases sh sw P", "sizes t_floats top_floats
// unpack_rows pack_rows", "inner <16 ints>", "mirror <16 ints>", and with a CSR "rowptr ..." (group * (Mg * P + 1),
// group-relative), "colidx ...", "nnz_g ...", "src ...".
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

static void print_desc(const char *name, const escoin_conv_desc &d) {
  printf("%s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", name, d.N, d.C, d.H, d.W, d.M, d.KH, d.KW, d.pad_h, d.pad_w, d.stride_h,
         d.stride_w, d.dil_h, d.dil_w, d.group, d.has_bias, d.fuse_relu);
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  escoin_conv_desc d = {};
  d.N = next_int(f); d.C = next_int(f); d.H = next_int(f); d.W = next_int(f); d.M = next_int(f);
  d.KH = next_int(f); d.KW = next_int(f); d.pad_h = next_int(f); d.pad_w = next_int(f);
  d.stride_h = next_int(f); d.stride_w = next_int(f); d.dil_h = next_int(f); d.dil_w = next_int(f);
  d.group = next_int(f); d.has_bias = next_int(f); d.fuse_relu = next_int(f);
  const bool is_f64 = next_int(f) != 0;
  const bool with_csr = next_int(f) != 0;
  D2sPlan dp;
  const bool serves = d2s_plan(d, is_f64, &dp);
  printf("serves %d\n", serves ? 1 : 0);
  if (!serves) {
    printf("error %s\n", dp.error);
    fclose(f);
    return 0;
  }
  printf("top %d %d\n", dp.OH, dp.OW);
  printf("phases %d %d %d\n", dp.sh, dp.sw, dp.P);
  printf("sizes %ld %ld %ld %ld\n", dp.t_floats, dp.top_floats, dp.unpack_rows, dp.pack_rows);
  print_desc("inner", dp.inner);
  print_desc("mirror", dp.mirror);
  if (with_csr) {
    // the layer's CSR lives in the mirror convolution's geometry
    Geometry g = {};
    g.d = dp.mirror;
    g.OH = d.H; g.OW = d.W;
    g.Cg = dp.mirror.C / d.group;
    g.Mg = dp.mirror.M / d.group;
    g.kdim = g.Cg * d.KH * d.KW;
    std::vector<std::vector<int>> rowptr(d.group), colidx(d.group);
    for (int grp = 0; grp < d.group; ++grp) {
      for (int m = 0; m <= g.Mg; ++m) rowptr[grp].push_back(next_int(f));
      for (int j = 0; j < rowptr[grp][g.Mg]; ++j) colidx[grp].push_back(next_int(f));
    }
    const DerivedCsr t = d2s_csr(CsrView{&g, &rowptr, &colidx}, dp);
    print_row("rowptr", t.rowptr);
    print_row("colidx", t.colidx);
    print_row("nnz_g", t.nnz_g);
    print_row("src", t.src);
  }
  fclose(f);
  return 0;
}
