// tests/cpp/s2d_tables_check.cpp -- the host-only side of plan option "s2d": align_rules.h s2d_plan (the serve predicate
// and the inner descriptor) and csr_tables.h s2d_csr (the inner CSR and the entry map), printed for tests/test_s2d_host.py
// to compare with its numpy restatement.  Built with plain g++ against align_rules.cpp and csr_tables.cpp, no ROCm
// include path.
//
//   s2d_tables_check CASEFILE
//   s2d_tables_check --div
// CASEFILE: "N C H W M KH KW pad_h pad_w stride_h stride_w dil_h dil_w group has_bias fuse_relu is_f64", then per conv
// group its rowptr (Mg + 1 ints) and its colidx (rowptr[Mg] ints), whitespace separated.
// Prints: "serves 0|1"; when served "phases PH PW x_floats", "inner N C H W M KH KW pad_h pad_w stride_h stride_w dil_h
// dil_w group has_bias fuse_relu", "rowptr ..." (group * (Mg + 1), group-relative), "colidx ...", "nnz_g ...", "src ...".
#include <cstdio>
#include <cstdlib>
#include <string>
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

// "--div": the pack / unpack kernels' division by multiplication against the machine's, for every divisor up to 4096
// and a spread of larger ones, on numerators at both ends of [0, 2^31), around every multiple boundary near them and on
// a pseudo-random spread; and the lanes-per-row rule.  Prints "div OK <checked>" or the first mismatch.
static int check_div() {
  long checked = 0;
  unsigned rng = 12345u;
  auto one = [&](unsigned d, unsigned n) {
    ++checked;
    if (s2d_div(n, s2d_div_make(d)) == n / d) return true;
    printf("div MISMATCH d=%u n=%u got %u want %u\n", d, n, s2d_div(n, s2d_div_make(d)), n / d);
    return false;
  };
  std::vector<unsigned> ds;
  for (unsigned d = 1; d <= 4096; ++d) ds.push_back(d);
  for (unsigned k = 13; k < 31; ++k) ds.push_back((1u << k) - 1), ds.push_back(1u << k), ds.push_back((1u << k) + 1);
  ds.push_back(0x7fffffffu);
  const unsigned top = 0x7fffffffu;
  for (unsigned d : ds) {
    for (unsigned n = 0; n < 3 * d + 3 && n <= top && n < 20000; ++n)
      if (!one(d, n)) return 1;
    const unsigned q = top / d;
    for (unsigned back = 0; back < 3; ++back) {
      if (q < back) break;
      const unsigned long long m = (unsigned long long)(q - back) * d;
      for (int off = -2; off <= 2; ++off) {
        const long long n = (long long)m + off;
        if (n >= 0 && n <= (long long)top && !one(d, (unsigned)n)) return 1;
      }
    }
    for (int k = 0; k < 64; ++k) {
      rng = rng * 1664525u + 1013904223u;
      if (!one(d, rng & top)) return 1;
    }
    if (!one(d, top)) return 1;
  }
  for (unsigned span = 1; span <= 300; ++span) {
    const unsigned k = s2d_lane_shift(span);
    const bool ok = k <= 6 && ((1u << k) >= span || k == 6) && (k == 0 || (1u << (k - 1)) < span);
    if (!ok) {
      printf("lane_shift MISMATCH span=%u got %u\n", span, k);
      return 1;
    }
  }
  printf("div OK %ld\n", checked);
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  if (std::string(argv[1]) == "--div") return check_div();
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  Geometry g = {};
  escoin_conv_desc &d = g.d;
  d.N = next_int(f); d.C = next_int(f); d.H = next_int(f); d.W = next_int(f); d.M = next_int(f);
  d.KH = next_int(f); d.KW = next_int(f); d.pad_h = next_int(f); d.pad_w = next_int(f);
  d.stride_h = next_int(f); d.stride_w = next_int(f); d.dil_h = next_int(f); d.dil_w = next_int(f);
  d.group = next_int(f); d.has_bias = next_int(f); d.fuse_relu = next_int(f);
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
  S2dPlan sp;
  const bool serves = s2d_plan(g, is_f64, &sp);
  printf("serves %d\n", serves ? 1 : 0);
  if (!serves) return 0;
  printf("phases %d %d %ld\n", sp.PH, sp.PW, sp.x_floats);
  const escoin_conv_desc &in = sp.inner;
  printf("inner %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", in.N, in.C, in.H, in.W, in.M, in.KH, in.KW, in.pad_h, in.pad_w,
         in.stride_h, in.stride_w, in.dil_h, in.dil_w, in.group, in.has_bias, in.fuse_relu);
  const DerivedCsr t = s2d_csr(CsrView{&g, &rowptr, &colidx}, sp);
  print_row("rowptr", t.rowptr);
  print_row("colidx", t.colidx);
  print_row("nnz_g", t.nnz_g);
  print_row("src", t.src);
  return 0;
}
