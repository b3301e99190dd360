// tests/cpp/b2s_plan_check.cpp -- the host-only side of plan option "b2s": align_rules.h b2s_plan (the serve predicate, the
// block, the inner descriptor and the scratch sizes), printed for tests/test_b2s_host.py to compare with its numpy
// restatement.  Built with plain g++ against align_rules.cpp, no ROCm include path.
//
//   b2s_plan_check CASEFILE
// CASEFILE: one case per line, "N C H W M KH KW pad_h pad_w stride_h stride_w dil_h dil_w group has_bias fuse_relu is_f64
// block n_cu".  Prints per case one line: "0", or "1 B x_floats t_floats  N C H W M KH KW pad_h pad_w stride_h stride_w dil_h
// dil_w group has_bias fuse_relu" (the inner descriptor).
#include <cstdio>

#include "align_rules.h"

using namespace escoin;

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  for (;;) {
    Geometry g = {};
    escoin_conv_desc &d = g.d;
    int is_f64 = 0, block = 0, n_cu = 0;
    const int got = fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &d.N, &d.C, &d.H, &d.W, &d.M, &d.KH, &d.KW,
                           &d.pad_h, &d.pad_w, &d.stride_h, &d.stride_w, &d.dil_h, &d.dil_w, &d.group, &d.has_bias, &d.fuse_relu, &is_f64,
                           &block, &n_cu);
    if (got == EOF) break;
    if (got != 19) {
      fprintf(stderr, "short case line\n");
      return 2;
    }
    g.OH = (d.H + 2 * d.pad_h - (d.dil_h * (d.KH - 1) + 1)) / d.stride_h + 1;
    g.OW = (d.W + 2 * d.pad_w - (d.dil_w * (d.KW - 1) + 1)) / d.stride_w + 1;
    g.Cg = d.C / d.group;
    g.Mg = d.M / d.group;
    g.kdim = g.Cg * d.KH * d.KW;
    B2sPlan bp;
    if (!b2s_plan(g, is_f64 != 0, block, n_cu, &bp)) {
      printf("0\n");
      continue;
    }
    const escoin_conv_desc &in = bp.inner;
    printf("1 %d %ld %ld  %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", bp.B, bp.x_floats, bp.t_floats, in.N, in.C, in.H, in.W, in.M,
           in.KH, in.KW, in.pad_h, in.pad_w, in.stride_h, in.stride_w, in.dil_h, in.dil_w, in.group, in.has_bias, in.fuse_relu);
  }
  fclose(f);
  return 0;
}
