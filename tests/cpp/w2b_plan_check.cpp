// tests/cpp/w2b_plan_check.cpp -- align_rules.h w2b_plan for tests/test_w2b_host.py, built with plain g++ and no ROCm include
// path.  w2b_plan_check CASEFILE: per line the 16 fields of escoin_conv_desc in order, then is_f64 and strip.  Prints per
// case "0", or "1 S SW Wi x_floats t_floats" and the 16 fields of the inner descriptor.
#include <cstdio>
#include <cstring>

#include "align_rules.h"

using namespace escoin;

int main(int argc, char **argv) {
  FILE *f = argc == 2 ? fopen(argv[1], "r") : nullptr;
  static_assert(sizeof(escoin_conv_desc) == 16 * sizeof(int), "the descriptor is 16 ints");
  for (int v[18], n = 0; f && fscanf(f, "%d", &v[n]) == 1;) {
    if (++n < 18) continue;
    n = 0;
    Geometry g = {};
    escoin_conv_desc &d = g.d;
    memcpy(&d, v, sizeof(d));
    g.OH = (d.H + 2 * d.pad_h - (d.dil_h * (d.KH - 1) + 1)) / d.stride_h + 1;
    g.OW = (d.W + 2 * d.pad_w - (d.dil_w * (d.KW - 1) + 1)) / d.stride_w + 1;
    g.Cg = d.C / d.group, g.Mg = d.M / d.group, g.kdim = g.Cg * d.KH * d.KW;
    W2bPlan wp;
    if (!w2b_plan(g, v[16] != 0, v[17], &wp)) {
      printf("0\n");
      continue;
    }
    printf("1 %d %d %d %ld %ld", wp.S, wp.SW, wp.Wi, wp.x_floats, wp.t_floats);
    memcpy(v, &wp.inner, sizeof(wp.inner));
    for (int i = 0; i < 16; ++i) printf(" %d", v[i]);
    printf("\n");
  }
  return f ? 0 : 2;
}
