// tests/cpp/dgrad_bf16_rule_check.cpp -- align_rules.h dgb_plan, printed for tests/test_dgrad_bf16_host.py (test code; plain
// g++, no ROCm include path).  Arguments: N C H W M KH KW pad_h pad_w stride_h stride_w dil_h dil_w group is_f64.
// Prints "plan serves lds_bytes phases ctiles cols_total tiles_max".
#include <cstdio>
#include <cstdlib>

#include "align_rules.h"

using namespace escoin;

int main(int argc, char **argv) {
  if (argc != 16) return 2;
  int v[15];
  for (int i = 0; i < 15; ++i) v[i] = atoi(argv[i + 1]);
  Geometry g = {};
  escoin_conv_desc &d = g.d;
  d.N = v[0]; d.C = v[1]; d.H = v[2]; d.W = v[3]; d.M = v[4]; d.KH = v[5]; d.KW = v[6]; d.pad_h = v[7]; d.pad_w = v[8];
  d.stride_h = v[9]; d.stride_w = v[10]; d.dil_h = v[11]; d.dil_w = v[12]; d.group = v[13];
  g.OH = (d.H + 2 * d.pad_h - (d.dil_h * (d.KH - 1) + 1)) / d.stride_h + 1;
  g.OW = (d.W + 2 * d.pad_w - (d.dil_w * (d.KW - 1) + 1)) / d.stride_w + 1;
  g.Cg = d.C / d.group; g.Mg = d.M / d.group; g.kdim = g.Cg * d.KH * d.KW;
  DgmPlan p;
  const bool ok = dgb_plan(g, v[14] != 0, &p);
  printf("plan %d %zu %d %d %ld %ld\n", ok ? 1 : 0, p.lds_bytes, p.phases_h * p.phases_w, p.ctiles, p.cols_total, p.tiles_max);
  return 0;
}
