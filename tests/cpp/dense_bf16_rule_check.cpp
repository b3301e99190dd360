// tests/cpp/dense_bf16_rule_check.cpp -- align_rules.h db16_plan, printed for tests/test_dense_bf16_host.py (test code; plain
// g++, no ROCm include path).  Arguments: N C H W M KH KW pad_h pad_w stride_h stride_w dil_h dil_w group is_f64 n_images
// groups n_cu.  Prints "plan rc bm n_ptiles n_mtiles ksteps tiles workgroups".
#include <cstdio>
#include <cstdlib>

#include "align_rules.h"

using namespace escoin;

int main(int argc, char **argv) {
  if (argc != 19) return 2;
  int v[18];
  for (int i = 0; i < 18; ++i) v[i] = atoi(argv[i + 1]);
  Geometry g = {};
  escoin_conv_desc &d = g.d;
  d.N = v[0]; d.C = v[1]; d.H = v[2]; d.W = v[3]; d.M = v[4]; d.KH = v[5]; d.KW = v[6]; d.pad_h = v[7]; d.pad_w = v[8];
  d.stride_h = v[9]; d.stride_w = v[10]; d.dil_h = v[11]; d.dil_w = v[12]; d.group = v[13];
  g.OH = (d.H + 2 * d.pad_h - (d.dil_h * (d.KH - 1) + 1)) / d.stride_h + 1;
  g.OW = (d.W + 2 * d.pad_w - (d.dil_w * (d.KW - 1) + 1)) / d.stride_w + 1;
  g.Cg = d.C / d.group; g.Mg = d.M / d.group; g.kdim = g.Cg * d.KH * d.KW;
  Db16Plan p;
  const LaunchVerdict r = db16_plan(g, v[14] != 0, v[15], v[16], v[17], &p);
  printf("plan %d %d %d %d %d %ld %ld\n", r.rc, p.bm, p.n_ptiles, p.n_mtiles, p.ksteps, p.tiles, p.workgroups);
  return 0;
}
