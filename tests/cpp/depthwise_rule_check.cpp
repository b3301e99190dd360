// tests/cpp/depthwise_rule_check.cpp -- align_rules.h dw_plan and bwd_choice with option "depthwise", printed for
// tests/test_depthwise_host.py (test code).  Built with plain g++ against align_rules.cpp, no ROCm include path.
//   depthwise_rule_check N C H W M KH KW pad_h pad_w stride_h stride_w dil_h dil_w group is_f64 band_rows n_cu
// Prints "served 0|1"; when served the plan's fields, per forward band "fwd o0 o1 first_row rows" (dw_window), per bottom band
// "bwd h0 h1 first_top_row rows" (dw_top_rows); then bwd_choice's data path with the option off / on under AUTO, on under
// GENERIC, on under BWD_MFMA, on under AUTO with an inner plan.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "align_rules.h"

using namespace escoin;

int main(int argc, char **argv) {
  if (argc != 18) return 2;
  int v[17];
  for (int i = 0; i < 17; ++i) v[i] = atoi(argv[i + 1]);
  Geometry g = {};
  escoin_conv_desc &d = g.d;
  d.N = v[0]; d.C = v[1]; d.H = v[2]; d.W = v[3]; d.M = v[4]; d.KH = v[5]; d.KW = v[6]; d.pad_h = v[7]; d.pad_w = v[8];
  d.stride_h = v[9]; d.stride_w = v[10]; d.dil_h = v[11]; d.dil_w = v[12]; d.group = v[13];
  const bool f64 = v[14] != 0;
  const int band_rows = v[15], n_cu = v[16];
  g.OH = (d.H + 2 * d.pad_h - (d.dil_h * (d.KH - 1) + 1)) / d.stride_h + 1;
  g.OW = (d.W + 2 * d.pad_w - (d.dil_w * (d.KW - 1) + 1)) / d.stride_w + 1;
  g.Cg = d.C / d.group; g.Mg = d.M / d.group; g.kdim = g.Cg * d.KH * d.KW;
  DwPlan p;
  const bool served = dw_plan(g, f64, band_rows, n_cu, &p);
  printf("served %d\n", served ? 1 : 0);
  if (served) {
    printf("plan %d %d %d %d %d %d %zu %ld %d %d %d %d %d %zu %ld\n", p.band, p.nbands, p.px, p.rows, p.padl, p.pitch, p.lds_bytes, p.units,
           p.dband, p.dnbands, p.dpx, p.drows, p.dpitch, p.dlds_bytes, p.dunits);
    int first, rows;
    for (int b = 0; b < p.nbands; ++b) {
      dw_window(d, b * p.band, std::min(g.OH, (b + 1) * p.band), &first, &rows);
      printf("fwd %d %d %d %d\n", b * p.band, std::min(g.OH, (b + 1) * p.band), first, rows);
    }
    for (int b = 0; b < p.dnbands; ++b) {
      dw_top_rows(d, g.OH, b * p.dband, std::min(d.H, (b + 1) * p.dband), &first, &rows);
      printf("bwd %d %d %d %d\n", b * p.dband, std::min(d.H, (b + 1) * p.dband), first, rows);
    }
  }
  auto path = [&](int on, int kernel, bool inner) {
    BwdOptions o{kernel, ESCOIN_WGRAD_AUTO, 0, inner};
    o.depthwise = on;
    o.dw_band_rows = band_rows;
    const BwdChoice c = bwd_choice(g, f64, (long)d.M * g.kdim, o, n_cu);
    return c.rc == ESCOIN_OK ? (int)c.data : -1;
  };
  printf("choice %d %d %d %d %d\n", path(0, ESCOIN_KERNEL_AUTO, false), path(1, ESCOIN_KERNEL_AUTO, false),
         path(1, ESCOIN_KERNEL_GENERIC, false), path(1, ESCOIN_BWD_MFMA, false), path(1, ESCOIN_KERNEL_AUTO, true));
  return 0;
}
