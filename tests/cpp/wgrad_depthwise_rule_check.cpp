// tests/cpp/wgrad_depthwise_rule_check.cpp -- align_rules.h dww_plan, bwd_choice with option "wgrad_depthwise" and csr_tables.h
// dww_segments, printed for tests/test_wgrad_depthwise_host.py (test code; plain g++, no ROCm include path).  Arguments: N C H W
// M KH KW pad_h pad_w stride_h stride_w dil_h dil_w group is_f64 band_rows slices n_cu n_images row_len -- every row of the
// pattern has row_len entries, except row 0, which is empty.  "choice": wgrad * 10^6 + slab rows with the option off / on / on
// under a forced ENTRY / on with "wgrad_pointwise" too; "refused": nnz = 2^31, 2^31 segments, a grid past its axis.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "align_rules.h"
#include "csr_tables.h"

using namespace escoin;

int main(int argc, char **argv) {
  if (argc != 21) return 2;
  int v[20];
  for (int i = 0; i < 20; ++i) v[i] = atoi(argv[i + 1]);
  Geometry g = {};
  escoin_conv_desc &d = g.d;
  d.N = v[0]; d.C = v[1]; d.H = v[2]; d.W = v[3]; d.M = v[4]; d.KH = v[5]; d.KW = v[6]; d.pad_h = v[7]; d.pad_w = v[8];
  d.stride_h = v[9]; d.stride_w = v[10]; d.dil_h = v[11]; d.dil_w = v[12]; d.group = v[13];
  const bool f64 = v[14] != 0;
  const int band_rows = v[15], slices = v[16], n_cu = v[17], n_images = v[18], row_len = v[19];
  g.OH = (d.H + 2 * d.pad_h - (d.dil_h * (d.KH - 1) + 1)) / d.stride_h + 1;
  g.OW = (d.W + 2 * d.pad_w - (d.dil_w * (d.KW - 1) + 1)) / d.stride_w + 1;
  g.Cg = d.C / d.group; g.Mg = d.M / d.group; g.kdim = g.Cg * d.KH * d.KW;
  std::vector<std::vector<int>> rowptr(d.group, std::vector<int>(g.Mg + 1, 0)), colidx(d.group);
  for (int grp = 0; grp < d.group; ++grp)
    for (int m = 0; m < g.Mg; ++m) {
      const int n = grp == 0 && m == 0 ? 0 : row_len;
      colidx[grp].resize(colidx[grp].size() + n, 0);
      rowptr[grp][m + 1] = rowptr[grp][m] + n;
    }
  const CsrView view{&g, &rowptr, &colidx};
  const std::vector<int> seg = dww_segments(view);
  const long nseg = (long)(seg.size() / kDwwSegWords), nnz = view.nnz();
  DwwPlan p, q;
  const bool served = dww_plan(g, f64, nnz, nseg, band_rows, slices, n_cu, &p);
  printf("served %d\n", served ? 1 : 0);
  if (served) printf("plan %d %d %d %d %d %d %d\n", p.band, p.nbands, p.px, p.S, p.per, p.slices(n_images), p.slices(d.N));
  auto choice = [&](int on, int kernel, int pointwise) {
    BwdOptions o{ESCOIN_KERNEL_AUTO, kernel, 0, false};
    o.wgrad_depthwise = on; o.wgrad_pointwise = pointwise; o.dw_band_rows = band_rows; o.dww_slices = slices;
    const BwdChoice c = bwd_choice(g, f64, nnz, o, n_cu);
    return c.rc == ESCOIN_OK ? c.wgrad * 1000000 + c.chunks_max : -1;
  };
  printf("choice %d %d %d %d\n", choice(0, ESCOIN_WGRAD_AUTO, 0), choice(1, ESCOIN_WGRAD_AUTO, 0), choice(1, ESCOIN_WGRAD_ENTRY, 0),
         choice(1, ESCOIN_WGRAD_AUTO, 1));
  printf("refused %d %d %d\n", !dww_plan(g, f64, 1L << 31, nseg, band_rows, slices, n_cu, &q), !dww_plan(g, f64, nnz, 1L << 31, band_rows, slices, n_cu, &q),
         !dww_plan(g, f64, nnz, kDwMaxUnits / (served ? p.S : 1) + 1, band_rows, slices, n_cu, &q));
  for (long i = 0; i < nseg; ++i) printf("seg %d %d %d\n", seg[3 * i], seg[3 * i + 1], seg[3 * i + 2]);
  return 0;
}
