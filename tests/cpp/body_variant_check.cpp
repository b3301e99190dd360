// tests/cpp/body_variant_check.cpp -- which compiled body a plan's launches run (csrc/align_rules.h body_variant), on
// the host alone (test code).
//
// Compiled with plain g++ against align_rules.cpp, stream_builder.cpp and jit_codegen.cpp: no HIP header, no device.
// Reads align_rules_check.cpp's manifest (one case per line, the options kernel / tiling_batch and n_cu are used),
// takes each case to its layout the way sconv_tiled.hip's tiled_build does, sizes the launch of the full batch with
// tiled_launch_shape, as launch_tiled_once does, and prints one JSON line per case: the layout's tiling_info and the rule's answer.
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "align_rules.h"

using namespace escoin;

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: body_variant_check <manifest>\n"); return 2; }
  std::ifstream in(argv[1]);
  Geometry g;
  escoin_conv_desc &d = g.d;
  SplitOptions o;
  int wgrad_kernel, is_f64, n_cu, n_cases = 0;
  std::string path;
  d.has_bias = d.fuse_relu = 0;
  while (in >> d.N >> d.C >> d.H >> d.W >> d.M >> d.KH >> d.KW >> d.pad_h >> d.pad_w >> d.stride_h >> d.stride_w >> d.dil_h >> d.dil_w >>
         d.group >> o.kernel >> o.conv_mode >> o.dense_gate >> o.dense_threshold_pct >> o.tiling_batch >> wgrad_kernel >> is_f64 >> n_cu >> path) {
    g.OH = (d.H + 2 * d.pad_h - (d.dil_h * (d.KH - 1) + 1)) / d.stride_h + 1;
    g.OW = (d.W + 2 * d.pad_w - (d.dil_w * (d.KW - 1) + 1)) / d.stride_w + 1;
    g.Cg = d.C / d.group;
    g.Mg = d.M / d.group;
    g.kdim = g.Cg * d.KH * d.KW;
    std::vector<float> w((size_t)d.M * g.kdim);
    FILE *f = fopen(path.c_str(), "rb");
    if (!f || fread(w.data(), 4, w.size(), f) != w.size()) { fprintf(stderr, "%s: short or missing weights\n", path.c_str()); return 2; }
    fclose(f);
    CsrIndex rowptr(d.group), colidx(d.group);
    CsrValues values(d.group);
    long nnz = 0;
    for (int grp = 0; grp < d.group; ++grp) {
      rowptr[grp].assign(g.Mg + 1, 0);
      const float *A = w.data() + (size_t)grp * g.Mg * g.kdim;
      for (int i = 0; i < g.Mg; ++i) {
        for (int j = 0; j < g.kdim; ++j)
          if (A[(size_t)i * g.kdim + j] != 0) {
            values[grp].push_back(A[(size_t)i * g.kdim + j]);
            colidx[grp].push_back(j);
          }
        rowptr[grp][i + 1] = (int)colidx[grp].size();
      }
      nnz += (long)colidx[grp].size();
    }
    const float density = (float)((double)nnz / std::max<double>(1.0, (double)d.M * g.kdim));
    BodyLaunch bl;
    Tiling t;
    std::string info = "(no tiled layout)";
    jit::Program prog;
    JitLayout lay;
    if (o.kernel != ESCOIN_KERNEL_TILED) lay = jit_layout(g, density, o.tiling_batch, n_cu);
    if (lay.ok && jit_generate(g, density, o.tiling_batch, n_cu, &lay, rowptr, colidx, values, &prog)) {
      t = lay.t;
      bl.jit = true; bl.chained = prog.chained; bl.dma_in_code = lay.tab_len > 0;
      info = tiling_info(t, true, lay.nbuf, lds_bytes_for(t, 0, lay.nbuf, lay.tab_len), lay.tab_len, prog.chained);
    } else {
      const StreamLayout sl = stream_layout(g, density, o.tiling_batch, n_cu, rowptr, colidx, values);
      if (sl.ok) {
        t = sl.t;
        bl.stage_bytes = sl.stage_bytes;
        info = tiling_info(t, false, sl.nbuf, lds_bytes_for(t, sl.stage_bytes, sl.nbuf), 0, false);
      }
    }
    int variant = 0;
    if (t.ok) {
      // the launch of the full batch, every conv group sparse (the XCD grouping does not enter the rule: no code size)
      const TiledLaunchShape ls = tiled_launch_shape(g, t, d.N, d.group, bl.jit, 0, n_cu);
      bl.strided = strided_pointwise(g);
      bl.epi_store = ls.epi_store;
      bl.workgroups = (long)ls.grid_x * ls.grid_y;
      variant = body_variant(g, t, bl, -1);
      if (body_variant(g, t, bl, 0) != 0) { fprintf(stderr, "option 0 must give the generic body\n"); return 2; }
    }
    printf("{\"case\": %d, \"body_variant\": %d, \"tiling_info\": \"%s\"}\n", n_cases++, variant, info.c_str());
    fflush(stdout);
  }
  return n_cases > 0 ? 0 : 2;
}
