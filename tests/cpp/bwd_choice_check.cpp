// tests/cpp/bwd_choice_check.cpp -- the backward's kernel choice (csrc/align_rules.h bwd_choice) run on the host alone
// (test code).
//
// Compiled with plain g++ against align_rules.cpp, stream_builder.cpp and jit_codegen.cpp: no HIP header, no device.
// Reads a manifest, one case per line
//   N C H W M KH KW pad_h pad_w stride_h stride_w dil_h dil_w group  backward_kernel wgrad_kernel wgrad_channel_block s2d
//   is_f64 nnz n_cu
// and prints one JSON line per case: the refusal (rc, error) or what the first escoin_backward builds -- the data path,
// and what the stats "wgrad_kernel", "wgrad_lds_bytes" and "dgrad_lds_bytes" answer after a weight gradient has run (all
// three 0 for a refusal: no state is built).
#include <cstdio>
#include <fstream>

#include "align_rules.h"

using namespace escoin;

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: bwd_choice_check <manifest>\n"); return 2; }
  std::ifstream in(argv[1]);
  static const char *const kPath[] = {"inner", "transposed", "gather", "mfma"};
  Geometry g;
  escoin_conv_desc &d = g.d;
  BwdOptions o;
  int s2d, is_f64, n_cu, n_cases = 0;
  long nnz;
  d.has_bias = d.fuse_relu = 0;
  while (in >> d.N >> d.C >> d.H >> d.W >> d.M >> d.KH >> d.KW >> d.pad_h >> d.pad_w >> d.stride_h >> d.stride_w >> d.dil_h >> d.dil_w >>
         d.group >> o.backward_kernel >> o.wgrad_kernel >> o.wgrad_channel_block >> s2d >> is_f64 >> nnz >> n_cu) {
    // conv_layer.cpp:16-19
    g.OH = (d.H + 2 * d.pad_h - (d.dil_h * (d.KH - 1) + 1)) / d.stride_h + 1;
    g.OW = (d.W + 2 * d.pad_w - (d.dil_w * (d.KW - 1) + 1)) / d.stride_w + 1;
    g.Cg = d.C / d.group;
    g.Mg = d.M / d.group;
    g.kdim = g.Cg * d.KH * d.KW;
    o.s2d = s2d != 0;
    const BwdChoice c = bwd_choice(g, is_f64 != 0, nnz, o, n_cu);
    const bool ok = c.rc == ESCOIN_OK;
    const long wgrad_lds = !ok ? 0 : c.wgrad == ESCOIN_WGRAD_STAGED ? (long)c.stg.lds_bytes : c.wgrad == ESCOIN_WGRAD_MFMA ? (long)c.wgm.lds_bytes : 0;
    printf("{\"case\": %d, \"rc\": %d, \"error\": \"%s\", \"data\": \"%s\", \"wgrad_kernel\": %d, \"wgrad_lds_bytes\": %ld, "
           "\"dgrad_lds_bytes\": %ld, \"chunks_max\": %d}\n",
           n_cases++, c.rc, c.error, ok ? kPath[c.data] : "", ok ? c.wgrad : 0, wgrad_lds,
           ok && c.data == kBwdMfma ? (long)c.dgm.lds_bytes : 0, ok ? c.chunks_max : 0);
  }
  return n_cases > 0 ? 0 : 2;
}
