// tests/cpp/align_rules_check.cpp -- WeightAlign's rules (csrc/align_rules.h) run on the host alone (test code).
//
// Compiled with plain g++ against align_rules.cpp, stream_builder.cpp and jit_codegen.cpp: no HIP header, no device.
// Reads a manifest, one case per line
//   N C H W M KH KW pad_h pad_w stride_h stride_w dil_h dil_w group  kernel conv_mode dense_gate dense_threshold_pct
//   tiling_batch wgrad_kernel is_f64 n_cu  <file of M * C/group * KH * KW float32 weights>
// takes each case through the rules in the order escoin_capi.hip's upload() and sconv_tiled.hip's tiled_build() call
// them (no device step can fail here, so the ladder has no fallback branches) and prints one JSON line per case with
// what escoin_plan_stat / escoin_plan_tiling_info would answer.
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "align_rules.h"

using namespace escoin;

struct Result {
  int kernel_choice = ESCOIN_KERNEL_GENERIC, small_rule = 0, columns = 0, wgrad = ESCOIN_WGRAD_ENTRY;
  long lds_bytes = 0, code_bytes = 0, jit_rows = 0, jit_records = 0, wgrad_lds = 0;
  std::string info, error;
};

static Result run(const Geometry &g, const SplitOptions &o, int wgrad_kernel, bool is_f64, int n_cu, const std::vector<float> &w) {
  Result r;
  // caffe_cpu_sparse_dense2csr per conv group: row-major scan, keep != 0
  const int G = g.d.group;
  CsrIndex rowptr(G), colidx(G);
  CsrValues values(G);
  std::vector<long> nnz_per_group(G);
  long nnz_all = 0;
  for (int grp = 0; grp < G; ++grp) {
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
    nnz_per_group[grp] = (long)colidx[grp].size();
    nnz_all += nnz_per_group[grp];
  }
  // the backward's weight-gradient kernel, as sconv_backward.hip bwd_build asks for it (stat "wgrad_lds_bytes")
  const BwdChoice bc = bwd_choice(g, is_f64, nnz_all, BwdOptions{ESCOIN_KERNEL_AUTO, wgrad_kernel, 0, false}, n_cu);
  if (bc.rc != ESCOIN_OK) { r.error = bc.error; return r; }
  r.wgrad = bc.wgrad;
  r.wgrad_lds = bc.wgrad == ESCOIN_WGRAD_STAGED ? (long)bc.stg.lds_bytes : bc.wgrad == ESCOIN_WGRAD_MFMA ? (long)bc.wgm.lds_bytes : 0;
  if (is_f64) return r;     // a double plan runs the generic kernel
  const GroupSplit split = group_split(dense_groups(g, nnz_per_group, o, n_cu));
  if (split.use_dense) {
    r.kernel_choice = ESCOIN_KERNEL_DENSE;
    return r;
  }
  const bool explicit_tiled = o.kernel == ESCOIN_KERNEL_TILED || o.kernel == ESCOIN_KERNEL_JIT;
  if (!(explicit_tiled || (o.kernel == ESCOIN_KERNEL_AUTO && tiled_supported(g, n_cu)))) return r;
  if (!tiled_supported(g, n_cu)) { r.error = "tiled kernel requested for a geometry it does not support"; return r; }
  // groups that run on the MFMA kernel contribute empty units
  long nnz = 0;
  for (int grp = 0; grp < G; ++grp) {
    if (split.n_dense > 0 && (grp >= 64 || ((split.dense_mask >> grp) & 1ull))) {
      rowptr[grp].assign(g.Mg + 1, 0);
      colidx[grp].clear();
      values[grp].clear();
    }
    nnz += (long)colidx[grp].size();
  }
  const int n_groups_sparse = split.n_dense > 0 ? std::max(1, split.n_sparse) : G;
  const float density = (float)((double)nnz / std::max<double>(1.0, (double)g.Mg * n_groups_sparse * g.kdim));
  if (o.kernel == ESCOIN_KERNEL_JIT || o.kernel == ESCOIN_KERNEL_AUTO) {
    JitLayout lay = jit_layout(g, density, o.tiling_batch, n_cu);
    if (lay.ok) r.small_rule = small_launch_rule(g, o.kernel, split.n_dense, o.tiling_batch, nnz_all, lay.t, lay.jopt.chain.on, n_cu);
    if (r.small_rule == 2) return r;
    jit::Program prog;
    if (lay.ok && jit_generate(g, density, o.tiling_batch, n_cu, &lay, rowptr, colidx, values, &prog)) {
      r.kernel_choice = ESCOIN_KERNEL_JIT;
      r.lds_bytes = (long)lds_bytes_for(lay.t, 0, lay.nbuf, lay.tab_len);
      r.columns = lay.t.n_ocblk;
      r.code_bytes = (long)prog.code.size() * 4;
      r.jit_rows = prog.n_rows;
      r.jit_records = prog.n_records;
      r.info = tiling_info(lay.t, true, lay.nbuf, (size_t)r.lds_bytes, lay.tab_len, prog.chained);
      return r;
    }
    if (o.kernel == ESCOIN_KERNEL_JIT) { r.error = "generated-code kernel requested but the layer does not fit it"; return r; }
  }
  const StreamLayout lay = stream_layout(g, density, o.tiling_batch, n_cu, rowptr, colidx, values);
  if (lay.ok) {
    r.kernel_choice = ESCOIN_KERNEL_TILED;
    r.lds_bytes = (long)lds_bytes_for(lay.t, lay.stage_bytes, lay.nbuf);
    r.columns = lay.t.n_ocblk;
    r.info = tiling_info(lay.t, false, lay.nbuf, (size_t)r.lds_bytes, 0, false);
  } else if (o.kernel == ESCOIN_KERNEL_TILED) {
    r.error = "tiled kernel requested but its weight stream does not fit the LDS budget";
  }
  return r;
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: align_rules_check <manifest>\n"); return 2; }
  std::ifstream in(argv[1]);
  Geometry g;
  escoin_conv_desc &d = g.d;
  SplitOptions o;
  int wgrad_kernel, is_f64, n_cu, n_cases = 0;
  std::string path;
  d.has_bias = d.fuse_relu = 0;
  while (in >> d.N >> d.C >> d.H >> d.W >> d.M >> d.KH >> d.KW >> d.pad_h >> d.pad_w >> d.stride_h >> d.stride_w >> d.dil_h >> d.dil_w >>
         d.group >> o.kernel >> o.conv_mode >> o.dense_gate >> o.dense_threshold_pct >> o.tiling_batch >> wgrad_kernel >> is_f64 >> n_cu >> path) {
    // conv_layer.cpp:16-19
    g.OH = (d.H + 2 * d.pad_h - (d.dil_h * (d.KH - 1) + 1)) / d.stride_h + 1;
    g.OW = (d.W + 2 * d.pad_w - (d.dil_w * (d.KW - 1) + 1)) / d.stride_w + 1;
    g.Cg = d.C / d.group;
    g.Mg = d.M / d.group;
    g.kdim = g.Cg * d.KH * d.KW;
    std::vector<float> w((size_t)d.M * g.kdim);
    FILE *f = fopen(path.c_str(), "rb");
    if (!f || fread(w.data(), 4, w.size(), f) != w.size()) { fprintf(stderr, "%s: short or missing weights\n", path.c_str()); return 2; }
    fclose(f);
    const Result r = run(g, o, wgrad_kernel, is_f64 != 0, n_cu, w);
    printf("{\"case\": %d, \"kernel_choice\": %d, \"tiling_info\": \"%s\", \"small_launch_rule\": %d, \"lds_bytes\": %ld, \"workgroup_columns\": %d, "
           "\"code_bytes\": %ld, \"jit_rows\": %ld, \"jit_records\": %ld, \"wgrad_kernel\": %d, \"wgrad_lds_bytes\": %ld, \"error\": \"%s\"}\n",
           n_cases++, r.kernel_choice, r.info.c_str(), r.small_rule, r.lds_bytes, r.columns, r.code_bytes, r.jit_rows, r.jit_records, r.wgrad,
           r.wgrad_lds, r.error.c_str());
    fflush(stdout);
  }
  return n_cases > 0 ? 0 : 2;
}
