// tests/cpp/shim_b2s_selftest.cpp -- InnerProductLayer<Dtype> and Caffe::set_b2s through the C++ shim: one InnerProduct
// layer (a 7 x 3 x 5 x 2 bottom, axis 1: M_ = 7 rows of K_ = 30 inputs; 11 outputs, about half of the weights pruned) runs
// Forward, Backward, SolverUpdate, Forward, Prune and Forward again.  Every element of the tops, the bottom diff and the
// weight and bias diffs lies within the derived bound of a plain float64 loop -- gamma(terms + 4) x the sum of the terms'
// magnitudes, terms = the nonzeros of the output's row (forward), of the input's column (data gradient) or the batch (weight
// and bias gradients), tools/error_bound.py; the weight diff is exactly zero outside the pattern; the solver's new weights
// are w - rate * diff at the pattern and 0 outside it; the prune keeps the asked count and zeroes the blob where it dropped.
//
//   shim_b2s_selftest              Caffe::GPU, float, Caffe::set_b2s(true) and (false): stat "b2s" says which ran (needs a GPU)
//   shim_b2s_selftest --cpu-only   Caffe::CPU, float and double, the setter on: accepted and ignored; touches no device
//   shim_b2s_selftest --transpose  inner_product_param.transpose = true: SetUp aborts with a message that names it
// Prints one line per run, exit code = number of failures.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "caffe_shim.hpp"

using namespace caffe;

static unsigned rng = 11;
static double urand() {   // [-1, 1)
  rng = rng * 1664525u + 1013904223u;
  return ((rng >> 8) & 0xFFFFFF) / 8388608.0 - 1.0;
}

enum { NB = 7, D1 = 3, D2 = 5, D3 = 2, K = D1 * D2 * D3, M = 11 };

static double gam(double k, double u) { return k * u / (1.0 - k * u); }

template <typename Dtype>
struct Check {
  double u, tiny;     // unit roundoff and the smallest subnormal of Dtype
  double worst = 0;
  void add(double got, double want, double mag, double terms) {
    const double bound = gam(terms + 4, u) * mag + (terms + 4) * tiny;
    worst = std::max(worst, std::isfinite(got) ? std::fabs(got - want) / bound : (double)INFINITY);
  }
};

// top = x * w^T + b against the loop; returns the worst error / bound
template <typename Dtype>
static double worst_top(const vector<Dtype> &x, const vector<Dtype> &w, const vector<Dtype> &b, const Dtype *top, double u, double tiny) {
  Check<Dtype> c{u, tiny};
  for (int n = 0; n < NB; ++n)
    for (int m = 0; m < M; ++m) {
      double sum = b[m], mag = std::fabs((double)b[m]);
      int terms = 0;
      for (int k = 0; k < K; ++k) {
        const double t = (double)w[m * K + k] * (double)x[n * K + k];
        sum += t, mag += std::fabs(t), terms += w[m * K + k] != 0;
      }
      c.add(top[n * M + m], sum, mag, terms);
    }
  return c.worst;
}

template <typename Dtype>
static int run(const char *label, bool b2s, bool gpu) {
  const double u = sizeof(Dtype) == 4 ? std::ldexp(1.0, -24) : std::ldexp(1.0, -53);
  const double tiny = sizeof(Dtype) == 4 ? std::ldexp(1.0, -149) : std::ldexp(1.0, -1074);
  Caffe::set_b2s(b2s);
  rng = 11;
  LayerParameter lp;
  lp.name = "ip";
  lp.type = "InnerProduct";
  lp.inner_product_param.num_output = M;
  shared_ptr<Layer<Dtype> > layer = LayerRegistry<Dtype>::CreateLayer(lp);
  vector<int> bshape(4);
  bshape[0] = NB; bshape[1] = D1; bshape[2] = D2; bshape[3] = D3;
  Blob<Dtype> bottom(bshape), top;
  vector<Blob<Dtype> *> bv(1, &bottom), tv(1, &top);
  Dtype *d = bottom.mutable_cpu_data();
  for (int i = 0; i < bottom.count(); ++i) d[i] = (Dtype)urand();
  layer->SetUp(bv, tv);
  bool ok = !strcmp(layer->type(), "InnerProduct") && top.num_axes() == 2 && top.shape(0) == NB && top.shape(1) == M;
  Blob<Dtype> &wb = *layer->blobs()[0];
  Blob<Dtype> &bb = *layer->blobs()[1];
  ok = ok && wb.num_axes() == 2 && wb.shape(0) == M && wb.shape(1) == K && bb.count() == M;
  Dtype *w = wb.mutable_cpu_data();
  for (int i = 0; i < wb.count(); ++i) {
    const Dtype v = (Dtype)(0.1 * urand() + 0.2);
    w[i] = urand() < 0 ? (Dtype)0 : v;                                   // about half pruned
  }
  Dtype *b = bb.mutable_cpu_data();
  for (int i = 0; i < bb.count(); ++i) b[i] = (Dtype)urand();
  const vector<Dtype> x(bottom.cpu_data(), bottom.cpu_data() + bottom.count());
  const vector<Dtype> w0(wb.cpu_data(), wb.cpu_data() + wb.count()), b0(bb.cpu_data(), bb.cpu_data() + bb.count());
  layer->WeightAlign();
  layer->Forward(bv, tv);
  const double f0 = worst_top(x, w0, b0, top.cpu_data(), u, tiny);
  Dtype *tdp = top.mutable_cpu_diff();
  for (int i = 0; i < top.count(); ++i) tdp[i] = (Dtype)urand();
  const vector<Dtype> td(top.cpu_diff(), top.cpu_diff() + top.count());
  memset(wb.mutable_cpu_diff(), 0, sizeof(Dtype) * wb.count());
  memset(bb.mutable_cpu_diff(), 0, sizeof(Dtype) * bb.count());
  Dtype *bd = bottom.mutable_cpu_diff();
  for (int i = 0; i < bottom.count(); ++i) bd[i] = (Dtype)NAN;          // the data gradient overwrites
  layer->Backward(tv, vector<bool>(1, true), bv);
  Check<Dtype> cd{u, tiny}, cw{u, tiny}, cb{u, tiny};
  for (int n = 0; n < NB; ++n)
    for (int k = 0; k < K; ++k) {
      double sum = 0, mag = 0;
      int terms = 0;
      for (int m = 0; m < M; ++m) {
        const double t = (double)w0[m * K + k] * (double)td[n * M + m];
        sum += t, mag += std::fabs(t), terms += w0[m * K + k] != 0;
      }
      cd.add(bottom.cpu_diff()[n * K + k], sum, mag, terms);
    }
  const vector<Dtype> wdiff(wb.cpu_diff(), wb.cpu_diff() + wb.count());
  for (int m = 0; m < M; ++m) {
    double bs = 0, bmag = 0;
    for (int n = 0; n < NB; ++n) bs += td[n * M + m], bmag += std::fabs((double)td[n * M + m]);
    cb.add(bb.cpu_diff()[m], bs, bmag, NB);
    for (int k = 0; k < K; ++k) {
      if (w0[m * K + k] == 0) {
        ok = ok && wdiff[m * K + k] == 0;                                  // the pattern is preserved
        continue;
      }
      double sum = 0, mag = 0;
      for (int n = 0; n < NB; ++n) {
        const double t = (double)x[n * K + k] * (double)td[n * M + m];
        sum += t, mag += std::fabs(t);
      }
      cw.add(wdiff[m * K + k], sum, mag, NB);
    }
  }
  escoin_solver_desc rule;
  memset(&rule, 0, sizeof(rule));
  rule.type = ESCOIN_SOLVER_SGD;
  rule.rate = 0.05, rule.momentum = 0.9, rule.diff_scale = 1.0;
  layer->SolverUpdate(rule);
  const vector<Dtype> w1(wb.cpu_data(), wb.cpu_data() + wb.count()), b1(bb.cpu_data(), bb.cpu_data() + bb.count());
  double sw = 0;      // the step: history = rate * diff (two roundings), w - history (one)
  bool moved = false;
  for (int i = 0; i < wb.count(); ++i) {
    if (w0[i] == 0) { ok = ok && w1[i] == 0; continue; }
    const double want = (double)w0[i] - 0.05 * (double)wdiff[i];
    sw = std::max(sw, std::fabs((double)w1[i] - want) / (4 * u * (std::fabs((double)w0[i]) + std::fabs(0.05 * (double)wdiff[i])) + tiny));
    moved = moved || w1[i] != w0[i];
  }
  layer->Forward(bv, tv);
  const double f1 = worst_top(x, w1, b1, top.cpu_data(), u, tiny);
  BaseConvolutionLayer<Dtype> *conv = dynamic_cast<BaseConvolutionLayer<Dtype> *>(layer.get());
  ok = ok && conv != nullptr;
  const long nnz0 = conv->nnz();
  long in_pattern = 0;
  for (int i = 0; i < wb.count(); ++i) in_pattern += w0[i] != 0;
  ok = ok && nnz0 == in_pattern;
  escoin_prune_desc prune;
  memset(&prune, 0, sizeof(prune));
  prune.mode = ESCOIN_PRUNE_KEEP;
  prune.keep = nnz0 / 2;
  layer->Prune(prune);
  ok = ok && conv->nnz() == nnz0 / 2;
  const vector<Dtype> w2(wb.cpu_data(), wb.cpu_data() + wb.count());
  long left = 0;
  for (int i = 0; i < wb.count(); ++i) {
    left += w2[i] != 0;
    ok = ok && (w2[i] == 0 || w2[i] == w1[i]);
  }
  ok = ok && left == nnz0 / 2;
  layer->Forward(bv, tv);
  const double f2 = worst_top(x, w2, b1, top.cpu_data(), u, tiny);
  const long ran = gpu ? conv->plan_stat("b2s") : -1, fast = gpu ? conv->plan_stat("update_fast") : -1;
  ok = ok && f0 <= 1.0 && f1 <= 1.0 && f2 <= 1.0 && cd.worst <= 1.0 && cw.worst <= 1.0 && cb.worst <= 1.0 && sw <= 1.0 && moved;
  if (gpu) ok = ok && ran == (b2s && sizeof(Dtype) == 4 ? 1 : 0);
  printf("%s b2s %d ran %ld (update_fast %ld): forward err / bound %.3g %.3g %.3g, data gradient %.3g, weight gradient %.3g, bias gradient %.3g, "
         "solver step %.3g, nnz %ld -> %ld  %s\n", label, (int)b2s, ran, fast, f0, f1, f2, cd.worst, cw.worst, cb.worst, sw, nnz0, conv->nnz(),
         ok ? "OK" : "FAIL");
  Caffe::set_b2s(false);
  return ok ? 0 : 1;
}

int main(int argc, char **argv) {
  const bool cpu_only = argc > 1 && !strcmp(argv[1], "--cpu-only");
  if (argc > 1 && !strcmp(argv[1], "--transpose")) {
    Caffe::set_mode(Caffe::CPU);
    LayerParameter lp;
    lp.name = "ip_t";
    lp.type = "InnerProduct";
    lp.inner_product_param.num_output = M;
    lp.inner_product_param.transpose = true;
    shared_ptr<Layer<float> > layer = LayerRegistry<float>::CreateLayer(lp);
    Blob<float> bottom(NB, D1, D2, D3), top;
    vector<Blob<float> *> bv(1, &bottom), tv(1, &top);
    layer->SetUp(bv, tv);       // aborts
    printf("transpose = true was accepted FAIL\n");
    return 1;
  }
  int fails = 0;
  Caffe::set_mode(cpu_only ? Caffe::CPU : Caffe::GPU);
  Caffe::set_cpu_threads(2);
  if (Caffe::b2s()) {
    printf("default b2s on FAIL\n");
    ++fails;
  }
  bool listed = false;
  const vector<string> types = LayerRegistry<float>::LayerTypeList();
  for (size_t i = 0; i < types.size(); ++i) listed = listed || types[i] == "InnerProduct";
  if (!listed) {
    printf("InnerProduct not registered FAIL\n");
    ++fails;
  }
  if (cpu_only) {
    fails += run<float>("float CPU", true, false);
    fails += run<double>("double CPU", true, false);
  } else {
    fails += run<float>("float GPU", true, true);
    fails += run<float>("float GPU", false, true);
    fails += run<double>("double GPU", true, true);
  }
  printf(fails ? "%d FAILED\n" : "all OK\n", fails);
  return fails;
}
