// tests/cpp/shim_s2b_selftest.cpp -- Caffe::set_s2b through the C++ shim: one dilated ConvolutionLayer<float>
// (2 x 5 x 8 x 7 -> 6, 3x3 dilation 2 pad 2, about half of the weights pruned) runs Forward, Backward, SolverUpdate and
// Forward again, once under Caffe::set_s2b(true) and once with it off.  Every element of both tops and both bottom diffs
// lies within the derived bound of a float64 restatement -- gamma(terms + 4) x the sum of the terms' magnitudes, terms =
// the nonzeros of the output channel's row (forward) or of the input channel's taps (data gradient), tools/error_bound.py
// -- the weight and bias gradients, which the option does not touch, and with them the solver's new blobs are the same
// bits in both runs, and each plan's stat "s2b" says whether the inner plan ran.
//
//   shim_s2b_selftest            Caffe::GPU (needs a GPU)
//   shim_s2b_selftest --cpu-only Caffe::CPU: the setter is accepted and ignored; touches no device
// Prints one line per run, exit code = number of failures.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "caffe_shim.hpp"

using namespace caffe;

static unsigned rng = 11;
static float urand() {   // [-1, 1)
  rng = rng * 1664525u + 1013904223u;
  return (float)(((rng >> 8) & 0xFFFFFF) / 8388608.0 - 1.0);
}

enum { N = 2, C = 5, H = 8, W = 7, M = 6, K = 3, DIL = 2, PAD = 2 };

struct Run {
  vector<float> x, td;                 // bottom data and top diff (the same in every run)
  vector<float> w0, b0, w1, b1;        // the blobs before and after SolverUpdate
  vector<float> top0, top1, diff;      // the tops of the two Forwards, the bottom diff
  vector<float> wdiff, bdiff;          // the weight and bias gradients
  int OH = 0, OW = 0;
  long s2b = -1, fast = -1;            // stats "s2b" and "update_fast" (GPU mode)
};

static Run run_with(bool s2b) {
  Caffe::set_s2b(s2b);
  rng = 11;
  LayerParameter lp;
  lp.type = "Convolution";
  ConvolutionParameter &cp = lp.convolution_param;
  cp.num_output = M;
  cp.kernel_h = cp.kernel_w = K;
  cp.dilation = DIL;
  cp.pad_h = cp.pad_w = PAD;
  shared_ptr<Layer<float> > layer = LayerRegistry<float>::CreateLayer(lp);
  Blob<float> bottom(N, C, H, W), top;
  vector<Blob<float> *> bv(1, &bottom), tv(1, &top);
  float *d = bottom.mutable_cpu_data();
  for (int i = 0; i < bottom.count(); ++i) d[i] = urand();
  layer->SetUp(bv, tv);
  Blob<float> &wb = *layer->blobs()[0];
  Blob<float> &bb = *layer->blobs()[1];
  float *w = wb.mutable_cpu_data();
  for (int i = 0; i < wb.count(); ++i) {
    const float v = 0.1f * urand() + 0.2f;
    w[i] = urand() < 0.f ? 0.f : v;                                    // about half pruned
  }
  float *b = bb.mutable_cpu_data();
  for (int i = 0; i < bb.count(); ++i) b[i] = urand();
  Run r;
  r.x.assign(bottom.cpu_data(), bottom.cpu_data() + bottom.count());
  r.w0.assign(wb.cpu_data(), wb.cpu_data() + wb.count());
  r.b0.assign(bb.cpu_data(), bb.cpu_data() + bb.count());
  layer->WeightAlign();
  layer->Forward(bv, tv);
  r.OH = top.height(), r.OW = top.width();
  r.top0.assign(top.cpu_data(), top.cpu_data() + top.count());
  float *td = top.mutable_cpu_diff();
  for (int i = 0; i < top.count(); ++i) td[i] = urand();
  r.td.assign(top.cpu_diff(), top.cpu_diff() + top.count());
  memset(wb.mutable_cpu_diff(), 0, sizeof(float) * wb.count());
  memset(bb.mutable_cpu_diff(), 0, sizeof(float) * bb.count());
  float *bd = bottom.mutable_cpu_diff();
  for (int i = 0; i < bottom.count(); ++i) bd[i] = NAN;               // the data gradient overwrites
  layer->Backward(tv, vector<bool>(1, true), bv);
  r.diff.assign(bottom.cpu_diff(), bottom.cpu_diff() + bottom.count());
  r.wdiff.assign(wb.cpu_diff(), wb.cpu_diff() + wb.count());
  r.bdiff.assign(bb.cpu_diff(), bb.cpu_diff() + bb.count());
  escoin_solver_desc rule;
  memset(&rule, 0, sizeof(rule));
  rule.type = ESCOIN_SOLVER_SGD;
  rule.rate = 0.05, rule.momentum = 0.9, rule.diff_scale = 1.0;
  layer->SolverUpdate(rule);
  r.w1.assign(wb.cpu_data(), wb.cpu_data() + wb.count());
  r.b1.assign(bb.cpu_data(), bb.cpu_data() + bb.count());
  layer->Forward(bv, tv);
  r.top1.assign(top.cpu_data(), top.cpu_data() + top.count());
  BaseConvolutionLayer<float> *conv = dynamic_cast<BaseConvolutionLayer<float> *>(layer.get());
  const bool gpu = conv && Caffe::mode() == Caffe::GPU;
  r.s2b = gpu ? conv->plan_stat("s2b") : -1;
  r.fast = gpu ? conv->plan_stat("update_fast") : -1;
  Caffe::set_s2b(false);
  return r;
}

static double gam(double k) {
  const double u = std::ldexp(1.0, -24);
  return k * u / (1.0 - k * u);
}

// the worst |got - exact| / bound over a top computed with weights w and bias b (a non-finite element counts as infinite)
static double worst_top(const Run &r, const vector<float> &w, const vector<float> &b, const vector<float> &top) {
  double worst = 0;
  for (int n = 0; n < N; ++n)
    for (int m = 0; m < M; ++m) {
      int terms = 0;
      for (int j = 0; j < C * K * K; ++j) terms += w[m * C * K * K + j] != 0.f;
      const double kk = terms + 4;
      for (int oh = 0; oh < r.OH; ++oh)
        for (int ow = 0; ow < r.OW; ++ow) {
          double sum = b[m], mag = std::fabs((double)b[m]);
          for (int c = 0; c < C; ++c)
            for (int kr = 0; kr < K; ++kr)
              for (int kc = 0; kc < K; ++kc) {
                const int h = oh + kr * DIL - PAD, x = ow + kc * DIL - PAD;
                if (h < 0 || x < 0 || h >= H || x >= W) continue;
                const double t = (double)w[((m * C + c) * K + kr) * K + kc] * (double)r.x[((n * C + c) * H + h) * W + x];
                sum += t, mag += std::fabs(t);
              }
          const float got = top[((n * M + m) * r.OH + oh) * r.OW + ow];
          const double bound = gam(kk) * mag + kk * std::ldexp(1.0, -149);
          worst = std::max(worst, std::isfinite(got) ? std::fabs((double)got - sum) / bound : INFINITY);
        }
    }
  return worst;
}

// the same over the bottom diff
static double worst_diff(const Run &r) {
  double worst = 0;
  for (int c = 0; c < C; ++c) {
    int terms = 0;
    for (int m = 0; m < M; ++m)
      for (int j = 0; j < K * K; ++j) terms += r.w0[(m * C + c) * K * K + j] != 0.f;
    const double kk = terms + 4;
    for (int n = 0; n < N; ++n)
      for (int h = 0; h < H; ++h)
        for (int w = 0; w < W; ++w) {
          double sum = 0, mag = 0;
          for (int m = 0; m < M; ++m)
            for (int kr = 0; kr < K; ++kr)
              for (int kc = 0; kc < K; ++kc) {
                const int th = h + PAD - kr * DIL, tw = w + PAD - kc * DIL;
                if (th < 0 || tw < 0 || th >= r.OH || tw >= r.OW) continue;
                const double t = (double)r.w0[((m * C + c) * K + kr) * K + kc] *
                                 (double)r.td[((n * M + m) * r.OH + th) * r.OW + tw];
                sum += t, mag += std::fabs(t);
              }
          const float got = r.diff[((n * C + c) * H + h) * W + w];
          const double bound = gam(kk) * mag + kk * std::ldexp(1.0, -149);
          worst = std::max(worst, std::isfinite(got) ? std::fabs((double)got - sum) / bound : INFINITY);
        }
  }
  return worst;
}

static bool same(const vector<float> &a, const vector<float> &b) {
  return a.size() == b.size() && memcmp(a.data(), b.data(), sizeof(float) * a.size()) == 0;
}

int main(int argc, char **argv) {
  const bool cpu_only = argc > 1 && !strcmp(argv[1], "--cpu-only");
  int fails = 0;
  Caffe::set_mode(cpu_only ? Caffe::CPU : Caffe::GPU);
  Caffe::set_cpu_threads(2);
  if (Caffe::s2b()) {
    printf("default s2b on FAIL\n");
    ++fails;
  }
  const Run a = run_with(true);
  const Run c = run_with(false);
  const double fa = std::max(worst_top(a, a.w0, a.b0, a.top0), worst_top(a, a.w1, a.b1, a.top1));
  const double fc = std::max(worst_top(c, c.w0, c.b0, c.top0), worst_top(c, c.w1, c.b1, c.top1));
  const double da = worst_diff(a), dc = worst_diff(c);
  bool changed = !same(a.w0, a.w1) && !same(a.b0, a.b1);
  bool ok = a.OH == 8 && a.OW == 7 && fa <= 1.0 && fc <= 1.0 && da <= 1.0 && dc <= 1.0 && changed;
  // what the option does not touch: the weight and bias gradients, and with them the solver's new blobs
  ok = ok && same(a.wdiff, c.wdiff) && same(a.bdiff, c.bdiff) && same(a.w1, c.w1) && same(a.b1, c.b1);
  if (cpu_only) {
    // one host kernel whatever the setter says: the same bits
    ok = ok && same(a.top0, c.top0) && same(a.top1, c.top1) && same(a.diff, c.diff);
    printf("float CPU setter ignored: forward err / bound %.3g, data gradient %.3g  %s\n", fa, da, ok ? "OK" : "FAIL");
  } else {
    ok = ok && a.s2b == 1 && c.s2b == 0 && a.fast == 1 && c.fast == 1;
    printf("float GPU s2b on ran %ld (update_fast %ld), off ran %ld: forward err / bound %.3g, off %.3g; data gradient %.3g, off %.3g  %s\n",
           a.s2b, a.fast, c.s2b, fa, fc, da, dc, ok ? "OK" : "FAIL");
  }
  fails += ok ? 0 : 1;
  printf(fails ? "%d FAILED\n" : "all OK\n", fails);
  return fails;
}
