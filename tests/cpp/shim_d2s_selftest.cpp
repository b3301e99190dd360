// tests/cpp/shim_d2s_selftest.cpp -- DeconvolutionLayer<float> through the C++ shim: the layers k4s2p1 (3 x 8 -> 6, 5 x 7, 4x4
// / 2 / 1) and k3s2p1 (2 x 5 -> 7, 6 x 5, 3x3 / 2 / 1) of tests/d2s_common.py, about 60 % of the weights pruned, run SetUp,
// WeightAlign, Forward and Backward.  Every element of the top, the bottom diff and the weight and bias diffs lies within the
// derived bound of a plain float64 loop over the layer's definition -- gamma(terms + 4) x the sum of the terms' magnitudes,
// terms = the nonzeros of the output phase's inner row (forward), of the bottom channel's row (data gradient), the inner
// pixels of the batch (weight gradient) and those plus the P phases (bias gradient), tools/error_bound.py; the weight diff is
// exactly zero outside the pattern.
//
//   shim_d2s_selftest              Caffe::GPU: stat "deconv" is 1 (needs a GPU)
//   shim_d2s_selftest --cpu-only   Caffe::CPU; touches no device
//   shim_d2s_selftest --double     DeconvolutionLayer<double>: SetUp aborts with the library's message
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

static double gam(double k, double u) { return k * u / (1.0 - k * u); }

struct Check {
  double worst = 0;
  void add(double got, double want, double mag, double terms) {
    const double u = std::ldexp(1.0, -24), tiny = std::ldexp(1.0, -149);
    const double bound = gam(terms + 4, u) * mag + (terms + 4) * tiny;
    worst = std::max(worst, std::isfinite(got) ? std::fabs(got - want) / bound : (double)INFINITY);
  }
};

struct Shape { const char *name; int N, C, M, H, W, K, S, P; };

static int run(const Shape &s, bool gpu) {
  rng = 11;
  LayerParameter lp;
  lp.name = s.name;
  lp.type = "Deconvolution";
  ConvolutionParameter &cp = lp.convolution_param;
  cp.num_output = s.M; cp.kernel_h = cp.kernel_w = s.K; cp.stride_h = cp.stride_w = s.S; cp.pad_h = cp.pad_w = s.P;
  shared_ptr<Layer<float> > layer = LayerRegistry<float>::CreateLayer(lp);
  Blob<float> bottom(s.N, s.C, s.H, s.W), top;
  vector<Blob<float> *> bv(1, &bottom), tv(1, &top);
  float *d = bottom.mutable_cpu_data();
  for (int i = 0; i < bottom.count(); ++i) d[i] = (float)urand();
  layer->SetUp(bv, tv);
  const int OH = s.S * (s.H - 1) + s.K - 2 * s.P, OW = s.S * (s.W - 1) + s.K - 2 * s.P;
  const int kp = (s.K + s.S - 1) / s.S, Hi = s.H + kp - 1, Wi = s.W + kp - 1, PP = s.S * s.S;
  bool ok = !strcmp(layer->type(), "Deconvolution") && top.shape(0) == s.N && top.shape(1) == s.M && top.shape(2) == OH && top.shape(3) == OW;
  Blob<float> &wb = *layer->blobs()[0];
  Blob<float> &bb = *layer->blobs()[1];
  ok = ok && wb.shape(0) == s.C && wb.shape(1) == s.M && wb.shape(2) == s.K && wb.shape(3) == s.K && bb.count() == s.M;
  float *w = wb.mutable_cpu_data();
  for (int i = 0; i < wb.count(); ++i) {
    const float v = (float)(0.1 * urand() + 0.2);
    w[i] = urand() < 0.2 ? 0.f : v;                                        // about 60 % pruned
  }
  float *b = bb.mutable_cpu_data();
  for (int i = 0; i < bb.count(); ++i) b[i] = (float)urand();
  const vector<float> x(bottom.cpu_data(), bottom.cpu_data() + bottom.count());
  const vector<float> w0(wb.cpu_data(), wb.cpu_data() + wb.count()), b0(bb.cpu_data(), bb.cpu_data() + bb.count());
  auto W = [&](int c, int m, int kr, int kc) { return w0[((c * s.M + m) * s.K + kr) * s.K + kc]; };
  layer->WeightAlign();
  layer->Forward(bv, tv);
  Check cf, cd, cw, cb;
  for (int n = 0; n < s.N; ++n)
    for (int m = 0; m < s.M; ++m)
      for (int oh = 0; oh < OH; ++oh)
        for (int ow = 0; ow < OW; ++ow) {
          double sum = b0[m], mag = std::fabs((double)b0[m]);
          int terms = 0;
          for (int c = 0; c < s.C; ++c)
            for (int kr = (oh + s.P) % s.S; kr < s.K; kr += s.S)
              for (int kc = (ow + s.P) % s.S; kc < s.K; kc += s.S) {
                terms += W(c, m, kr, kc) != 0;                               // the phase's inner row
                const int h = (oh + s.P - kr) / s.S, ww = (ow + s.P - kc) / s.S;
                if (oh + s.P - kr < 0 || ow + s.P - kc < 0 || h >= s.H || ww >= s.W) continue;
                const double t = (double)W(c, m, kr, kc) * (double)x[((n * s.C + c) * s.H + h) * s.W + ww];
                sum += t, mag += std::fabs(t);
              }
          cf.add(top.cpu_data()[((n * s.M + m) * OH + oh) * OW + ow], sum, mag, terms);
        }
  float *tdp = top.mutable_cpu_diff();
  for (int i = 0; i < top.count(); ++i) tdp[i] = (float)urand();
  const vector<float> td(top.cpu_diff(), top.cpu_diff() + top.count());
  memset(wb.mutable_cpu_diff(), 0, sizeof(float) * wb.count());
  memset(bb.mutable_cpu_diff(), 0, sizeof(float) * bb.count());
  float *bd = bottom.mutable_cpu_diff();
  for (int i = 0; i < bottom.count(); ++i) bd[i] = NAN;                    // the data gradient overwrites
  layer->Backward(tv, vector<bool>(1, true), bv);
  auto TD = [&](int n, int m, int oh, int ow) -> double {
    return oh < 0 || ow < 0 || oh >= OH || ow >= OW ? 0.0 : (double)td[((n * s.M + m) * OH + oh) * OW + ow];
  };
  for (int n = 0; n < s.N; ++n)
    for (int c = 0; c < s.C; ++c) {
      int row = 0;
      for (int m = 0; m < s.M; ++m)
        for (int k = 0; k < s.K * s.K; ++k) row += W(c, m, k / s.K, k % s.K) != 0;
      for (int h = 0; h < s.H; ++h)
        for (int ww = 0; ww < s.W; ++ww) {
          double sum = 0, mag = 0;
          for (int m = 0; m < s.M; ++m)
            for (int kr = 0; kr < s.K; ++kr)
              for (int kc = 0; kc < s.K; ++kc) {
                const double t = (double)W(c, m, kr, kc) * TD(n, m, h * s.S + kr - s.P, ww * s.S + kc - s.P);
                sum += t, mag += std::fabs(t);
              }
          cd.add(bottom.cpu_diff()[((n * s.C + c) * s.H + h) * s.W + ww], sum, mag, row);
        }
    }
  const double inner_pixels = (double)s.N * Hi * Wi;
  for (int c = 0; c < s.C; ++c)
    for (int m = 0; m < s.M; ++m)
      for (int kr = 0; kr < s.K; ++kr)
        for (int kc = 0; kc < s.K; ++kc) {
          const float got = wb.cpu_diff()[((c * s.M + m) * s.K + kr) * s.K + kc];
          if (W(c, m, kr, kc) == 0) {
            ok = ok && got == 0;                                             // the pattern is preserved
            continue;
          }
          double sum = 0, mag = 0;
          for (int n = 0; n < s.N; ++n)
            for (int h = 0; h < s.H; ++h)
              for (int ww = 0; ww < s.W; ++ww) {
                const double t = (double)x[((n * s.C + c) * s.H + h) * s.W + ww] * TD(n, m, h * s.S + kr - s.P, ww * s.S + kc - s.P);
                sum += t, mag += std::fabs(t);
              }
          cw.add(got, sum, mag, inner_pixels);
        }
  for (int m = 0; m < s.M; ++m) {
    double sum = 0, mag = 0;
    for (int n = 0; n < s.N; ++n)
      for (int oh = 0; oh < OH; ++oh)
        for (int ow = 0; ow < OW; ++ow) sum += TD(n, m, oh, ow), mag += std::fabs(TD(n, m, oh, ow));
    cb.add(bb.cpu_diff()[m], sum, mag, inner_pixels + PP);
  }
  BaseConvolutionLayer<float> *conv = dynamic_cast<BaseConvolutionLayer<float> *>(layer.get());
  ok = ok && conv != nullptr;
  long in_pattern = 0;
  for (int i = 0; i < wb.count(); ++i) in_pattern += w0[i] != 0;
  ok = ok && conv->nnz() == in_pattern;
  const long ran = gpu ? conv->plan_stat("deconv") : -1;
  if (gpu) ok = ok && ran == 1;
  ok = ok && cf.worst <= 1.0 && cd.worst <= 1.0 && cw.worst <= 1.0 && cb.worst <= 1.0;
  printf("%s %s deconv ran %ld: forward err / bound %.3g, data gradient %.3g, weight gradient %.3g, bias gradient %.3g, nnz %ld  %s\n",
         gpu ? "GPU" : "CPU", s.name, ran, cf.worst, cd.worst, cw.worst, cb.worst, conv->nnz(), ok ? "OK" : "FAIL");
  return ok ? 0 : 1;
}

int main(int argc, char **argv) {
  const bool cpu_only = argc > 1 && !strcmp(argv[1], "--cpu-only");
  if (argc > 1 && !strcmp(argv[1], "--double")) {
    Caffe::set_mode(Caffe::CPU);
    LayerParameter lp;
    lp.name = "up64";
    lp.type = "Deconvolution";
    lp.convolution_param.num_output = 2;
    lp.convolution_param.kernel_h = lp.convolution_param.kernel_w = 2;
    shared_ptr<Layer<double> > layer = LayerRegistry<double>::CreateLayer(lp);
    Blob<double> bottom(1, 2, 3, 3), top;
    vector<Blob<double> *> bv(1, &bottom), tv(1, &top);
    layer->SetUp(bv, tv);       // aborts
    printf("Dtype = double was accepted FAIL\n");
    return 1;
  }
  int fails = 0;
  Caffe::set_mode(cpu_only ? Caffe::CPU : Caffe::GPU);
  Caffe::set_cpu_threads(2);
  bool listed = false;
  const vector<string> types = LayerRegistry<float>::LayerTypeList();
  for (size_t i = 0; i < types.size(); ++i) listed = listed || types[i] == "Deconvolution";
  if (!listed) {
    printf("Deconvolution not registered FAIL\n");
    ++fails;
  }
  const Shape shapes[] = {{"k4s2p1", 3, 8, 6, 5, 7, 4, 2, 1}, {"k3s2p1", 2, 5, 7, 6, 5, 3, 2, 1}};
  for (const Shape &s : shapes) fails += run(s, !cpu_only);
  printf(fails ? "%d FAILED\n" : "all OK\n", fails);
  return fails;
}
