// tests/cpp/shim_dgrad_selftest.cpp -- Caffe::set_backward_kernel through the C++ shim: one ConvolutionLayer<float>
// (2 x 5 x 8 x 7 -> 6, 3x3 stride 2 pad 1, all weights kept: shape 2 of tests/test_dgrad_mfma_gpu.py) runs Backward once
// under Caffe::set_backward_kernel(ESCOIN_BWD_MFMA) and once under the default (AUTO: the gather kernel on a strided
// layer).  Every element of both bottom diffs lies within the derived bound of a float64 restatement of the data
// gradient -- gamma(taps + 4) x the sum of the terms' magnitudes, taps = 6 x 3 x 3 (tools/error_bound.py) -- and each
// plan's stat "bwd_data_kernel" says which kernel ran.
//
//   shim_dgrad_selftest            Caffe::GPU (needs a GPU)
//   shim_dgrad_selftest --cpu-only Caffe::CPU: the setter is accepted and ignored; touches no device
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

enum { N = 2, C = 5, H = 8, W = 7, M = 6, K = 3, S = 2, PAD = 1 };

struct Run {
  vector<float> diff;          // bottom diff
  vector<float> w, td;         // the layer's weights and top diff (the same in every run)
  int OH = 0, OW = 0;
  long ran = -1;               // stat "bwd_data_kernel" (GPU mode)
};

static Run bottom_diff_under(int k) {
  Caffe::set_backward_kernel(k);
  rng = 11;
  LayerParameter lp;
  lp.type = "Convolution";
  ConvolutionParameter &cp = lp.convolution_param;
  cp.num_output = M;
  cp.kernel_h = cp.kernel_w = K;
  cp.stride_h = cp.stride_w = S;
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
  for (int i = 0; i < wb.count(); ++i) w[i] = 0.1f * urand() + 0.2f;   // (never 0: every weight is a CSR entry)
  float *b = bb.mutable_cpu_data();
  for (int i = 0; i < bb.count(); ++i) b[i] = urand();
  layer->WeightAlign();
  layer->Forward(bv, tv);
  float *td = top.mutable_cpu_diff();
  for (int i = 0; i < top.count(); ++i) td[i] = urand();
  memset(wb.mutable_cpu_diff(), 0, sizeof(float) * wb.count());
  memset(bb.mutable_cpu_diff(), 0, sizeof(float) * bb.count());
  float *bd = bottom.mutable_cpu_diff();
  for (int i = 0; i < bottom.count(); ++i) bd[i] = NAN;               // the data gradient overwrites
  layer->Backward(tv, vector<bool>(1, true), bv);
  Run r;
  r.diff.assign(bottom.cpu_diff(), bottom.cpu_diff() + bottom.count());
  r.w.assign(wb.cpu_data(), wb.cpu_data() + wb.count());
  r.td.assign(top.cpu_diff(), top.cpu_diff() + top.count());
  r.OH = top.height(), r.OW = top.width();
  BaseConvolutionLayer<float> *conv = dynamic_cast<BaseConvolutionLayer<float> *>(layer.get());
  r.ran = (conv && Caffe::mode() == Caffe::GPU) ? conv->plan_stat("bwd_data_kernel") : -1;
  Caffe::set_backward_kernel(ESCOIN_KERNEL_AUTO);
  return r;
}

// the worst |got - exact| / bound over the bottom diff (a non-finite element counts as infinite)
static double worst_ratio(const Run &r) {
  const double u = std::ldexp(1.0, -24), kk = M * K * K + 4, gam = kk * u / (1.0 - kk * u);
  double worst = 0;
  for (int n = 0; n < N; ++n)
    for (int c = 0; c < C; ++c)
      for (int h = 0; h < H; ++h)
        for (int w = 0; w < W; ++w) {
          double sum = 0, mag = 0;
          for (int m = 0; m < M; ++m)
            for (int kr = 0; kr < K; ++kr)
              for (int kc = 0; kc < K; ++kc) {
                const int th = h + PAD - kr, tw = w + PAD - kc;
                if (th < 0 || tw < 0 || th % S || tw % S || th / S >= r.OH || tw / S >= r.OW) continue;
                const double t = (double)r.w[((m * C + c) * K + kr) * K + kc] *
                                 (double)r.td[((n * M + m) * r.OH + th / S) * r.OW + tw / S];
                sum += t, mag += std::fabs(t);
              }
          const float got = r.diff[((n * C + c) * H + h) * W + w];
          const double bound = gam * mag + kk * std::ldexp(1.0, -149);
          const double ratio = std::isfinite(got) ? std::fabs((double)got - sum) / bound : INFINITY;
          worst = std::max(worst, ratio);
        }
  return worst;
}

int main(int argc, char **argv) {
  const bool cpu_only = argc > 1 && !strcmp(argv[1], "--cpu-only");
  int fails = 0;
  Caffe::set_mode(cpu_only ? Caffe::CPU : Caffe::GPU);
  Caffe::set_cpu_threads(2);
  if (Caffe::backward_kernel() != ESCOIN_KERNEL_AUTO) {
    printf("default backward_kernel %d FAIL\n", Caffe::backward_kernel());
    ++fails;
  }
  const Run a = bottom_diff_under(ESCOIN_BWD_MFMA);
  const Run c = bottom_diff_under(ESCOIN_KERNEL_AUTO);
  const double ra = worst_ratio(a), rc = worst_ratio(c);
  bool ok = a.diff.size() == c.diff.size() && a.OH == 4 && a.OW == 4 && ra <= 1.0 && rc <= 1.0;
  if (cpu_only) {
    // one host data gradient whatever the setter says: the same bits
    ok = ok && memcmp(a.diff.data(), c.diff.data(), sizeof(float) * a.diff.size()) == 0;
    printf("float CPU setter ignored: err / bound %.3g  %s\n", ra, ok ? "OK" : "FAIL");
  } else {
    ok = ok && a.ran == ESCOIN_BWD_MFMA && c.ran == ESCOIN_KERNEL_GENERIC;
    printf("float GPU backward_kernel mfma ran %ld, default ran %ld: err / bound %.3g, default %.3g  %s\n", a.ran, c.ran, ra,
           rc, ok ? "OK" : "FAIL");
  }
  fails += ok ? 0 : 1;
  printf(fails ? "%d FAILED\n" : "all OK\n", fails);
  return fails;
}
