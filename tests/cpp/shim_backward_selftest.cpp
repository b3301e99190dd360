// tests/cpp/shim_backward_selftest.cpp -- ConvolutionLayer<Dtype>::Backward through the C++ shim, checked the way the
// reference's own conv tests check it (src/caffe/test/test_convolution_layer.cpp:709-812, TestGradient /
// TestDilatedGradient / Test1x1Gradient / TestGradientGroup) with a compact port of GradientChecker
// (include/caffe/test/test_gradient_check_util.hpp): loss = 1/2 sum(top^2), so top_diff = top; central differences with
// step 1e-2, |analytic - numeric| <= 1e-3 * max(|analytic|, |numeric|, 1) for every bottom element, weight and bias.
// Each case runs with all weights kept and with about half of them pruned.  The forward reads the CSR WeightAlign
// built, so a weight perturbation re-runs WeightAlign; weights with |w| < 2 * step are skipped (the pattern must not
// change), and a pruned weight's analytic gradient must be exactly 0 (the backward keeps the pattern).
//
//   shim_backward_selftest            float and double, Caffe::CPU and Caffe::GPU (needs a GPU)
//   shim_backward_selftest --cpu-only the Caffe::CPU combinations; touches no device
// Prints one line per case, exit code = number of failures.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "caffe_shim.hpp"

using namespace caffe;

static unsigned rng = 7;
static double urand() {   // [0, 1)
  rng = rng * 1664525u + 1013904223u;
  return ((rng >> 8) & 0xFFFFFF) / 16777216.0;
}
static double grand() {   // GaussianFiller stand-in (Box-Muller)
  double u1 = urand(), u2 = urand();
  if (u1 < 1e-7) u1 = 1e-7;
  return std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2);
}

struct Case {
  const char *name;
  int N, C, H, W, n_bottoms;
  int num_output, kernel, stride, pad, dilation, group;
};

static const Case kCases[] = {
    {"TestGradient", 2, 3, 6, 4, 2, 2, 3, 2, 0, 1, 1},
    {"TestDilatedGradient", 2, 3, 5, 6, 1, 2, 3, 1, 0, 2, 1},
    {"Test1x1Gradient", 2, 3, 6, 4, 2, 2, 1, 1, 0, 1, 1},
    {"TestGradientGroup", 2, 3, 6, 4, 2, 3, 3, 2, 0, 1, 3},
};

template <typename Dtype>
struct Net1 {
  shared_ptr<Layer<Dtype> > layer;
  vector<Blob<Dtype> *> bottom, top;
  vector<shared_ptr<Blob<Dtype> > > own;

  double loss() {   // Forward, then 1/2 sum(top^2)
    layer->Forward(bottom, top);
    double l = 0;
    for (Blob<Dtype> *t : top) {
      const Dtype *d = t->cpu_data();
      for (int i = 0; i < t->count(); ++i) l += 0.5 * (double)d[i] * (double)d[i];
    }
    return l;
  }
};

template <typename Dtype>
static int run_case(const Case &c, bool pruned) {
  const double step = 1e-2, threshold = 1e-3;
  LayerParameter lp;
  lp.type = "Convolution";
  ConvolutionParameter &cp = lp.convolution_param;
  cp.num_output = c.num_output;
  cp.kernel_h = cp.kernel_w = c.kernel;
  cp.stride_h = cp.stride_w = c.stride;
  cp.pad_h = cp.pad_w = c.pad;
  cp.dilation = c.dilation;
  cp.group = c.group;
  Net1<Dtype> net;
  net.layer = LayerRegistry<Dtype>::CreateLayer(lp);
  for (int b = 0; b < c.n_bottoms; ++b) {
    net.own.emplace_back(new Blob<Dtype>(c.N, c.C, c.H, c.W));
    net.bottom.push_back(net.own.back().get());
    Dtype *d = net.own.back()->mutable_cpu_data();
    for (int i = 0; i < net.own.back()->count(); ++i) d[i] = (Dtype)grand();
    net.own.emplace_back(new Blob<Dtype>());
    net.top.push_back(net.own.back().get());
  }
  net.layer->SetUp(net.bottom, net.top);
  Blob<Dtype> &wb = *net.layer->blobs()[0];
  Blob<Dtype> &bb = *net.layer->blobs()[1];
  {
    Dtype *w = wb.mutable_cpu_data();
    for (int i = 0; i < wb.count(); ++i) {
      w[i] = (Dtype)grand();
      if (pruned && urand() < 0.5) w[i] = 0;
    }
    Dtype *b = bb.mutable_cpu_data();
    for (int i = 0; i < bb.count(); ++i) b[i] = (Dtype)grand();
  }
  net.layer->WeightAlign();

  // analytic: top_diff = top, parameter diffs cleared (the solver's ClearParamDiffs), Backward
  net.loss();
  for (Blob<Dtype> *t : net.top) memcpy(t->mutable_cpu_diff(), t->cpu_data(), sizeof(Dtype) * t->count());
  memset(wb.mutable_cpu_diff(), 0, sizeof(Dtype) * wb.count());
  memset(bb.mutable_cpu_diff(), 0, sizeof(Dtype) * bb.count());
  net.layer->Backward(net.top, vector<bool>(net.bottom.size(), true), net.bottom);
  vector<vector<double> > gb(net.bottom.size());
  for (size_t b = 0; b < net.bottom.size(); ++b) {
    const Dtype *d = net.bottom[b]->cpu_diff();
    gb[b].assign(d, d + net.bottom[b]->count());
  }
  const Dtype *wdp = wb.cpu_diff();
  vector<double> gw(wdp, wdp + wb.count());
  const Dtype *bdp = bb.cpu_diff();
  vector<double> gbias(bdp, bdp + bb.count());

  int bad = 0, checked = 0;
  double worst = 0;
  auto compare = [&](double analytic, double numeric) {
    const double scale = std::max(std::max(std::fabs(analytic), std::fabs(numeric)), 1.0);
    const double err = std::fabs(analytic - numeric) / scale;
    worst = std::max(worst, err);
    ++checked;
    if (err > threshold) ++bad;
  };
  // bottoms
  for (size_t b = 0; b < net.bottom.size(); ++b)
    for (int i = 0; i < net.bottom[b]->count(); ++i) {
      Dtype *d = net.bottom[b]->mutable_cpu_data();
      const Dtype keep = d[i];
      d[i] = keep + (Dtype)step;
      const double lp_ = net.loss();
      d = net.bottom[b]->mutable_cpu_data();
      d[i] = keep - (Dtype)step;
      const double lm = net.loss();
      d = net.bottom[b]->mutable_cpu_data();
      d[i] = keep;
      compare(gb[b][i], (lp_ - lm) / (2 * step));
    }
  // weights: every perturbation is re-aligned (the forward reads the CSR); pruned weights must have a 0 gradient
  int pruned_nonzero = 0;
  for (int i = 0; i < wb.count(); ++i) {
    Dtype *w = wb.mutable_cpu_data();
    const Dtype keep = w[i];
    if (keep == 0) {
      if (gw[i] != 0) ++pruned_nonzero;
      continue;
    }
    if (std::fabs((double)keep) < 2 * step) continue;
    w[i] = keep + (Dtype)step;
    net.layer->WeightAlign();
    const double lp_ = net.loss();
    w = wb.mutable_cpu_data();
    w[i] = keep - (Dtype)step;
    net.layer->WeightAlign();
    const double lm = net.loss();
    w = wb.mutable_cpu_data();
    w[i] = keep;
    compare(gw[i], (lp_ - lm) / (2 * step));
  }
  net.layer->WeightAlign();
  // bias (read at every forward)
  for (int i = 0; i < bb.count(); ++i) {
    Dtype *b = bb.mutable_cpu_data();
    const Dtype keep = b[i];
    b[i] = keep + (Dtype)step;
    const double lp_ = net.loss();
    b = bb.mutable_cpu_data();
    b[i] = keep - (Dtype)step;
    const double lm = net.loss();
    b = bb.mutable_cpu_data();
    b[i] = keep;
    compare(gbias[i], (lp_ - lm) / (2 * step));
  }
  const bool ok = bad == 0 && pruned_nonzero == 0;
  printf("%s %s %-20s %-8s checked %4d  worst %.2e  pruned-with-gradient %d  %s\n", sizeof(Dtype) == 8 ? "double" : "float",
         Caffe::mode() == Caffe::GPU ? "GPU" : "CPU", c.name, pruned ? "pruned" : "dense", checked, worst,
         pruned_nonzero, ok ? "OK" : "FAIL");
  return ok ? 0 : 1;
}

int main(int argc, char **argv) {
  const bool cpu_only = argc > 1 && !strcmp(argv[1], "--cpu-only");
  int fails = 0;
  for (int m = 0; m < (cpu_only ? 1 : 2); ++m) {
    Caffe::set_mode(m == 0 ? Caffe::CPU : Caffe::GPU);
    Caffe::set_cpu_threads(2);
    for (const Case &c : kCases)
      for (int pruned = 0; pruned < 2; ++pruned) {
        fails += run_case<float>(c, pruned != 0);
        fails += run_case<double>(c, pruned != 0);
      }
  }
  printf(fails ? "%d FAILED\n" : "all OK\n", fails);
  return fails;
}
