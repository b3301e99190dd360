// tests/cpp/shim_wgrad_selftest.cpp -- Caffe::set_wgrad_kernel through the C++ shim: one ConvolutionLayer<float>
// (2 x 20 x 24 x 24 -> 36, 3x3 pad 1, all weights kept: the d_3x3 shape of tests/test_wgrad_mfma_gpu.py) runs Backward
// once under Caffe::set_wgrad_kernel(ESCOIN_WGRAD_MFMA) and once under the default (AUTO); blobs_[0]->diff of the two
// agrees within 1e-4 of its largest element, and each plan's stat "wgrad_kernel" says which kernel ran.
//
//   shim_wgrad_selftest            Caffe::GPU (needs a GPU)
//   shim_wgrad_selftest --cpu-only Caffe::CPU: the setter is accepted and ignored; touches no device
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

// Backward's blobs_[0]->diff for the layer created under wgrad kernel `k`; *ran = the plan's stat "wgrad_kernel"
// (GPU mode; -1 in CPU mode, where no device kernel runs).
static vector<float> weight_diff_under(int k, long *ran) {
  Caffe::set_wgrad_kernel(k);
  rng = 11;
  LayerParameter lp;
  lp.type = "Convolution";
  ConvolutionParameter &cp = lp.convolution_param;
  cp.num_output = 36;
  cp.kernel_h = cp.kernel_w = 3;
  cp.stride_h = cp.stride_w = 1;
  cp.pad_h = cp.pad_w = 1;
  shared_ptr<Layer<float> > layer = LayerRegistry<float>::CreateLayer(lp);
  Blob<float> bottom(2, 20, 24, 24), top;
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
  layer->Backward(tv, vector<bool>(1, true), bv);
  const float *wd = wb.cpu_diff();
  vector<float> out(wd, wd + wb.count());
  BaseConvolutionLayer<float> *conv = dynamic_cast<BaseConvolutionLayer<float> *>(layer.get());
  *ran = (conv && Caffe::mode() == Caffe::GPU) ? conv->plan_stat("wgrad_kernel") : -1;
  Caffe::set_wgrad_kernel(ESCOIN_WGRAD_AUTO);
  return out;
}

int main(int argc, char **argv) {
  const bool cpu_only = argc > 1 && !strcmp(argv[1], "--cpu-only");
  int fails = 0;
  Caffe::set_mode(cpu_only ? Caffe::CPU : Caffe::GPU);
  Caffe::set_cpu_threads(2);
  if (Caffe::wgrad_kernel() != ESCOIN_WGRAD_AUTO) {
    printf("default wgrad_kernel %d FAIL\n", Caffe::wgrad_kernel());
    ++fails;
  }
  long ran_mfma = 0, ran_auto = 0;
  const vector<float> a = weight_diff_under(ESCOIN_WGRAD_MFMA, &ran_mfma);
  const vector<float> c = weight_diff_under(ESCOIN_WGRAD_AUTO, &ran_auto);
  double scale = 0, worst = 0;
  for (size_t i = 0; i < c.size(); ++i) scale = std::max(scale, (double)std::fabs(c[i]));
  for (size_t i = 0; i < c.size(); ++i) worst = std::max(worst, std::fabs((double)a[i] - (double)c[i]));
  const double rel = worst / std::max(scale, 1e-30);
  bool ok = a.size() == c.size() && scale > 0 && rel <= 1e-4;
  if (cpu_only) {
    // one host weight gradient whatever the setter says: the same bits
    ok = ok && memcmp(a.data(), c.data(), sizeof(float) * a.size()) == 0;
    printf("float CPU setter ignored: rel %.2e  %s\n", rel, ok ? "OK" : "FAIL");
  } else {
    ok = ok && ran_mfma == ESCOIN_WGRAD_MFMA && (ran_auto == ESCOIN_WGRAD_ENTRY || ran_auto == ESCOIN_WGRAD_STAGED);
    printf("float GPU wgrad_kernel mfma ran %ld, default ran %ld: rel %.2e  %s\n", ran_mfma, ran_auto, rel, ok ? "OK" : "FAIL");
  }
  fails += ok ? 0 : 1;
  printf(fails ? "%d FAILED\n" : "all OK\n", fails);
  return fails;
}
