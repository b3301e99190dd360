// tests/cpp/shim_wgrad_pointwise_selftest.cpp -- Caffe::set_wgrad_pointwise through the C++ shim: a pointwise
// ConvolutionLayer<float> (3 x 40 x 19 x 19 -> 70, 1x1, four weights in five pruned: the pw_straddle shape of
// tests/test_wgrad_pointwise_gpu.py) and an InnerProductLayer<float> (70 x 300 -> 33 under Caffe::set_b2s) each run one
// Backward_gpu with the option on; blobs_[0]->diff and blobs_[1]->diff agree with the same layer's Backward in Caffe::CPU
// mode within 1e-4 of their largest element, the pruned positions' gradient stays 0, and each plan's stat "wgrad_kernel"
// says that the pointwise kernel ran -- and, with the option off, that it did not.
//
//   shim_wgrad_pointwise_selftest            needs a GPU
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

struct Grads {
  vector<float> w, b;
  vector<char> kept;
  long ran = -1;
};

// One layer's Backward under the current mode and options: blobs_[0]->diff, blobs_[1]->diff, the pattern, and the plan's
// stat "wgrad_kernel" (GPU mode; -1 in CPU mode, where no device kernel runs).
static Grads backward_of(bool inner_product) {
  rng = 11;
  LayerParameter lp;
  Blob<float> bottom, top;
  if (inner_product) {
    lp.type = "InnerProduct";
    lp.inner_product_param.num_output = 33;
    bottom.Reshape(70, 300, 1, 1);
  } else {
    lp.type = "Convolution";
    ConvolutionParameter &cp = lp.convolution_param;
    cp.num_output = 70;
    cp.kernel_h = cp.kernel_w = 1;
    cp.stride_h = cp.stride_w = 1;
    cp.pad_h = cp.pad_w = 0;
    bottom.Reshape(3, 40, 19, 19);
  }
  shared_ptr<Layer<float> > layer = LayerRegistry<float>::CreateLayer(lp);
  vector<Blob<float> *> bv(1, &bottom), tv(1, &top);
  float *d = bottom.mutable_cpu_data();
  for (int i = 0; i < bottom.count(); ++i) d[i] = urand();
  layer->SetUp(bv, tv);
  Blob<float> &wb = *layer->blobs()[0];
  Blob<float> &bb = *layer->blobs()[1];
  Grads g;
  g.kept.resize(wb.count());
  float *w = wb.mutable_cpu_data();
  for (int i = 0; i < wb.count(); ++i) {
    const float v = 0.1f * urand() + 0.2f;
    g.kept[i] = urand() > 0.6f;
    w[i] = g.kept[i] ? v : 0.f;
  }
  float *b = bb.mutable_cpu_data();
  for (int i = 0; i < bb.count(); ++i) b[i] = urand();
  layer->WeightAlign();
  layer->Forward(bv, tv);
  float *td = top.mutable_cpu_diff();
  for (int i = 0; i < top.count(); ++i) td[i] = urand();
  memset(wb.mutable_cpu_diff(), 0, sizeof(float) * wb.count());
  memset(bb.mutable_cpu_diff(), 0, sizeof(float) * bb.count());
  layer->Backward(tv, vector<bool>(1, true), bv);
  g.w.assign(wb.cpu_diff(), wb.cpu_diff() + wb.count());
  g.b.assign(bb.cpu_diff(), bb.cpu_diff() + bb.count());
  BaseConvolutionLayer<float> *conv = dynamic_cast<BaseConvolutionLayer<float> *>(layer.get());
  g.ran = (conv && Caffe::mode() == Caffe::GPU) ? conv->plan_stat("wgrad_kernel") : -1;
  return g;
}

static double rel(const vector<float> &a, const vector<float> &c) {
  if (a.size() != c.size() || a.empty()) return 1.0;
  double scale = 0, worst = 0;
  for (size_t i = 0; i < c.size(); ++i) scale = std::max(scale, (double)std::fabs(c[i]));
  for (size_t i = 0; i < c.size(); ++i) worst = std::max(worst, std::fabs((double)a[i] - (double)c[i]));
  return scale > 0 ? worst / scale : 1.0;
}

int main() {
  int fails = 0;
  Caffe::set_cpu_threads(2);
  if (Caffe::wgrad_pointwise()) {
    printf("default wgrad_pointwise on FAIL\n");
    ++fails;
  }
  for (int ip = 0; ip < 2; ++ip) {
    Caffe::set_b2s(ip != 0);
    Caffe::set_mode(Caffe::CPU);
    const Grads want = backward_of(ip != 0);
    Caffe::set_mode(Caffe::GPU);
    for (int on = 1; on >= 0; --on) {
      Caffe::set_wgrad_pointwise(on != 0);
      const Grads got = backward_of(ip != 0);
      const double rw = rel(got.w, want.w), rb = rel(got.b, want.b);
      bool ok = rw <= 1e-4 && rb <= 1e-4;
      for (size_t i = 0; i < got.w.size(); ++i) ok = ok && (got.kept[i] || got.w[i] == 0.f);
      ok = ok && (on ? got.ran == ESCOIN_WGRAD_POINTWISE : (got.ran == ESCOIN_WGRAD_ENTRY || got.ran == ESCOIN_WGRAD_STAGED));
      printf("float GPU %s wgrad_pointwise %d ran %ld: weight rel %.2e, bias rel %.2e  %s\n", ip ? "InnerProduct" : "Convolution", on,
             got.ran, rw, rb, ok ? "OK" : "FAIL");
      fails += ok ? 0 : 1;
    }
    Caffe::set_wgrad_pointwise(false);
  }
  Caffe::set_b2s(false);
  printf(fails ? "%d FAILED\n" : "all OK\n", fails);
  return fails;
}
