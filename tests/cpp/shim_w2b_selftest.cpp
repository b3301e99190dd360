// Caffe::set_w2b through the C++ shim: one ConvolutionLayer<float> (2 x 2 x 3 x 300 -> 4, 3x3 pad 1, half pruned) runs Forward_gpu
// and Backward_gpu with the option on and off.  All data are small integers, so every sum is exact in fp32 whatever its order:
// top, bottom diff, weight and bias gradients are the same bits, and each plan's stats say whether the strips ran.  Needs a GPU.
#include <cstdio>
#include <cstring>
#include <vector>

#include "caffe_shim.hpp"

using namespace caffe;
static unsigned rng = 11;
static float irand(int lim) {   // an integer in [-lim, lim]
  rng = rng * 1664525u + 1013904223u;
  return (float)((int)((rng >> 8) % (2 * lim + 1)) - lim);
}
static void fill(float *p, int n, int lim) {
  for (int i = 0; i < n; ++i) p[i] = irand(lim);
}
struct Run {
  vector<float> out[4];                // top, bottom diff, weight diff, bias diff
  long w2b = -1, strips = -1;
};
static Run run_with(bool w2b) {
  Caffe::set_w2b(w2b);
  rng = 11;
  LayerParameter lp;
  lp.type = "Convolution";
  ConvolutionParameter &cp = lp.convolution_param;
  cp.num_output = 4;
  cp.kernel_h = cp.kernel_w = 3;
  cp.pad_h = cp.pad_w = 1;
  shared_ptr<Layer<float> > layer = LayerRegistry<float>::CreateLayer(lp);
  Blob<float> bottom(2, 2, 3, 300), top;
  vector<Blob<float> *> bv(1, &bottom), tv(1, &top);
  fill(bottom.mutable_cpu_data(), bottom.count(), 3);
  layer->SetUp(bv, tv);
  Blob<float> &wb = *layer->blobs()[0], &bb = *layer->blobs()[1];
  fill(wb.mutable_cpu_data(), wb.count(), 2);
  for (int i = 0; i < wb.count(); i += 2) wb.mutable_cpu_data()[i] = 0.f;     // half pruned, at least
  fill(bb.mutable_cpu_data(), bb.count(), 5);
  layer->WeightAlign();
  layer->Forward(bv, tv);
  fill(top.mutable_cpu_diff(), top.count(), 3);
  memset(wb.mutable_cpu_diff(), 0, sizeof(float) * wb.count());
  memset(bb.mutable_cpu_diff(), 0, sizeof(float) * bb.count());
  layer->Backward(tv, vector<bool>(1, true), bv);
  Run r;
  r.out[0].assign(top.cpu_data(), top.cpu_data() + top.count());
  r.out[1].assign(bottom.cpu_diff(), bottom.cpu_diff() + bottom.count());
  r.out[2].assign(wb.cpu_diff(), wb.cpu_diff() + wb.count());
  r.out[3].assign(bb.cpu_diff(), bb.cpu_diff() + bb.count());
  BaseConvolutionLayer<float> *conv = dynamic_cast<BaseConvolutionLayer<float> *>(layer.get());
  r.w2b = conv ? conv->plan_stat("w2b") : -1;
  r.strips = conv ? conv->plan_stat("w2b_strips") : -1;
  Caffe::set_w2b(false);
  return r;
}
int main() {
  Caffe::set_mode(Caffe::GPU);
  bool ok = !Caffe::w2b();                                              // off by default
  const Run a = run_with(true), c = run_with(false);
  for (int i = 0; i < 4; ++i) {
    bool any = false;
    for (float v : a.out[i]) any = any || v != 0.f;
    ok = ok && any && a.out[i].size() == c.out[i].size() && !memcmp(a.out[i].data(), c.out[i].data(), sizeof(float) * a.out[i].size());
  }
  ok = ok && a.w2b == 1 && a.strips == 2 && c.w2b == 0 && c.strips == 0;
  printf("float GPU w2b on ran %ld (%ld strips), off ran %ld: top, bottom diff, weight and bias gradients equal  %s\n", a.w2b, a.strips,
         c.w2b, ok ? "OK" : "FAIL");
  printf(ok ? "all OK\n" : "1 FAILED\n");
  return ok ? 0 : 1;
}
