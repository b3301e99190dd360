// tests/cpp/shim_wgrad_depthwise_selftest.cpp -- Caffe::set_wgrad_depthwise through the C++ shim: a depthwise
// ConvolutionLayer<float> (2 x 6 x 9 x 9, 3x3, pad 1, group 6) runs Backward_gpu with the option on and off, and the plan's stat
// "wgrad_kernel" reads 5 and not 5 (the gradients themselves: tests/test_wgrad_depthwise_gpu.py).  Needs a GPU.
#include <cmath>
#include <cstdio>

#include "caffe_shim.hpp"

using namespace caffe;

static long ran_with(bool on) {
  Caffe::set_wgrad_depthwise(on);
  LayerParameter lp;
  lp.type = "Convolution";
  ConvolutionParameter &cp = lp.convolution_param;
  cp.num_output = cp.group = 6;
  cp.kernel_h = cp.kernel_w = 3;
  cp.pad_h = cp.pad_w = 1;
  Blob<float> bottom, top;
  bottom.Reshape(2, 6, 9, 9);
  shared_ptr<Layer<float> > layer = LayerRegistry<float>::CreateLayer(lp);
  vector<Blob<float> *> bv(1, &bottom), tv(1, &top);
  for (int i = 0; i < bottom.count(); ++i) bottom.mutable_cpu_data()[i] = std::sin(0.37f * i);
  layer->SetUp(bv, tv);
  Blob<float> &wb = *layer->blobs()[0];
  for (int i = 0; i < wb.count(); ++i) wb.mutable_cpu_data()[i] = i % 4 ? 0.1f + 0.01f * i : 0.f;
  layer->WeightAlign();
  layer->Forward(bv, tv);
  for (int i = 0; i < top.count(); ++i) top.mutable_cpu_diff()[i] = std::cos(0.11f * i);
  layer->Backward(tv, vector<bool>(1, true), bv);
  return dynamic_cast<BaseConvolutionLayer<float> *>(layer.get())->plan_stat("wgrad_kernel");
}

int main() {
  const bool off_by_default = !Caffe::wgrad_depthwise();
  Caffe::set_mode(Caffe::GPU);
  const long on = ran_with(true), off = ran_with(false);
  const bool ok = off_by_default && on == ESCOIN_WGRAD_DEPTHWISE && off != ESCOIN_WGRAD_DEPTHWISE && off > 0;
  printf("float GPU Convolution wgrad_depthwise ran %ld / %ld  %s\n", on, off, ok ? "all OK" : "FAIL");
  return ok ? 0 : 1;
}
