// tests/cpp/shim_wgrad_bf16_selftest.cpp -- Caffe::set_wgrad_math through the C++ shim: a dense ConvolutionLayer<float> under
// Caffe::set_wgrad_kernel(ESCOIN_WGRAD_MFMA) runs Backward_gpu with the option on and off; stat "wgrad_math" reads 1 and 0
// (the gradients themselves: tests/test_wgrad_bf16_gpu.py).  Needs a GPU.
#include <cmath>
#include <cstdio>

#include "caffe_shim.hpp"

using namespace caffe;

static long ran_with(int math) {
  Caffe::set_wgrad_math(math);
  LayerParameter lp;
  lp.type = "Convolution";
  ConvolutionParameter &cp = lp.convolution_param;
  cp.num_output = 16;
  cp.kernel_h = cp.kernel_w = 3;
  cp.pad_h = cp.pad_w = 1;
  Blob<float> bottom, top;
  bottom.Reshape(2, 8, 9, 9);
  shared_ptr<Layer<float> > layer = LayerRegistry<float>::CreateLayer(lp);
  vector<Blob<float> *> bv(1, &bottom), tv(1, &top);
  for (int i = 0; i < bottom.count(); ++i) bottom.mutable_cpu_data()[i] = std::sin(0.37f * i);
  layer->SetUp(bv, tv);
  Blob<float> &wb = *layer->blobs()[0];
  for (int i = 0; i < wb.count(); ++i) wb.mutable_cpu_data()[i] = 0.1f + 0.01f * (i % 17);
  layer->WeightAlign();
  layer->Forward(bv, tv);
  for (int i = 0; i < top.count(); ++i) top.mutable_cpu_diff()[i] = std::cos(0.11f * i);
  layer->Backward(tv, vector<bool>(1, true), bv);
  BaseConvolutionLayer<float> *conv = dynamic_cast<BaseConvolutionLayer<float> *>(layer.get());
  return conv->plan_stat("wgrad_kernel") == ESCOIN_WGRAD_MFMA ? conv->plan_stat("wgrad_math") : -1;
}

int main() {
  const bool off_by_default = Caffe::wgrad_math() == ESCOIN_MATH_FP32;
  Caffe::set_mode(Caffe::GPU);
  Caffe::set_wgrad_kernel(ESCOIN_WGRAD_MFMA);
  const long on = ran_with(ESCOIN_MATH_BF16), off = ran_with(ESCOIN_MATH_FP32);
  const bool ok = off_by_default && on == ESCOIN_MATH_BF16 && off == ESCOIN_MATH_FP32;
  printf("float GPU Convolution wgrad_math ran %ld / %ld  %s\n", on, off, ok ? "all OK" : "FAIL");
  return ok ? 0 : 1;
}
