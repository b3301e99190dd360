// tests/cpp/shim_dense_split_selftest.cpp -- Caffe::set_dense_split through the C++ shim: a dense ConvolutionLayer<float> runs
// Forward_gpu with the option on and off; stat "dense_split" reads 1 and 0 (results: tests/test_dense_split_gpu.py).  Needs a GPU.
#include <cmath>
#include <cstdio>

#include "caffe_shim.hpp"

using namespace caffe;

static long ran_with(bool on) {
  Caffe::set_dense_split(on);
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
  BaseConvolutionLayer<float> *conv = dynamic_cast<BaseConvolutionLayer<float> *>(layer.get());
  return conv->plan_stat("dense_variant") > 0 ? conv->plan_stat("dense_split") : -1;
}

int main() {
  const bool off_by_default = !Caffe::dense_split();
  Caffe::set_mode(Caffe::GPU);
  const long on = ran_with(true), off = ran_with(false);
  const bool ok = off_by_default && on == 1 && off == 0;
  printf("float GPU Convolution dense_split ran %ld / %ld  %s\n", on, off, ok ? "all OK" : "FAIL");
  return ok ? 0 : 1;
}
