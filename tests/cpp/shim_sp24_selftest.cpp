// tests/cpp/shim_sp24_selftest.cpp -- Caffe::set_sp24 through the C++ shim: a ConvolutionLayer<float> with 2:4 weights runs
// its dense launch (LOWERED_GEMM) through Forward_gpu with the option on and off; stat "dense_sp24" reads 1 and 0 and the
// two tops agree within bf16's rounding (results: tests/test_sp24_gpu.py).  Needs a GPU.
#include <cmath>
#include <cstdio>
#include <vector>

#include "caffe_shim.hpp"

using namespace caffe;

static long ran_with(bool on, std::vector<float> *out) {
  Caffe::set_sp24(on);
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
  // rows of K = 72: positions 1 and 2 of every group of 4
  for (int i = 0; i < wb.count(); ++i) wb.mutable_cpu_data()[i] = (i % 4 == 1 || i % 4 == 2) ? 0.1f + 0.01f * (i % 17) : 0.f;
  layer->WeightAlign();
  layer->Forward(bv, tv);
  out->assign(top.cpu_data(), top.cpu_data() + top.count());
  BaseConvolutionLayer<float> *conv = dynamic_cast<BaseConvolutionLayer<float> *>(layer.get());
  if (conv->plan_stat("sp24_pattern") != (on ? 1 : 0)) return -2;
  return conv->plan_stat("dense_variant") > 0 ? conv->plan_stat("dense_sp24") : -1;
}

int main() {
  const bool off_by_default = !Caffe::sp24();
  Caffe::set_mode(Caffe::GPU);
  Caffe::set_conv_mode(Caffe::LOWERED_GEMM);
  std::vector<float> a, b;
  const long on = ran_with(true, &a), off = ran_with(false, &b);
  float worst = 0.f, scale = 0.f;
  for (size_t i = 0; i < a.size() && i < b.size(); ++i) {
    worst = std::fmax(worst, std::fabs(a[i] - b[i]));
    scale = std::fmax(scale, std::fabs(b[i]));
  }
  // (36 products of operands rounded to 8 bits each, against the fp32 kernel's: 2^-7 of the largest output is generous)
  const bool ok = off_by_default && on == 1 && off == 0 && a.size() == b.size() && scale > 0.f && worst <= scale / 128;
  printf("float GPU Convolution sp24 ran %ld / %ld, largest difference %g of %g  %s\n", on, off, worst, scale, ok ? "all OK" : "FAIL");
  return ok ? 0 : 1;
}
