// tests/cpp/shim_dgrad_bf16_selftest.cpp -- Caffe::set_dgrad_math through the C++ shim: one ConvolutionLayer<float>
// (2 x 5 x 8 x 7 -> 6, 3x3 stride 2 pad 1, all weights kept: the layer of shim_dgrad_selftest.cpp) runs Backward_gpu under
// Caffe::set_backward_kernel(ESCOIN_BWD_MFMA) with the option on and off; stat "dgrad_math" reads 1 and 0, and under 1 every
// element of the bottom diff lies within the fp32 accumulation bound -- gamma(taps + 4) x the sum of the terms' magnitudes,
// taps = 6 x 3 x 3 -- of a float64 restatement on the weights and the top diff rounded to bf16.  Needs a GPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "caffe_shim.hpp"

using namespace caffe;

enum { N = 2, C = 5, H = 8, W = 7, M = 6, K = 3, S = 2, PAD = 1, OH = 4, OW = 4 };

static double bf16_rne(float v) {   // nearest even (finite inputs)
  uint32_t u;
  memcpy(&u, &v, 4);
  u = (u + 0x7FFFu + ((u >> 16) & 1u)) & 0xFFFF0000u;
  memcpy(&v, &u, 4);
  return v;
}

// stat "dgrad_math" after one Backward under the option, or -1 where the MFMA kernel did not run; *worst: the largest
// |got - exact| / bound over the bottom diff against the operands rounded (math = bf16) or as they are
static long ran_with(int math, double *worst) {
  Caffe::set_dgrad_math(math);
  LayerParameter lp;
  lp.type = "Convolution";
  ConvolutionParameter &cp = lp.convolution_param;
  cp.num_output = M;
  cp.kernel_h = cp.kernel_w = K;
  cp.stride_h = cp.stride_w = S;
  cp.pad_h = cp.pad_w = PAD;
  Blob<float> bottom(N, C, H, W), top;
  shared_ptr<Layer<float> > layer = LayerRegistry<float>::CreateLayer(lp);
  vector<Blob<float> *> bv(1, &bottom), tv(1, &top);
  for (int i = 0; i < bottom.count(); ++i) bottom.mutable_cpu_data()[i] = std::sin(0.37f * i);
  layer->SetUp(bv, tv);
  Blob<float> &wb = *layer->blobs()[0];
  for (int i = 0; i < wb.count(); ++i) wb.mutable_cpu_data()[i] = 0.1f + 0.013f * (i % 17);   // (never 0: every weight is a CSR entry)
  layer->WeightAlign();
  layer->Forward(bv, tv);
  for (int i = 0; i < top.count(); ++i) top.mutable_cpu_diff()[i] = std::cos(0.11f * i);
  for (int i = 0; i < bottom.count(); ++i) bottom.mutable_cpu_diff()[i] = NAN;                // the data gradient overwrites
  layer->Backward(tv, vector<bool>(1, true), bv);
  const float *w = wb.cpu_data(), *td = top.cpu_diff(), *got = bottom.cpu_diff();
  const double u = std::ldexp(1.0, -24), kk = M * K * K + 4, gam = kk * u / (1.0 - kk * u);
  *worst = top.height() == OH && top.width() == OW ? 0 : INFINITY;
  for (int n = 0; n < N; ++n)
    for (int c = 0; c < C; ++c)
      for (int h = 0; h < H; ++h)
        for (int x = 0; x < W; ++x) {
          double sum = 0, mag = 0;
          for (int m = 0; m < M; ++m)
            for (int kr = 0; kr < K; ++kr)
              for (int kc = 0; kc < K; ++kc) {
                const int th = h + PAD - kr, tw = x + PAD - kc;
                if (th < 0 || tw < 0 || th % S || tw % S || th / S >= OH || tw / S >= OW) continue;
                const float wv = w[((m * C + c) * K + kr) * K + kc], gv = td[((n * M + m) * OH + th / S) * OW + tw / S];
                const double t = math ? bf16_rne(wv) * bf16_rne(gv) : (double)wv * (double)gv;
                sum += t, mag += std::fabs(t);
              }
          const float g = got[((n * C + c) * H + h) * W + x];
          const double ratio = std::isfinite(g) ? std::fabs((double)g - sum) / (gam * mag + kk * std::ldexp(1.0, -149)) : INFINITY;
          *worst = std::max(*worst, ratio);
        }
  BaseConvolutionLayer<float> *conv = dynamic_cast<BaseConvolutionLayer<float> *>(layer.get());
  return conv->plan_stat("bwd_data_kernel") == ESCOIN_BWD_MFMA ? conv->plan_stat("dgrad_math") : -1;
}

int main() {
  const bool off_by_default = Caffe::dgrad_math() == ESCOIN_MATH_FP32;
  Caffe::set_mode(Caffe::GPU);
  Caffe::set_backward_kernel(ESCOIN_BWD_MFMA);
  double r_on = 0, r_off = 0;
  const long on = ran_with(ESCOIN_MATH_BF16, &r_on), off = ran_with(ESCOIN_MATH_FP32, &r_off);
  const bool ok = off_by_default && on == ESCOIN_MATH_BF16 && off == ESCOIN_MATH_FP32 && r_on <= 1.0 && r_off <= 1.0;
  printf("float GPU Convolution dgrad_math ran %ld / %ld: err / bound %.3g / %.3g  %s\n", on, off, r_on, r_off, ok ? "all OK" : "FAIL");
  return ok ? 0 : 1;
}
