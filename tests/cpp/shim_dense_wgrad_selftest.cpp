// tests/cpp/shim_dense_wgrad_selftest.cpp -- ConvolutionLayer<Dtype>::DenseWeightDiff through the C++ shim.  A layer
// (Convolution and ConvolutionReLU) runs Forward, takes a random top diff, and DenseWeightDiff writes the dense weight
// gradient into a blob of blobs_[0]'s shape.  Checked:
//   every position, inside and outside the pattern, against a double-precision loop nest with the per-element bound
//   (pixels + 4) x eps x sum |G x bottom| (any summation order of those terms);
//   inside the pattern it agrees with the diff Backward accumulated into a zeroed blobs_[0], within the same bound;
//   blobs_[0]'s data and diff are not touched by the call;
//   the blob is accepted by Rewire as its score: the grown positions are the rule's (a stable sort on the integer keys of
//   the score as the layer computed it), and a second call after the Rewire gives the same bits (the result does not
//   depend on the pattern).
//
//   shim_dense_wgrad_selftest            float and double, Caffe::CPU and Caffe::GPU; needs a GPU
//   shim_dense_wgrad_selftest --cpu-only the Caffe::CPU combinations; touches no device
// Prints one line per case, exit code = number of failures.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "caffe_shim.hpp"

using namespace caffe;

static unsigned rng = 47;
static double urand() {
  rng = rng * 1664525u + 1013904223u;
  return ((rng >> 8) & 0xFFFFFF) / 16777216.0;
}

struct Case {
  const char *name;
  const char *type;
  int N, C, H, W;
  int num_output, kernel, stride, pad, dilation, group;
};

static const Case kCases[] = {
    {"Simple3x3", "Convolution", 2, 3, 6, 4, 4, 3, 1, 1, 1, 1},
    {"Pointwise", "Convolution", 2, 6, 6, 4, 4, 1, 1, 0, 1, 1},
    {"Group3", "Convolution", 2, 3, 6, 4, 3, 3, 2, 0, 1, 3},
    {"Wide70", "Convolution", 3, 8, 20, 19, 70, 3, 2, 1, 1, 1},       // 2 M-tiles, 2 column tiles, stride 2
    {"ReLU3x3", "ConvolutionReLU", 2, 4, 7, 5, 6, 3, 1, 1, 1, 2},
};

static uint64_t key_of(float v) {
  uint32_t k;
  memcpy(&k, &v, 4);
  return k & 0x7fffffffu;
}
static uint64_t key_of(double v) {
  uint64_t k;
  memcpy(&k, &v, 8);
  return k & 0x7fffffffffffffffull;
}

template <typename Dtype>
static int run_case(const Case &c) {
  const Caffe::Brew brew = Caffe::mode();
  LayerParameter lp;
  lp.type = c.type;
  ConvolutionParameter &cp = lp.convolution_param;
  cp.num_output = c.num_output;
  cp.kernel_h = cp.kernel_w = c.kernel;
  cp.stride_h = cp.stride_w = c.stride;
  cp.pad_h = cp.pad_w = c.pad;
  cp.dilation = c.dilation;
  cp.group = c.group;
  shared_ptr<Layer<Dtype> > base = LayerRegistry<Dtype>::CreateLayer(lp);
  ConvolutionLayer<Dtype> *layer = dynamic_cast<ConvolutionLayer<Dtype> *>(base.get());
  if (!layer) return 1;
  const bool relu = !strcmp(c.type, "ConvolutionReLU");
  Blob<Dtype> bottom_blob(c.N, c.C, c.H, c.W), top_blob;
  vector<Blob<Dtype> *> bottom(1, &bottom_blob), top(1, &top_blob);
  layer->SetUp(bottom, top);
  {
    Dtype *x = bottom_blob.mutable_cpu_data();
    for (int i = 0; i < bottom_blob.count(); ++i) x[i] = (Dtype)(2 * urand() - 1);
    for (int k = 0; k < 2; ++k) {
      Blob<Dtype> &b = *layer->blobs()[k];
      Dtype *w = b.mutable_cpu_data();
      for (int i = 0; i < b.count(); ++i) {
        w[i] = (Dtype)(2 * urand() - 1);
        if (k == 0 && urand() < 0.5) w[i] = 0;
      }
    }
  }
  Blob<Dtype> &wb = *layer->blobs()[0];
  const int count = wb.count();
  vector<char> in_pattern((size_t)count, 0);
  long n = 0;
  for (int i = 0; i < count; ++i)
    if (wb.cpu_data()[i] != 0) in_pattern[(size_t)i] = 1, ++n;
  layer->WeightAlign();
  layer->Forward(bottom, top);
  {
    Dtype *td = top_blob.mutable_cpu_diff();
    for (int i = 0; i < top_blob.count(); ++i) td[i] = (Dtype)(2 * urand() - 1);
  }
  // Backward into a zeroed diff: the masked gradient
  std::fill(wb.mutable_cpu_diff(), wb.mutable_cpu_diff() + count, (Dtype)0);
  layer->Backward(top, vector<bool>(1, false), bottom);
  const vector<Dtype> w_before(wb.cpu_data(), wb.cpu_data() + count), d_before(wb.cpu_diff(), wb.cpu_diff() + count);

  Blob<Dtype> out;
  layer->DenseWeightDiff(top, bottom, &out);
  int bad = 0;
  if (out.count() != count || out.shape() != wb.shape()) return 1;
  const vector<Dtype> got(out.cpu_data(), out.cpu_data() + count);
  if (memcmp(wb.cpu_data(), w_before.data(), sizeof(Dtype) * count) || memcmp(wb.cpu_diff(), d_before.data(), sizeof(Dtype) * count)) ++bad;

  // the double-precision loop nest and the bound
  const int OH = top_blob.shape(2), OW = top_blob.shape(3), Cg = c.C / c.group, Mg = c.num_output / c.group, K = c.kernel;
  const Dtype *x = bottom_blob.cpu_data(), *t = top_blob.cpu_data(), *td = top_blob.cpu_diff();
  const double eps = std::numeric_limits<Dtype>::epsilon() / 2, terms = (double)c.N * OH * OW + 4;
  double worst = 0;
  int outside_nonzero = 0, masked_bad = 0;
  for (int oc = 0; oc < c.num_output; ++oc)
    for (int ic = 0; ic < Cg; ++ic)
      for (int kr = 0; kr < K; ++kr)
        for (int kc = 0; kc < K; ++kc) {
          double s = 0, mag = 0;
          for (int img = 0; img < c.N; ++img)
            for (int oh = 0; oh < OH; ++oh)
              for (int ow = 0; ow < OW; ++ow) {
                const int h = oh * c.stride - c.pad + kr * c.dilation, w = ow * c.stride - c.pad + kc * c.dilation;
                if (h < 0 || h >= c.H || w < 0 || w >= c.W) continue;
                const size_t gi = (((size_t)img * c.num_output + oc) * OH + oh) * OW + ow;
                if (relu && !(t[gi] > 0)) continue;
                const double xv = x[(((size_t)img * c.C + (oc / Mg) * Cg + ic) * c.H + h) * c.W + w];
                s += (double)td[gi] * xv;
                mag += std::fabs((double)td[gi] * xv);
              }
          const size_t at = (((size_t)oc * Cg + ic) * K + kr) * K + kc;
          const double B = terms * eps * mag / (1 - terms * eps) + terms * 1e-300 + (sizeof(Dtype) == 4 ? terms * 1.5e-45 : 0);
          worst = std::max(worst, std::fabs((double)got[at] - s) / B);
          if (!in_pattern[at]) outside_nonzero += got[at] != 0;
          else if (std::fabs((double)got[at] - (double)d_before[at]) > 2 * B) ++masked_bad;
        }
  if (!(worst <= 1.0)) ++bad;
  if (masked_bad) ++bad;

  // the blob as Rewire's score
  vector<int> cand;
  for (int i = 0; i < count; ++i)
    if (!in_pattern[(size_t)i]) cand.push_back(i);
  const long grow = std::min<long>(std::max<long>(n / 4, 1), (long)cand.size());
  std::stable_sort(cand.begin(), cand.end(), [&](int p, int q) { return key_of(got[(size_t)p]) > key_of(got[(size_t)q]); });
  vector<char> is_grown((size_t)count, 0);
  for (long i = 0; i < grow; ++i) is_grown[(size_t)cand[(size_t)i]] = 1;
  Blob<Dtype> init_blob(vector<int>(1, count));
  for (int i = 0; i < count; ++i) init_blob.mutable_cpu_data()[i] = (Dtype)(urand() + 0.25);
  escoin_rewire_desc rd;
  memset(&rd, 0, sizeof(rd));
  rd.grow = grow;
  rd.score = brew == Caffe::GPU ? out.gpu_data() : out.cpu_data();
  rd.init = brew == Caffe::GPU ? init_blob.gpu_data() : init_blob.cpu_data();
  layer->Rewire(rd);
  if (layer->nnz() != n + grow || layer->plan_stat("rewire_last_grown") != grow) ++bad;
  int grown_wrong = 0;
  for (int i = 0; i < count; ++i) {
    const bool now = wb.cpu_data()[i] != 0;
    grown_wrong += now != (in_pattern[(size_t)i] || is_grown[(size_t)i]);
  }
  if (grown_wrong) ++bad;
  // the same bits on the new pattern
  Blob<Dtype> again;
  layer->DenseWeightDiff(top, bottom, &again);
  if (again.count() != count || memcmp(again.cpu_data(), got.data(), sizeof(Dtype) * count)) ++bad;
  const long calls = layer->plan_stat("dwg_count");
  const bool device = brew == Caffe::GPU && sizeof(Dtype) == 4;
  if (calls != (device ? 2 : 0)) ++bad;

  const bool ok = bad == 0 && grow > 0 && (cand.empty() || outside_nonzero > 0);
  printf("%s %s %-10s nnz %ld -> %ld  differing %d  worst %.3g of the bound  outside-nonzero %d  grown-wrong %d  device-calls %ld  %s\n",
         sizeof(Dtype) == 8 ? "double" : "float", brew == Caffe::GPU ? "GPU" : "CPU", c.name, n, n + grow, bad, worst,
         outside_nonzero, grown_wrong, calls, ok ? "OK" : "FAIL");
  return ok ? 0 : 1;
}

int main(int argc, char **argv) {
  const bool cpu_only = argc > 1 && !strcmp(argv[1], "--cpu-only");
  int fails = 0;
  for (int m = 0; m < (cpu_only ? 1 : 2); ++m) {
    Caffe::set_mode(m == 0 ? Caffe::CPU : Caffe::GPU);
    Caffe::set_cpu_threads(2);
    for (const Case &c : kCases) {
      fails += run_case<float>(c);
      fails += run_case<double>(c);
    }
  }
  printf(fails ? "%d FAILED\n" : "all OK\n", fails);
  return fails;
}
