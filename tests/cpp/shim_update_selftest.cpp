// tests/cpp/shim_update_selftest.cpp -- Layer<Dtype>::WeightUpdate through the C++ shim: a training step is Forward,
// Backward, the solver's update of the blobs, WeightUpdate.  Two identical layers take three steps of plain SGD on the
// masked diff (loss = 1/2 sum(top^2), so top_diff = top); one calls WeightUpdate() after every step, the other
// WeightAlign().  After every step the tops of the two must be the same bits, and so must the weights at the end; a
// pruned weight must still be exactly 0.  Geometries: the reference's gradient cases (test_convolution_layer.cpp:709-812).
//
//   shim_update_selftest            float and double, Caffe::CPU and Caffe::GPU, and a layer aligned in GPU mode
//                                   whose steps run in CPU mode (the host-source update of a device plan); needs a GPU
//   shim_update_selftest --cpu-only the Caffe::CPU combinations; touches no device
// Prints one line per case, exit code = number of failures.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "caffe_shim.hpp"

using namespace caffe;

static unsigned rng = 11;
static double urand() {
  rng = rng * 1664525u + 1013904223u;
  return ((rng >> 8) & 0xFFFFFF) / 16777216.0;
}

struct Case {
  const char *name;
  int N, C, H, W;
  int num_output, kernel, stride, pad, dilation, group;
};

static const Case kCases[] = {
    {"Simple3x3", 2, 3, 6, 4, 4, 3, 1, 1, 1, 1},
    {"Strided", 2, 3, 6, 4, 2, 3, 2, 0, 1, 1},
    {"Dilated", 2, 3, 7, 6, 2, 3, 1, 0, 2, 1},
    {"Pointwise", 2, 6, 6, 4, 4, 1, 1, 0, 1, 1},
    {"Group3", 2, 3, 6, 4, 3, 3, 2, 0, 1, 3},
};

template <typename Dtype>
struct Net1 {
  shared_ptr<Layer<Dtype> > layer;
  shared_ptr<Blob<Dtype> > bottom_blob, top_blob;
  vector<Blob<Dtype> *> bottom, top;
};

template <typename Dtype>
static void make_net(const Case &c, Net1<Dtype> *net) {
  LayerParameter lp;
  lp.type = "Convolution";
  ConvolutionParameter &cp = lp.convolution_param;
  cp.num_output = c.num_output;
  cp.kernel_h = cp.kernel_w = c.kernel;
  cp.stride_h = cp.stride_w = c.stride;
  cp.pad_h = cp.pad_w = c.pad;
  cp.dilation = c.dilation;
  cp.group = c.group;
  net->layer = LayerRegistry<Dtype>::CreateLayer(lp);
  net->bottom_blob.reset(new Blob<Dtype>(c.N, c.C, c.H, c.W));
  net->top_blob.reset(new Blob<Dtype>());
  net->bottom.assign(1, net->bottom_blob.get());
  net->top.assign(1, net->top_blob.get());
  net->layer->SetUp(net->bottom, net->top);
}

// one step: Forward, top_diff = top, ClearParamDiffs, Backward, w -= lr * diff (weights and bias)
template <typename Dtype>
static void sgd_step(Net1<Dtype> &net, Dtype lr) {
  net.layer->Forward(net.bottom, net.top);
  Blob<Dtype> &t = *net.top[0];
  memcpy(t.mutable_cpu_diff(), t.cpu_data(), sizeof(Dtype) * t.count());
  for (int b = 0; b < 2; ++b) {
    Blob<Dtype> &blob = *net.layer->blobs()[b];
    memset(blob.mutable_cpu_diff(), 0, sizeof(Dtype) * blob.count());
  }
  net.layer->Backward(net.top, vector<bool>(1, true), net.bottom);
  for (int b = 0; b < 2; ++b) {
    Blob<Dtype> &blob = *net.layer->blobs()[b];
    const Dtype *d = blob.cpu_diff();
    Dtype *w = blob.mutable_cpu_data();
    for (int i = 0; i < blob.count(); ++i) w[i] -= lr * d[i];
  }
}

// mixed: the layers are aligned in GPU mode, the steps run in CPU mode, the last comparison in GPU mode again
template <typename Dtype>
static int run_case(const Case &c, bool mixed) {
  const Caffe::Brew brew = Caffe::mode();
  Net1<Dtype> a, b;
  make_net(c, &a);
  make_net(c, &b);
  {
    Dtype *x = a.bottom_blob->mutable_cpu_data();
    for (int i = 0; i < a.bottom_blob->count(); ++i) x[i] = (Dtype)(2 * urand() - 1);
    memcpy(b.bottom_blob->mutable_cpu_data(), x, sizeof(Dtype) * a.bottom_blob->count());
    for (int k = 0; k < 2; ++k) {
      Blob<Dtype> &wa = *a.layer->blobs()[k], &wb = *b.layer->blobs()[k];
      Dtype *w = wa.mutable_cpu_data();
      for (int i = 0; i < wa.count(); ++i) {
        w[i] = (Dtype)(2 * urand() - 1);
        if (k == 0 && urand() < 0.5) w[i] = 0;
      }
      memcpy(wb.mutable_cpu_data(), w, sizeof(Dtype) * wa.count());
    }
  }
  Blob<Dtype> &wa = *a.layer->blobs()[0], &wb = *b.layer->blobs()[0];
  vector<char> pruned(wa.count());
  for (int i = 0; i < wa.count(); ++i) pruned[i] = wa.cpu_data()[i] == 0;
  a.layer->WeightUpdate();     // not aligned yet: aligns
  b.layer->WeightAlign();
  if (mixed) Caffe::set_mode(Caffe::CPU);
  int bad = 0;
  for (int step = 0; step < 3; ++step) {
    sgd_step(a, (Dtype)0.01);
    sgd_step(b, (Dtype)0.01);
    a.layer->WeightUpdate();
    b.layer->WeightAlign();
    if (mixed && step == 2) Caffe::set_mode(Caffe::GPU);
    a.layer->Forward(a.bottom, a.top);
    b.layer->Forward(b.bottom, b.top);
    if (a.top[0]->count() != b.top[0]->count() ||
        memcmp(a.top[0]->cpu_data(), b.top[0]->cpu_data(), sizeof(Dtype) * a.top[0]->count()) != 0)
      ++bad;
  }
  Caffe::set_mode(brew);
  if (memcmp(wa.cpu_data(), wb.cpu_data(), sizeof(Dtype) * wa.count()) != 0) ++bad;
  int revived = 0, moved = 0;
  for (int i = 0; i < wa.count(); ++i) {
    if (pruned[i] && wa.cpu_data()[i] != 0) ++revived;
    if (!pruned[i]) ++moved;
  }
  const bool ok = bad == 0 && revived == 0 && a.layer->blobs()[0]->count() > 0;
  printf("%s %s %-10s steps 3  differing %d  pruned-revived %d  kept %d  %s\n", sizeof(Dtype) == 8 ? "double" : "float",
         mixed ? "MIXED" : brew == Caffe::GPU ? "GPU" : "CPU", c.name, bad, revived, moved, ok ? "OK" : "FAIL");
  return ok ? 0 : 1;
}

int main(int argc, char **argv) {
  const bool cpu_only = argc > 1 && !strcmp(argv[1], "--cpu-only");
  int fails = 0;
  for (int m = 0; m < (cpu_only ? 1 : 3); ++m) {
    Caffe::set_mode(m == 0 ? Caffe::CPU : Caffe::GPU);
    Caffe::set_cpu_threads(2);
    for (const Case &c : kCases) {
      fails += run_case<float>(c, m == 2);
      fails += run_case<double>(c, m == 2);
    }
  }
  printf(fails ? "%d FAILED\n" : "all OK\n", fails);
  return fails;
}
