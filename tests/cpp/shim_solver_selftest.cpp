// tests/cpp/shim_solver_selftest.cpp -- Layer<Dtype>::SolverUpdate through the C++ shim.  Two identical layers take three
// training steps per solver rule (loss = 1/2 sum(top^2), so top_diff = top).  One does what exists without the fused
// step: ClearParamDiffs, Backward, the rule's arithmetic written here on the host over the dense blobs (Normalize,
// Regularize, ComputeUpdateValue, Blob::Update), then WeightUpdate().  The other calls Backward and SolverUpdate(), and
// never clears a diff itself.  After every step the tops, blobs_[0] and blobs_[1] of the two must be the same bits and
// every pruned weight still exactly 0.  This file is compiled with -ffp-contract=off: the host arithmetic below is one
// rounding per operation, like the library's.  Geometries: the reference's gradient cases
// (test_convolution_layer.cpp:709-812).
//
//   shim_solver_selftest            float and double, Caffe::CPU and Caffe::GPU; needs a GPU
//   shim_solver_selftest --cpu-only the Caffe::CPU combinations; touches no device
// Prints one line per case, exit code = number of failures.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "caffe_shim.hpp"

using namespace caffe;

static unsigned rng = 23;
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

struct Rule {
  const char *name;
  escoin_solver_desc d;
};

static escoin_solver_desc make_rule(int type, int reg, double rate, double diff_scale) {
  escoin_solver_desc d;
  memset(&d, 0, sizeof(d));
  d.type = type, d.regularization = reg;
  d.rate = rate, d.momentum = 0.9, d.momentum2 = 0.999, d.delta = 1e-8, d.decay = 5e-4, d.diff_scale = diff_scale;
  return d;
}

template <typename Dtype>
struct Net1 {
  shared_ptr<Layer<Dtype> > layer;
  shared_ptr<Blob<Dtype> > bottom_blob, top_blob;
  vector<Blob<Dtype> *> bottom, top;
  vector<Dtype> h[2], h2[2];     // the host-written solver's dense histories of blobs_[0] and blobs_[1]
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

// sgd_solver.cpp:118-204, sgd_solver.cu:7-12, nesterov_solver.cu:7-14, adam_solver.cu:7-15 and Blob::Update over one
// dense blob, every operation in Dtype
template <typename Dtype>
static void host_rule(const escoin_solver_desc &d, int n, Dtype *w, const Dtype *diff, Dtype *h, Dtype *h2) {
  const Dtype rate = (Dtype)d.rate, mom = (Dtype)d.momentum, mom2 = (Dtype)d.momentum2, delta = (Dtype)d.delta;
  const Dtype decay = (Dtype)d.decay, scale = (Dtype)d.diff_scale;
  const Dtype one_plus = (Dtype)1 + mom, one_minus1 = (Dtype)1 - mom, one_minus2 = (Dtype)1 - mom2;
  for (int i = 0; i < n; ++i) {
    Dtype g = diff[i];
    if (d.diff_scale != 1.0) g = scale * g;
    if (d.decay != 0.0 && d.regularization == ESCOIN_REG_L2) {
      const Dtype r = decay * w[i];
      g = g + r;
    } else if (d.decay != 0.0 && d.regularization == ESCOIN_REG_L1) {
      const Dtype sign = (Dtype)((Dtype(0) < w[i]) - (w[i] < Dtype(0)));
      const Dtype r = decay * sign;
      g = g + r;
    }
    Dtype u;
    if (d.type == ESCOIN_SOLVER_ADAM) {
      const Dtype a = h[i] * mom, b = g * one_minus1;
      const Dtype m = a + b;
      const Dtype gg = g * g;
      const Dtype c = h2[i] * mom2, e = gg * one_minus2;
      const Dtype v = c + e;
      const Dtype num = rate * m, den = std::sqrt(v) + delta;
      u = num / den;
      h[i] = m, h2[i] = v;
    } else {
      const Dtype a = mom * h[i], b = rate * g;
      const Dtype hn = a + b;
      if (d.type == ESCOIN_SOLVER_NESTEROV) {
        const Dtype c = one_plus * hn;
        u = c - a;
      } else {
        u = hn;
      }
      h[i] = hn;
    }
    w[i] = w[i] - u;
  }
}

template <typename Dtype>
static void forward_backward(Net1<Dtype> &net, bool clear_param_diffs) {
  net.layer->Forward(net.bottom, net.top);
  Blob<Dtype> &t = *net.top[0];
  memcpy(t.mutable_cpu_diff(), t.cpu_data(), sizeof(Dtype) * t.count());
  if (clear_param_diffs)
    for (int b = 0; b < 2; ++b) {
      Blob<Dtype> &blob = *net.layer->blobs()[b];
      memset(blob.mutable_cpu_diff(), 0, sizeof(Dtype) * blob.count());
    }
  net.layer->Backward(net.top, vector<bool>(1, true), net.bottom);
}

template <typename Dtype>
static int run_case(const Case &c, const Rule &rule) {
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
      a.h[k].assign(wa.count(), 0), a.h2[k].assign(wa.count(), 0);
    }
  }
  Blob<Dtype> &wa = *a.layer->blobs()[0];
  vector<char> pruned(wa.count());
  for (int i = 0; i < wa.count(); ++i) pruned[i] = wa.cpu_data()[i] == 0;
  a.layer->WeightAlign();
  b.layer->WeightAlign();
  int bad = 0, revived = 0;
  for (int step = 0; step < 3; ++step) {
    escoin_solver_desc d = rule.d;
    d.rate = rule.d.rate / (1 + step);          // an lr policy
    forward_backward(a, true);
    for (int k = 0; k < 2; ++k) {
      Blob<Dtype> &blob = *a.layer->blobs()[k];
      host_rule<Dtype>(d, blob.count(), blob.mutable_cpu_data(), blob.cpu_diff(), a.h[k].data(), a.h2[k].data());
    }
    a.layer->WeightUpdate();
    forward_backward(b, false);
    b.layer->SolverUpdate(d);
    a.layer->Forward(a.bottom, a.top);
    b.layer->Forward(b.bottom, b.top);
    if (a.top[0]->count() != b.top[0]->count() ||
        memcmp(a.top[0]->cpu_data(), b.top[0]->cpu_data(), sizeof(Dtype) * a.top[0]->count()) != 0)
      ++bad;
    for (int k = 0; k < 2; ++k) {
      Blob<Dtype> &ba = *a.layer->blobs()[k], &bb = *b.layer->blobs()[k];
      if (memcmp(ba.cpu_data(), bb.cpu_data(), sizeof(Dtype) * ba.count()) != 0) ++bad;
    }
    const Dtype *wb = b.layer->blobs()[0]->cpu_data();
    for (int i = 0; i < wa.count(); ++i)
      if (pruned[i] && (wb[i] != 0 || wa.cpu_data()[i] != 0)) ++revived;
  }
  int kept = 0;
  for (int i = 0; i < wa.count(); ++i) kept += !pruned[i];
  const bool ok = bad == 0 && revived == 0 && kept > 0;
  printf("%s %s %-10s %-8s steps 3  differing %d  pruned-revived %d  kept %d  %s\n", sizeof(Dtype) == 8 ? "double" : "float",
         brew == Caffe::GPU ? "GPU" : "CPU", c.name, rule.name, bad, revived, kept, ok ? "OK" : "FAIL");
  return ok ? 0 : 1;
}

int main(int argc, char **argv) {
  const bool cpu_only = argc > 1 && !strcmp(argv[1], "--cpu-only");
  const Rule rules[] = {
      {"sgd", make_rule(ESCOIN_SOLVER_SGD, ESCOIN_REG_L2, 0.01, 1.0)},
      {"nesterov", make_rule(ESCOIN_SOLVER_NESTEROV, ESCOIN_REG_L1, 0.01, 0.5)},
      {"adam", make_rule(ESCOIN_SOLVER_ADAM, ESCOIN_REG_L2, 0.001, 1.0 / 3.0)},
  };
  int fails = 0;
  for (int m = 0; m < (cpu_only ? 1 : 2); ++m) {
    Caffe::set_mode(m == 0 ? Caffe::CPU : Caffe::GPU);
    Caffe::set_cpu_threads(2);
    for (const Case &c : kCases)
      for (const Rule &r : rules) {
        fails += run_case<float>(c, r);
        fails += run_case<double>(c, r);
      }
  }
  printf(fails ? "%d FAILED\n" : "all OK\n", fails);
  return fails;
}
