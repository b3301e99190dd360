// tests/cpp/shim_rewire_selftest.cpp -- Layer<Dtype>::Rewire through the C++ shim.  A layer takes two training steps
// (loss = 1/2 sum(top^2), SolverUpdate), a Backward fills the diffs, then Rewire drops a third of the entries by magnitude
// and grows as many at the positions outside the pattern where a dense score is largest, with nonzero initial values.
// Checked, all bit for bit:
//   both selections are the rule's (stable sorts on the integer keys, written here);
//   the dropped positions of blobs_[0] are +0 in data and diff, the grown positions hold the grown values, every other
//   element is untouched;
//   the weights' histories travel through the map into zeroed arrays (kept entries keep theirs, grown entries start at
//   zero); the bias histories are untouched;
//   a SolverUpdate after Rewire equals the same on a layer rebuilt from the blob with hand-re-indexed histories (blobs,
//   histories and the next forward's top);
//   a WeightAlign from the blob afterwards reproduces the rewired pattern.
//
//   shim_rewire_selftest            float and double, Caffe::CPU and Caffe::GPU; needs a GPU
//   shim_rewire_selftest --cpu-only the Caffe::CPU combinations; touches no device
// Prints one line per case, exit code = number of failures.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

#include "caffe_shim.hpp"

using namespace caffe;

static unsigned rng = 31;
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
    {"Pointwise", 2, 6, 6, 4, 4, 1, 1, 0, 1, 1},
    {"Group3", 2, 3, 6, 4, 3, 3, 2, 0, 1, 3},
};

struct Rule {
  const char *name;
  escoin_solver_desc d;
};

static escoin_solver_desc make_rule(int type, int reg, double rate) {
  escoin_solver_desc d;
  memset(&d, 0, sizeof(d));
  d.type = type, d.regularization = reg;
  d.rate = rate, d.momentum = 0.9, d.momentum2 = 0.999, d.delta = 1e-8, d.decay = 5e-4, d.diff_scale = 1.0;
  return d;
}

// the layer under test with its histories in reach: the rebuilt layer receives hand-re-indexed ones
template <typename Dtype>
struct OpenLayer : public ConvolutionLayer<Dtype> {
  explicit OpenLayer(const LayerParameter &p) : ConvolutionLayer<Dtype>(p) {}
  vector<shared_ptr<Blob<Dtype> > > &histories() { return this->history_; }
};

template <typename Dtype>
struct Net1 {
  shared_ptr<OpenLayer<Dtype> > layer;
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
  net->layer.reset(new OpenLayer<Dtype>(lp));
  net->bottom_blob.reset(new Blob<Dtype>(c.N, c.C, c.H, c.W));
  net->top_blob.reset(new Blob<Dtype>());
  net->bottom.assign(1, net->bottom_blob.get());
  net->top.assign(1, net->top_blob.get());
  net->layer->SetUp(net->bottom, net->top);
}

template <typename Dtype>
static void forward_backward(Net1<Dtype> &net) {
  net.layer->Forward(net.bottom, net.top);
  Blob<Dtype> &t = *net.top[0];
  memcpy(t.mutable_cpu_diff(), t.cpu_data(), sizeof(Dtype) * t.count());
  net.layer->Backward(net.top, vector<bool>(1, true), net.bottom);
}

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
static vector<Dtype> copy_of(const Dtype *p, int n) { return vector<Dtype>(p, p + n); }

template <typename Dtype>
static bool same(const Dtype *a, const Dtype *b, size_t n) { return memcmp(a, b, sizeof(Dtype) * n) == 0; }

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
      Blob<Dtype> &wa = *a.layer->blobs()[k];
      Dtype *w = wa.mutable_cpu_data();
      for (int i = 0; i < wa.count(); ++i) {
        w[i] = (Dtype)(2 * urand() - 1);
        if (k == 0 && urand() < 0.4) w[i] = 0;
      }
    }
  }
  Blob<Dtype> &wa = *a.layer->blobs()[0], &ba = *a.layer->blobs()[1];
  const int count = wa.count();
  vector<int> pattern;     // the CSR entries' positions in blobs_[0]: row-major, which is (group, row, column) order
  vector<char> in_pattern((size_t)count, 0);
  for (int i = 0; i < count; ++i)
    if (wa.cpu_data()[i] != 0) pattern.push_back(i), in_pattern[(size_t)i] = 1;
  a.layer->WeightAlign();
  const long n = a.layer->nnz();
  int bad = 0;
  if (n != (long)pattern.size()) ++bad;
  for (int step = 0; step < 2; ++step) {
    forward_backward(a);
    a.layer->SolverUpdate(rule.d);
  }
  forward_backward(a);      // the diffs the step after the rewire will consume
  // what the rewire must leave: computed from the blob as it is now
  const vector<Dtype> w_old = copy_of(wa.cpu_data(), count), d_old = copy_of(wa.cpu_diff(), count);
  vector<vector<Dtype> > h_old(4);
  for (int k = 0; k < 4; ++k) h_old[k] = copy_of(a.layer->solver_history()[k]->cpu_data(), a.layer->solver_history()[k]->count());
  const long keep = n - n / 3;
  vector<long> order((size_t)n);
  std::iota(order.begin(), order.end(), 0L);
  std::stable_sort(order.begin(), order.end(), [&](long p, long q) { return key_of(w_old[pattern[p]]) > key_of(w_old[pattern[q]]); });
  vector<char> kept((size_t)n, 0);
  for (long i = 0; i < keep; ++i) kept[(size_t)order[(size_t)i]] = 1;
  // the dense score and the initial values; a few scores tie
  vector<Dtype> score((size_t)count), init((size_t)count);
  for (int i = 0; i < count; ++i) {
    score[(size_t)i] = (Dtype)((int)(urand() * 16) / 16.0 - 0.5);
    init[(size_t)i] = (Dtype)(urand() + 0.25) * (urand() < 0.5 ? (Dtype)-1 : (Dtype)1);
  }
  vector<int> cand;
  for (int i = 0; i < count; ++i)
    if (!in_pattern[(size_t)i]) cand.push_back(i);
  const long grow = std::min<long>(n / 3, (long)cand.size());
  std::stable_sort(cand.begin(), cand.end(), [&](int p, int q) { return key_of(score[(size_t)p]) > key_of(score[(size_t)q]); });
  vector<char> is_grown((size_t)count, 0);
  for (long i = 0; i < grow; ++i) is_grown[(size_t)cand[(size_t)i]] = 1;

  Blob<Dtype> score_blob(vector<int>(1, count)), init_blob(vector<int>(1, count));
  memcpy(score_blob.mutable_cpu_data(), score.data(), sizeof(Dtype) * count);
  memcpy(init_blob.mutable_cpu_data(), init.data(), sizeof(Dtype) * count);
  escoin_prune_desc pd;
  memset(&pd, 0, sizeof(pd));
  pd.mode = ESCOIN_PRUNE_KEEP;
  pd.keep = keep;
  escoin_rewire_desc rd;
  memset(&rd, 0, sizeof(rd));
  rd.drop = &pd;
  rd.grow = grow;
  rd.score = brew == Caffe::GPU ? score_blob.gpu_data() : score_blob.cpu_data();
  rd.init = brew == Caffe::GPU ? init_blob.gpu_data() : init_blob.cpu_data();
  a.layer->Rewire(rd);

  const long new_nnz = keep + grow;
  int zeroed = 0, nonzero_diff_dropped = 0;
  if (a.layer->nnz() != new_nnz || a.layer->plan_stat("rewire_last_dropped") != n - keep || a.layer->plan_stat("rewire_last_grown") != grow) ++bad;
  vector<Dtype> w_want = w_old, d_want = d_old;
  for (long e = 0; e < n; ++e)
    if (!kept[(size_t)e]) {
      w_want[pattern[e]] = (Dtype)0, d_want[pattern[e]] = (Dtype)0;      // +0: all bits clear
      ++zeroed;
      nonzero_diff_dropped += d_old[pattern[e]] != 0;
    }
  for (int i = 0; i < count; ++i)
    if (is_grown[(size_t)i]) w_want[(size_t)i] = init[(size_t)i];
  if (!same(wa.cpu_data(), w_want.data(), count) || !same(wa.cpu_diff(), d_want.data(), count)) ++bad;
  // histories: the weights' re-indexed into zeros, the bias' untouched.  The new pattern in position order:
  vector<vector<Dtype> > h_want(4);
  {
    long e = 0;
    for (int i = 0; i < count; ++i) {
      if (in_pattern[(size_t)i]) {
        if (kept[(size_t)e])
          for (int k = 0; k < 2; ++k) h_want[k].push_back(h_old[k][(size_t)e]);
        ++e;
      } else if (is_grown[(size_t)i]) {
        for (int k = 0; k < 2; ++k) h_want[k].push_back((Dtype)0);
      }
    }
  }
  h_want[2] = h_old[2], h_want[3] = h_old[3];
  int live_history = 0;
  for (int k = 0; k < 4; ++k) {
    const Blob<Dtype> &h = *a.layer->solver_history()[k];
    if (h.count() != (int)h_want[k].size() || !same(h.cpu_data(), h_want[k].data(), h_want[k].size())) ++bad;
    if (k == 0)
      for (int i = 0; i < h.count(); ++i) live_history += h.cpu_data()[i] != 0;
  }
  // the rebuilt layer: the blob as it must be, the same diffs and bias, hand-re-indexed histories
  Blob<Dtype> &wb = *b.layer->blobs()[0], &bb = *b.layer->blobs()[1];
  memcpy(wb.mutable_cpu_data(), w_want.data(), sizeof(Dtype) * count);
  memcpy(wb.mutable_cpu_diff(), d_want.data(), sizeof(Dtype) * count);
  memcpy(bb.mutable_cpu_data(), ba.cpu_data(), sizeof(Dtype) * ba.count());
  memcpy(bb.mutable_cpu_diff(), ba.cpu_diff(), sizeof(Dtype) * ba.count());
  b.layer->WeightAlign();
  if (b.layer->nnz() != new_nnz) ++bad;
  b.layer->histories().assign(4, shared_ptr<Blob<Dtype> >());
  for (int k = 0; k < 4; ++k) {
    b.layer->histories()[k].reset(new Blob<Dtype>(vector<int>(1, (int)h_want[k].size())));
    if (!h_want[k].empty()) memcpy(b.layer->histories()[k]->mutable_cpu_data(), h_want[k].data(), sizeof(Dtype) * h_want[k].size());
  }
  a.layer->SolverUpdate(rule.d);
  b.layer->SolverUpdate(rule.d);
  if (!same(wa.cpu_data(), wb.cpu_data(), count) || !same(ba.cpu_data(), bb.cpu_data(), ba.count())) ++bad;
  if (!same(wa.cpu_diff(), wb.cpu_diff(), count)) ++bad;
  const bool adam = rule.d.type == ESCOIN_SOLVER_ADAM;
  for (int k = 0; k < (adam ? 4 : 3); ++k) {
    if (k == 1 && !adam) continue;
    const Blob<Dtype> &ha = *a.layer->solver_history()[k], &hb = *b.layer->solver_history()[k];
    if (ha.count() != hb.count() || !same(ha.cpu_data(), hb.cpu_data(), ha.count())) ++bad;
  }
  a.layer->Forward(a.bottom, a.top);
  b.layer->Forward(b.bottom, b.top);
  if (a.top[0]->count() != b.top[0]->count() || !same(a.top[0]->cpu_data(), b.top[0]->cpu_data(), a.top[0]->count())) ++bad;
  int moved = 0;
  for (int i = 0; i < count; ++i) moved += wa.cpu_data()[i] != w_want[i];
  // a WeightAlign from the blob reproduces the rewired pattern
  const vector<Dtype> top_before = copy_of(a.top[0]->cpu_data(), a.top[0]->count());
  a.layer->WeightAlign();
  int realign_bad = a.layer->nnz() != new_nnz;
  a.layer->Forward(a.bottom, a.top);
  realign_bad += !same(a.top[0]->cpu_data(), top_before.data(), top_before.size());
  const bool ok = bad == 0 && realign_bad == 0 && zeroed == n - keep && zeroed > 0 && grow > 0 && live_history > 0 &&
                  nonzero_diff_dropped > 0 && moved > 0;
  printf("%s %s %-10s %-5s nnz %ld -> %ld  differing %d  zeroed %d  grown %ld  live-history %d  realign-differing %d  %s\n",
         sizeof(Dtype) == 8 ? "double" : "float", brew == Caffe::GPU ? "GPU" : "CPU", c.name, rule.name, n, new_nnz, bad, zeroed,
         grow, live_history, realign_bad, ok ? "OK" : "FAIL");
  return ok ? 0 : 1;
}

int main(int argc, char **argv) {
  const bool cpu_only = argc > 1 && !strcmp(argv[1], "--cpu-only");
  const Rule rules[] = {
      {"sgd", make_rule(ESCOIN_SOLVER_SGD, ESCOIN_REG_L2, 0.01)},
      {"adam", make_rule(ESCOIN_SOLVER_ADAM, ESCOIN_REG_L2, 0.001)},
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
