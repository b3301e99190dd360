// caffe_shim.hpp -- header-only mirror of the slice of Caffe's C++ API that the sparse
// convolution path sits behind, so that ConvolutionLayer<Dtype> below could be pasted into a
// Caffe-HIP tree: same class names, method names, argument meaning and (fatal) error behaviour
// as the reference.  It is NOT Caffe: only what the hot path touches exists.
//
//   caffe::Caffe                 include/caffe/common.hpp:102-205   (mode, conv_mode, SetDevice)
//   caffe::SyncedMemory          include/caffe/syncedmem.hpp:56-91, src/caffe/syncedmem.cpp:40-140
//   caffe::Blob<Dtype>           include/caffe/blob.hpp
//   caffe::LayerParameter / ConvolutionParameter   caffe.proto:573-624 as PODs (no protobuf here)
//   caffe::Layer<Dtype>          include/caffe/layer.hpp:33-475 (SetUp, Forward wrapper, WeightAlign)
//   caffe::BaseConvolutionLayer  include/caffe/layers/base_conv_layer.hpp:20-202
//   caffe::ConvolutionLayer      include/caffe/layers/conv_layer.hpp:30-80, conv_layer.cu:8-40
//   caffe::ConvolutionReLULayer  include/caffe/layers/conv_relu_layer.hpp, conv_relu_layer.cu:8-30
//   caffe::InnerProductLayer     include/caffe/layers/inner_product_layer.hpp, inner_product_layer.cpp / .cu
//
// Backward_gpu / Backward_cpu (conv_layer.cu:42-73, conv_layer.cpp:65-99) call the library's pattern-preserving
// backward (escoin_backward[_cpu], include/escoin.h): gradients flow through the CSR's nonzeros only and the weight
// gradient lands at the CSR's positions only, so a fine-tuning step keeps the pruned weights at 0.
//
// Forward_gpu and Forward_cpu both call the C ABI (include/escoin.h): Caffe::GPU mode runs the HIP kernels,
// Caffe::CPU mode the library's host kernel (escoin_forward_cpu; no device is touched, so a CPU-mode net runs on a
// machine without a GPU).  Every class is a template over Dtype = float | double like the reference's
// (INSTANTIATE_CLASS, conv_layer.cpp:102): EscApi<Dtype> below maps the type to the C entry points.
#ifndef ESCOIN_CAFFE_SHIM_HPP_
#define ESCOIN_CAFFE_SHIM_HPP_

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "escoin.h"

// glog-style fatal checks (the reference aborts on every error: device_alternate.hpp:51-78)
#define ESC_CHECK(cond)                                                                     \
  do {                                                                                      \
    if (!(cond)) {                                                                          \
      fprintf(stderr, "Check failed: %s (%s:%d)\n", #cond, __FILE__, __LINE__);             \
      abort();                                                                              \
    }                                                                                       \
  } while (0)
#define ESC_HIP_CHECK(expr)                                                                 \
  do {                                                                                      \
    hipError_t e__ = (expr);                                                                \
    if (e__ != hipSuccess) {                                                                \
      fprintf(stderr, "HIP_CHECK failed: %s: %s (%s:%d)\n", #expr, hipGetErrorString(e__),  \
              __FILE__, __LINE__);                                                          \
      abort();                                                                              \
    }                                                                                       \
  } while (0)
#define ESCOIN_CHECK(expr)                                                                  \
  do {                                                                                      \
    int rc__ = (expr);                                                                      \
    if (rc__ != 0) {                                                                        \
      fprintf(stderr, "ESCOIN_CHECK failed: %s -> %d: %s (%s:%d)\n", #expr, rc__,           \
              escoin_last_error(), __FILE__, __LINE__);                                     \
      abort();                                                                              \
    }                                                                                       \
  } while (0)
#define NOT_IMPLEMENTED                                                                     \
  do {                                                                                      \
    fprintf(stderr, "Not Implemented Yet (%s:%d)\n", __FILE__, __LINE__);                   \
    abort();                                                                                \
  } while (0)

namespace caffe {

using std::shared_ptr;
using std::string;
using std::vector;

// common.hpp:102-205.  Thread-local singleton like the reference (common.cpp:13-19).
class Caffe {
 public:
  enum Brew { CPU, GPU };
  enum ConvMode { LOWERED_GEMM, LOWERED_SPARSE, SCONV, SCONV_PAR };   // common.hpp:112
  static Caffe &Get() {
    static thread_local Caffe instance;
    return instance;
  }
  static Brew mode() { return Get().mode_; }
  static void set_mode(Brew m) { Get().mode_ = m; }
  static ConvMode conv_mode() { return Get().conv_mode_; }
  static void set_conv_mode(ConvMode m) { Get().conv_mode_ = m; }    // common.hpp:161
  static void SetDevice(int device_id) { ESC_HIP_CHECK(hipSetDevice(device_id)); }
  static hipStream_t stream() { return nullptr; }   // every reference launch uses stream 0
  // host threads of CPU mode (0 = all the process may run on): the reference takes OMP_NUM_THREADS for its ICC build's
  // batch loop (conv_layer.cpp:41-43); there is no OpenMP runtime here, so the number is a setting
  static int cpu_threads() { return Get().cpu_threads_; }
  static void set_cpu_threads(int n) { Get().cpu_threads_ = n; }
  // the weight gradient's stage-1 kernel (ESCOIN_WGRAD_*, include/escoin.h option "wgrad_kernel") of the plans layers
  // create from now on; CPU mode has one weight gradient and ignores it
  static int wgrad_kernel() { return Get().wgrad_kernel_; }
  static void set_wgrad_kernel(int k) { Get().wgrad_kernel_ = k; }
  // the data gradient's kernel (ESCOIN_KERNEL_* or ESCOIN_BWD_MFMA, include/escoin.h option "backward_kernel") of the
  // plans layers create from now on; CPU mode has one data gradient and ignores it
  static int backward_kernel() { return Get().backward_kernel_; }
  static void set_backward_kernel(int k) { Get().backward_kernel_ = k; }
  // whether the plans layers create from now on run strided layers on the stride-1 kernels via space-to-depth
  // (include/escoin.h option "s2d"); a layer the option does not serve, and CPU mode, run as without it
  static bool s2d() { return Get().s2d_; }
  static void set_s2d(bool on) { Get().s2d_ = on; }
  // the same for dilated stride-1 layers via space-to-batch (include/escoin.h option "s2b")
  static bool s2b() { return Get().s2b_; }
  static void set_s2b(bool on) { Get().s2b_ = on; }
  // the same for inner-product layers (one pixel, a 1x1 kernel) via batch-to-space (include/escoin.h option "b2s")
  static bool b2s() { return Get().b2s_; }
  static void set_b2s(bool on) { Get().b2s_ = on; }
  // whether the plans layers create from now on compute the weight gradient of pointwise layers (1x1, pad 0; inner-product
  // layers through "b2s") by the pointwise kernel (include/escoin.h option "wgrad_pointwise"); a layer the option does not
  // serve, a forced wgrad_kernel, and CPU mode, run as without it
  static bool wgrad_pointwise() { return Get().wgrad_pointwise_; }
  static void set_wgrad_pointwise(bool on) { Get().wgrad_pointwise_ = on; }

 private:
  // the reference leaves conv_mode_ uninitialised; here it defaults to SCONV_PAR
  Caffe() : mode_(CPU), conv_mode_(SCONV_PAR), cpu_threads_(0), wgrad_kernel_(ESCOIN_WGRAD_AUTO), backward_kernel_(ESCOIN_KERNEL_AUTO), s2d_(false), s2b_(false), b2s_(false), wgrad_pointwise_(false) {}
  Brew mode_;
  ConvMode conv_mode_;
  int cpu_threads_;
  int wgrad_kernel_;
  int backward_kernel_;
  bool s2d_;
  bool s2b_;
  bool b2s_;
  bool wgrad_pointwise_;
};

// Dtype -> C ABI.  The float entry points are the unsuffixed ones, double the _f64 twins (include/escoin.h).
template <typename Dtype> struct EscApi;
template <> struct EscApi<float> {
  static int weight_align(escoin_plan *p, const float *w, int on_dev, void *s) { return escoin_weight_align(p, w, on_dev, s); }
  static int get_csr(const escoin_plan *p, int *rp, int *ci, float *v) { return escoin_plan_get_csr(p, rp, ci, v, 0); }
  static int weight_align_cpu(escoin_plan *p, const float *w) { return escoin_weight_align_cpu(p, w); }
  static int forward(escoin_plan *p, const float *b, const float *bias, float *t, int n, void *s) { return escoin_forward(p, b, bias, t, n, s); }
  static int forward_cpu(escoin_plan *p, const float *b, const float *bias, float *t, int n, int threads) { return escoin_forward_cpu(p, b, bias, t, n, threads); }
  static int backward(escoin_plan *p, const float *b, const float *t, const float *td, float *bd, float *wd, float *bsd, int n, void *s) { return escoin_backward(p, b, t, td, bd, wd, bsd, n, s); }
  static int backward_cpu(escoin_plan *p, const float *b, const float *t, const float *td, float *bd, float *wd, float *bsd, int n, int threads) { return escoin_backward_cpu(p, b, t, td, bd, wd, bsd, n, threads); }
  static int update_values(escoin_plan *p, const float *w, int on_dev, void *s) { return escoin_update_values(p, w, on_dev, s); }
  static int update_values_cpu(escoin_plan *p, const float *w) { return escoin_update_values_cpu(p, w); }
  static int solver_step(escoin_plan *p, const escoin_solver_desc *d, float *g, float *h, float *h2, float *w, void *s) { return escoin_solver_step(p, d, g, h, h2, w, s); }
  static int solver_step_cpu(escoin_plan *p, const escoin_solver_desc *d, float *g, float *h, float *h2, float *w) { return escoin_solver_step_cpu(p, d, g, h, h2, w); }
  static int solver_array_step(const escoin_solver_desc *d, long n, float *w, float *g, float *h, float *h2, void *s) { return escoin_solver_array_step(d, n, w, g, h, h2, s); }
  static int solver_array_step_cpu(const escoin_solver_desc *d, long n, float *w, float *g, float *h, float *h2) { return escoin_solver_array_step_cpu(d, n, w, g, h, h2); }
  static int dense_wgrad(escoin_plan *p, const float *b, const float *t, const float *td, float *dd, int n, int acc, void *s) { return escoin_dense_wgrad(p, b, t, td, dd, n, acc, s); }
  static int dense_wgrad_cpu(escoin_plan *p, const float *b, const float *t, const float *td, float *dd, int n, int acc, int threads) { return escoin_dense_wgrad_cpu(p, b, t, td, dd, n, acc, threads); }
};
template <> struct EscApi<double> {
  static int weight_align(escoin_plan *p, const double *w, int on_dev, void *s) { return escoin_weight_align_f64(p, w, on_dev, s); }
  static int get_csr(const escoin_plan *p, int *rp, int *ci, double *v) { return escoin_plan_get_csr_f64(p, rp, ci, v, 0); }
  static int weight_align_cpu(escoin_plan *p, const double *w) { return escoin_weight_align_cpu_f64(p, w); }
  static int forward(escoin_plan *p, const double *b, const double *bias, double *t, int n, void *s) { return escoin_forward_f64(p, b, bias, t, n, s); }
  static int forward_cpu(escoin_plan *p, const double *b, const double *bias, double *t, int n, int threads) { return escoin_forward_cpu_f64(p, b, bias, t, n, threads); }
  static int backward(escoin_plan *p, const double *b, const double *t, const double *td, double *bd, double *wd, double *bsd, int n, void *s) { return escoin_backward_f64(p, b, t, td, bd, wd, bsd, n, s); }
  static int backward_cpu(escoin_plan *p, const double *b, const double *t, const double *td, double *bd, double *wd, double *bsd, int n, int threads) { return escoin_backward_cpu_f64(p, b, t, td, bd, wd, bsd, n, threads); }
  static int update_values(escoin_plan *p, const double *w, int on_dev, void *s) { return escoin_update_values_f64(p, w, on_dev, s); }
  static int update_values_cpu(escoin_plan *p, const double *w) { return escoin_update_values_cpu_f64(p, w); }
  static int solver_step(escoin_plan *p, const escoin_solver_desc *d, double *g, double *h, double *h2, double *w, void *s) { return escoin_solver_step_f64(p, d, g, h, h2, w, s); }
  static int solver_step_cpu(escoin_plan *p, const escoin_solver_desc *d, double *g, double *h, double *h2, double *w) { return escoin_solver_step_cpu_f64(p, d, g, h, h2, w); }
  static int solver_array_step(const escoin_solver_desc *d, long n, double *w, double *g, double *h, double *h2, void *s) { return escoin_solver_array_step_f64(d, n, w, g, h, h2, s); }
  static int solver_array_step_cpu(const escoin_solver_desc *d, long n, double *w, double *g, double *h, double *h2) { return escoin_solver_array_step_cpu_f64(d, n, w, g, h, h2); }
  static int dense_wgrad(escoin_plan *p, const double *b, const double *t, const double *td, double *dd, int n, int acc, void *s) { return escoin_dense_wgrad_f64(p, b, t, td, dd, n, acc, s); }
  static int dense_wgrad_cpu(escoin_plan *p, const double *b, const double *t, const double *td, double *dd, int n, int acc, int threads) { return escoin_dense_wgrad_cpu_f64(p, b, t, td, dd, n, acc, threads); }
};

// syncedmem.hpp:56-91: lazily mirrored host/device buffer with a head state.
class SyncedMemory {
 public:
  enum SyncedHead { UNINITIALIZED, HEAD_AT_CPU, HEAD_AT_GPU, SYNCED };
  explicit SyncedMemory(size_t size) : cpu_ptr_(nullptr), gpu_ptr_(nullptr), size_(size), head_(UNINITIALIZED) {}
  ~SyncedMemory() {
    if (cpu_ptr_) free(cpu_ptr_);
    if (gpu_ptr_) (void)hipFree(gpu_ptr_);
  }
  const void *cpu_data() { to_cpu(); return cpu_ptr_; }
  const void *gpu_data() { to_gpu(); return gpu_ptr_; }
  void *mutable_cpu_data() { to_cpu(); head_ = HEAD_AT_CPU; return cpu_ptr_; }
  void *mutable_gpu_data() { to_gpu(); head_ = HEAD_AT_GPU; return gpu_ptr_; }
  SyncedHead head() const { return head_; }
  size_t size() const { return size_; }

 private:
  void to_cpu() {   // syncedmem.cpp:40-64
    switch (head_) {
      case UNINITIALIZED:
        cpu_ptr_ = calloc(1, size_ ? size_ : 1);
        ESC_CHECK(cpu_ptr_);
        head_ = HEAD_AT_CPU;
        break;
      case HEAD_AT_GPU:
        if (!cpu_ptr_) { cpu_ptr_ = malloc(size_ ? size_ : 1); ESC_CHECK(cpu_ptr_); }
        ESC_HIP_CHECK(hipMemcpy(cpu_ptr_, gpu_ptr_, size_, hipMemcpyDeviceToHost));
        head_ = SYNCED;
        break;
      default: break;
    }
  }
  void to_gpu() {   // syncedmem.cpp:66-92
    switch (head_) {
      case UNINITIALIZED:
        ESC_HIP_CHECK(hipMalloc(&gpu_ptr_, size_ ? size_ : 1));
        ESC_HIP_CHECK(hipMemset(gpu_ptr_, 0, size_));
        head_ = HEAD_AT_GPU;
        break;
      case HEAD_AT_CPU:
        if (!gpu_ptr_) ESC_HIP_CHECK(hipMalloc(&gpu_ptr_, size_ ? size_ : 1));
        ESC_HIP_CHECK(hipMemcpy(gpu_ptr_, cpu_ptr_, size_, hipMemcpyHostToDevice));
        head_ = SYNCED;
        break;
      default: break;
    }
  }
  void *cpu_ptr_, *gpu_ptr_;
  size_t size_;
  SyncedHead head_;
};

template <typename Dtype>
class Blob {   // blob.hpp (data and diff)
 public:
  Blob() : count_(0), capacity_(0) {}
  explicit Blob(const vector<int> &shape) : count_(0), capacity_(0) { Reshape(shape); }
  Blob(int num, int channels, int height, int width) : count_(0), capacity_(0) {
    Reshape(num, channels, height, width);
  }
  void Reshape(int num, int channels, int height, int width) {
    vector<int> s(4);
    s[0] = num; s[1] = channels; s[2] = height; s[3] = width;
    Reshape(s);
  }
  void Reshape(const vector<int> &shape) {   // blob.cpp: grows, never shrinks
    count_ = 1;
    shape_ = shape;
    for (size_t i = 0; i < shape.size(); ++i) { ESC_CHECK(shape[i] >= 0); count_ *= shape[i]; }
    if (count_ > capacity_) {
      capacity_ = count_;
      data_.reset(new SyncedMemory(capacity_ * sizeof(Dtype)));
      diff_.reset(new SyncedMemory(capacity_ * sizeof(Dtype)));   // blob.cpp:31-33: allocated with the data
    }
  }
  const vector<int> &shape() const { return shape_; }
  int shape(int i) const { return shape_[i < 0 ? i + (int)shape_.size() : i]; }
  int num_axes() const { return (int)shape_.size(); }
  int count() const { return count_; }
  int count(int start, int end) const {
    int c = 1;
    for (int i = start; i < end; ++i) c *= shape(i);
    return c;
  }
  int num() const { return shape(0); }
  int channels() const { return shape(1); }
  int height() const { return shape(2); }
  int width() const { return shape(3); }
  const Dtype *cpu_data() const { ESC_CHECK(data_); return (const Dtype *)data_->cpu_data(); }
  const Dtype *gpu_data() const { ESC_CHECK(data_); return (const Dtype *)data_->gpu_data(); }
  Dtype *mutable_cpu_data() { ESC_CHECK(data_); return (Dtype *)data_->mutable_cpu_data(); }
  Dtype *mutable_gpu_data() { ESC_CHECK(data_); return (Dtype *)data_->mutable_gpu_data(); }
  // blob.hpp:224-229
  const Dtype *cpu_diff() const { ESC_CHECK(diff_); return (const Dtype *)diff_->cpu_data(); }
  const Dtype *gpu_diff() const { ESC_CHECK(diff_); return (const Dtype *)diff_->gpu_data(); }
  Dtype *mutable_cpu_diff() { ESC_CHECK(diff_); return (Dtype *)diff_->mutable_cpu_data(); }
  Dtype *mutable_gpu_diff() { ESC_CHECK(diff_); return (Dtype *)diff_->mutable_gpu_data(); }

 private:
  shared_ptr<SyncedMemory> data_, diff_;
  vector<int> shape_;
  int count_, capacity_;
};

// caffe.proto:573-624 as a POD (no protobuf runtime for C++ in this environment)
struct ConvolutionParameter {
  int num_output = 0;
  bool bias_term = true;
  int pad_h = 0, pad_w = 0;
  int kernel_h = 0, kernel_w = 0;
  int stride_h = 1, stride_w = 1;
  int dilation = 1;
  int group = 1;
};
// caffe.proto InnerProductParameter as a POD
struct InnerProductParameter {
  int num_output = 0;
  bool bias_term = true;
  int axis = 1;             // the first axis of the inner product: K = count from it
  bool transpose = false;   // not supported: InnerProductLayer aborts
};
struct LayerParameter {
  string name, type;
  ConvolutionParameter convolution_param;
  InnerProductParameter inner_product_param;
};

template <typename Dtype>
class Layer {   // layer.hpp:33-475
 public:
  explicit Layer(const LayerParameter &param) : layer_param_(param), test_time_(0) {}
  virtual ~Layer() {}
  void SetUp(const vector<Blob<Dtype> *> &bottom, const vector<Blob<Dtype> *> &top) {   // :69-77
    ESC_CHECK((int)bottom.size() >= MinBottomBlobs());
    ESC_CHECK((int)top.size() >= MinTopBlobs());
    if (EqualNumBottomTopBlobs()) ESC_CHECK(bottom.size() == top.size());
    LayerSetUp(bottom, top);
    Reshape(bottom, top);
  }
  virtual void LayerSetUp(const vector<Blob<Dtype> *> &, const vector<Blob<Dtype> *> &) {}
  virtual void Reshape(const vector<Blob<Dtype> *> &bottom, const vector<Blob<Dtype> *> &top) = 0;
  virtual void WeightAlign() {}   // layer.hpp:97-98, called by Net::CopyTrainedLayersFrom (net.cpp:819)
  // What a solver calls after ApplyUpdate (Net::Update, net.cpp) on every layer: the learnable blobs changed, the
  // sparsity pattern did not.  The reference has no counterpart -- it would have to WeightAlign again.
  virtual void WeightUpdate() {}
  // SGDSolver::ApplyUpdate's per-parameter work (Normalize, Regularize, ComputeUpdateValue) and Net::Update for this
  // layer's learnable blobs in one call (include/escoin.h, "Solver step"); a layer without learnable blobs does nothing.
  virtual void SolverUpdate(const escoin_solver_desc &) {}
  // Magnitude pruning of this layer's weights (include/escoin.h, "Pruning"): what a solver with a pruning schedule calls
  // between two iterations; a layer without a sparse plan does nothing.
  virtual void Prune(const escoin_prune_desc &) {}
  // Drop-and-grow rewiring of this layer's weights (include/escoin.h, "Rewiring"): what a solver with a dynamic-sparse
  // schedule (RigL, SET) calls between two iterations; a layer without a sparse plan does nothing.
  virtual void Rewire(const escoin_rewire_desc &) {}
  // layer.hpp:435-475: Reshape every call, mode switch, per-layer forward time in microseconds
  inline Dtype Forward(const vector<Blob<Dtype> *> &bottom, const vector<Blob<Dtype> *> &top) {
    Reshape(bottom, top);
    hipEvent_t e0, e1;
    const bool gpu = Caffe::mode() == Caffe::GPU;
    if (gpu) {
      ESC_HIP_CHECK(hipEventCreate(&e0));
      ESC_HIP_CHECK(hipEventCreate(&e1));
      ESC_HIP_CHECK(hipEventRecord(e0, Caffe::stream()));
    }
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    switch (Caffe::mode()) {
      case Caffe::CPU: Forward_cpu(bottom, top); break;
      case Caffe::GPU: Forward_gpu(bottom, top); break;
    }
    if (!gpu) test_time_ = std::chrono::duration<float, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (gpu) {
      ESC_HIP_CHECK(hipEventRecord(e1, Caffe::stream()));
      ESC_HIP_CHECK(hipEventSynchronize(e1));
      float ms = 0;
      ESC_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
      test_time_ = ms * 1000.f;
      ESC_HIP_CHECK(hipEventDestroy(e0));
      ESC_HIP_CHECK(hipEventDestroy(e1));
    }
    return 0;
  }
  // layer.hpp:478-491: the mode switch; the bottoms' diffs for propagate_down[i], the parameters' diffs accumulated
  // for param_propagate_down
  inline void Backward(const vector<Blob<Dtype> *> &top, const vector<bool> &propagate_down,
                       const vector<Blob<Dtype> *> &bottom) {
    switch (Caffe::mode()) {
      case Caffe::CPU: Backward_cpu(top, propagate_down, bottom); break;
      case Caffe::GPU: Backward_gpu(top, propagate_down, bottom); break;
    }
  }
  // layer.hpp:287-300
  inline bool param_propagate_down(const int param_id) {
    return (param_propagate_down_.size() > (size_t)param_id) ? param_propagate_down_[param_id] : false;
  }
  inline void set_param_propagate_down(const int param_id, const bool value) {
    if (param_propagate_down_.size() <= (size_t)param_id) param_propagate_down_.resize(param_id + 1, true);
    param_propagate_down_[param_id] = value;
  }
  vector<shared_ptr<Blob<Dtype> > > &blobs() { return blobs_; }
  const LayerParameter &layer_param() const { return layer_param_; }
  virtual inline const char *type() const { return ""; }
  virtual inline int MinBottomBlobs() const { return -1; }
  virtual inline int MinTopBlobs() const { return -1; }
  virtual inline bool EqualNumBottomTopBlobs() const { return false; }
  float get_time() const { return test_time_; }   // layer.hpp:99

 protected:
  virtual void Forward_cpu(const vector<Blob<Dtype> *> &bottom, const vector<Blob<Dtype> *> &top) = 0;
  virtual void Forward_gpu(const vector<Blob<Dtype> *> &bottom, const vector<Blob<Dtype> *> &top) {
    Forward_cpu(bottom, top);
  }
  // layer.hpp:330-345 (Backward_cpu is pure there; here a layer without a backward aborts when asked for one)
  virtual void Backward_cpu(const vector<Blob<Dtype> *> &, const vector<bool> &, const vector<Blob<Dtype> *> &) {
    NOT_IMPLEMENTED;
  }
  virtual void Backward_gpu(const vector<Blob<Dtype> *> &top, const vector<bool> &propagate_down,
                            const vector<Blob<Dtype> *> &bottom) {
    Backward_cpu(top, propagate_down, bottom);
  }
  LayerParameter layer_param_;
  vector<shared_ptr<Blob<Dtype> > > blobs_;
  vector<bool> param_propagate_down_;   // layer.hpp:434
  float test_time_;
};

template <typename Dtype>
class BaseConvolutionLayer : public Layer<Dtype> {   // base_conv_layer.hpp:20-202
 public:
  explicit BaseConvolutionLayer(const LayerParameter &param)
      : Layer<Dtype>(param), plan_(nullptr), num_(0), channels_(0), group_(1), num_output_(0),
        bias_term_(true), fuse_relu_(false), planned_num_(0) {}
  virtual ~BaseConvolutionLayer() { if (plan_) escoin_plan_destroy(plan_); }   // base_conv_layer.cpp:16-42

  // base_conv_layer.cpp:276-446: parse the conv params, allocate and shape blobs_
  virtual void LayerSetUp(const vector<Blob<Dtype> *> &bottom, const vector<Blob<Dtype> *> &) {
    const ConvolutionParameter &cp = this->layer_param_.convolution_param;
    ESC_CHECK(bottom[0]->num_axes() == 4);
    ESC_CHECK(cp.kernel_h > 0 && cp.kernel_w > 0 && cp.num_output > 0);
    channels_ = bottom[0]->shape(1);
    num_output_ = cp.num_output;
    group_ = cp.group;
    bias_term_ = cp.bias_term;
    ESC_CHECK(channels_ % group_ == 0);     // :393
    ESC_CHECK(num_output_ % group_ == 0);   // :395
    this->blobs_.resize(bias_term_ ? 2 : 1);   // :423-427
    vector<int> wshape(4);
    wshape[0] = num_output_; wshape[1] = channels_ / group_; wshape[2] = cp.kernel_h; wshape[3] = cp.kernel_w;
    this->blobs_[0].reset(new Blob<Dtype>(wshape));
    if (bias_term_) this->blobs_[1].reset(new Blob<Dtype>(vector<int>(1, num_output_)));
    this->param_propagate_down_.resize(this->blobs_.size(), true);   // :445
  }

  // base_conv_layer.cpp:449-530: output shape, all bottoms identical, top reshape
  virtual void Reshape(const vector<Blob<Dtype> *> &bottom, const vector<Blob<Dtype> *> &top) {
    const ConvolutionParameter &cp = this->layer_param_.convolution_param;
    num_ = bottom[0]->shape(0);
    ESC_CHECK(bottom[0]->shape(1) == channels_);
    for (size_t i = 1; i < bottom.size(); ++i) ESC_CHECK(bottom[0]->shape() == bottom[i]->shape());   // :458-461
    escoin_conv_desc d = desc(bottom[0], cp);
    int oh = 0, ow = 0;
    ESCOIN_CHECK(escoin_out_shape(&d, &oh, &ow));   // compute_output_shape, conv_layer.cpp:8-22
    for (size_t i = 0; i < top.size(); ++i) top[i]->Reshape(num_, num_output_, oh, ow);
    bottom_dim_ = bottom[0]->count(1, 4);
    top_dim_ = top[0]->count(1, 4);
    plan_for(d);
  }

 protected:
  // The plan of descriptor d: the one the layer has where only the batch shrank, a fresh one otherwise.
  void plan_for(const escoin_conv_desc &d) {
    escoin_conv_desc same_but_n = d;
    same_but_n.N = plan_ ? desc_.N : d.N;
    const bool reusable = plan_ && d.N <= desc_.N && memcmp(&same_but_n, &desc_, sizeof(d)) == 0;
    if (!reusable) {
      // geometry changed, batch grew past the planned one, or first call: a fresh plan.  The
      // reference's Reshape leaves the CSR blobs alone (they depend on the weights only) but its
      // stretched indices and padded buffer go stale until the next WeightAlign; here a layer
      // that was aligned is re-aligned from blobs_[0] on the spot, so Forward keeps working.
      escoin_plan *fresh = nullptr;
      ESCOIN_CHECK(escoin_plan_create(&d, &fresh));
      ESCOIN_CHECK(escoin_plan_set_option(fresh, "wgrad_kernel", Caffe::wgrad_kernel()));
      ESCOIN_CHECK(escoin_plan_set_option(fresh, "backward_kernel", Caffe::backward_kernel()));
      // (a Deconvolution layer's plan is option "deconv"'s, which does not combine with the other derived-plan options)
      ESCOIN_CHECK(escoin_plan_set_option(fresh, "deconv", deconv_ ? 1 : 0));
      ESCOIN_CHECK(escoin_plan_set_option(fresh, "s2d", Caffe::s2d() && !deconv_ ? 1 : 0));
      ESCOIN_CHECK(escoin_plan_set_option(fresh, "s2b", Caffe::s2b() && !deconv_ ? 1 : 0));
      ESCOIN_CHECK(escoin_plan_set_option(fresh, "b2s", Caffe::b2s() && !deconv_ ? 1 : 0));
      ESCOIN_CHECK(escoin_plan_set_option(fresh, "wgrad_pointwise", Caffe::wgrad_pointwise() ? 1 : 0));
      if (plan_) escoin_plan_destroy(plan_);
      plan_ = fresh;
      desc_ = d;
      const bool was_aligned = aligned_;
      aligned_ = false;
      if (was_aligned) WeightAlign();
    }
  }

 public:
  // base_conv_layer.cpp:46-273: dense blobs_[0] -> CSR (+ the device weight streams), once
  virtual void WeightAlign() {
    ESC_CHECK(plan_ != nullptr);   // SetUp must have run
    // Caffe::ConvMode and ESCOIN_CONV_MODE_* share their values (common.hpp:112).  The reference's
    // WeightAlign only builds the CSR for the sparse modes and leaves LOWERED_GEMM alone
    // (base_conv_layer.cpp:49-53); here every mode is served from the aligned plan.
    ESCOIN_CHECK(escoin_plan_set_option(plan_, "conv_mode", (int)Caffe::conv_mode()));
    aligned_mode_ = Caffe::conv_mode();
    // GPU mode: CSR + the device weight streams / generated code (CSR branch of base_conv_layer.cpp:109-273).
    // CPU mode: the host CSR only (:46-107) -- no device is touched; a later Forward in GPU mode aligns the device
    // side on the spot (forward_gpu_sconv_par below).
    if (Caffe::mode() == Caffe::GPU) {
      ESCOIN_CHECK(EscApi<Dtype>::weight_align(plan_, this->blobs_[0]->gpu_data(), 1, Caffe::stream()));
      aligned_on_device_ = true;
    } else {
      ESCOIN_CHECK(EscApi<Dtype>::weight_align_cpu(plan_, this->blobs_[0]->cpu_data()));
      aligned_on_device_ = false;
    }
    aligned_ = true;
    history_.clear();   // SolverUpdate's histories are per CSR entry of THIS alignment
  }

  // After a solver step that kept the pattern (the masked gradient of Backward does): the new values of blobs_[0] go
  // into the aligned plan in place (include/escoin.h, "Weight updates") -- no CSR rebuild, no code generation, no
  // allocation, the backward state stays.  GPU mode reads the device blob, asynchronously on Caffe::stream(); CPU mode
  // the host blob, and updates the device side too if the plan has one.  A layer that is not aligned yet, or that was
  // aligned in CPU mode and now runs in GPU mode, aligns.
  virtual void WeightUpdate() {
    ESC_CHECK(plan_ != nullptr);
    if (!aligned_ || (Caffe::mode() == Caffe::GPU && !aligned_on_device_)) {
      WeightAlign();
      return;
    }
    if (Caffe::mode() == Caffe::GPU)
      ESCOIN_CHECK(EscApi<Dtype>::update_values(plan_, this->blobs_[0]->gpu_data(), 1, Caffe::stream()));
    else if (aligned_on_device_)
      ESCOIN_CHECK(EscApi<Dtype>::update_values(plan_, this->blobs_[0]->cpu_data(), 0, Caffe::stream()));
    else
      ESCOIN_CHECK(EscApi<Dtype>::update_values_cpu(plan_, this->blobs_[0]->cpu_data()));
  }

  // SGDSolver::ComputeUpdateValue + Net::Update of this layer as one fused call per blob (include/escoin.h, "Solver
  // step"): blobs_[0] through escoin_solver_step on the dense diff -- read and cleared at the pattern, the new values
  // written into the blob's data at the pattern AND into every copy the plan computes from, so no WeightUpdate follows
  // -- and blobs_[1] through the array step.  `rule` is the solver's rule for both blobs; its diff_is_dense and
  // clear_diff are set here.  The histories are layer-owned: for blobs_[0] compact (nnz elements in the plan's CSR order),
  // created zeroed on first use and dropped by every WeightAlign / WeightAlignFrom (the entries of a new alignment are
  // other weights, whether or not nnz changed; a solver that re-aligns mid-training restarts this layer's momentum --
  // Prune() below shrinks the pattern WITHOUT that: it carries the histories over through the entry map).  The brew
  // picks host or device pointers (a rule.rate_dev must match it); a plan that has a device side is stepped on the device in either brew, which keeps
  // both sides current.  A layer that is not aligned yet aligns first.
  virtual void SolverUpdate(const escoin_solver_desc &rule) {
    ESC_CHECK(plan_ != nullptr);
    if (!aligned_ || (Caffe::mode() == Caffe::GPU && !aligned_on_device_)) WeightAlign();
    escoin_solver_desc d = rule;
    d.diff_is_dense = 1;
    d.clear_diff = 1;
    const bool adam = rule.type == ESCOIN_SOLVER_ADAM;
    const long n = nnz();
    if (history_.empty()) {
      history_.assign(4, shared_ptr<Blob<Dtype> >());
      for (int k = 0; k < 4; ++k) history_[k].reset(new Blob<Dtype>(vector<int>(1, k < 2 ? (int)n : (bias_term_ ? num_output_ : 0))));
    }
    Blob<Dtype> &w = *this->blobs_[0];
    if (aligned_on_device_) {
      ESCOIN_CHECK(EscApi<Dtype>::solver_step(plan_, &d, w.mutable_gpu_diff(), history_[0]->mutable_gpu_data(),
                                              adam ? history_[1]->mutable_gpu_data() : nullptr, w.mutable_gpu_data(), Caffe::stream()));
      if (bias_term_) {
        Blob<Dtype> &b = *this->blobs_[1];
        ESCOIN_CHECK(EscApi<Dtype>::solver_array_step(&d, b.count(), b.mutable_gpu_data(), b.mutable_gpu_diff(), history_[2]->mutable_gpu_data(),
                                                      adam ? history_[3]->mutable_gpu_data() : nullptr, Caffe::stream()));
      }
    } else {
      ESCOIN_CHECK(EscApi<Dtype>::solver_step_cpu(plan_, &d, w.mutable_cpu_diff(), history_[0]->mutable_cpu_data(),
                                                  adam ? history_[1]->mutable_cpu_data() : nullptr, w.mutable_cpu_data()));
      if (bias_term_) {
        Blob<Dtype> &b = *this->blobs_[1];
        ESCOIN_CHECK(EscApi<Dtype>::solver_array_step_cpu(&d, b.count(), b.mutable_cpu_data(), b.mutable_cpu_diff(), history_[2]->mutable_cpu_data(),
                                                          adam ? history_[3]->mutable_cpu_data() : nullptr));
      }
    }
  }

  // Prunes the aligned plan in place (include/escoin.h, "Pruning") and keeps everything that is indexed by CSR entry in
  // step: the weights' histories are compacted through the entry map instead of being cleared (momentum survives a
  // pruning step), and the dropped positions of blobs_[0] -- data and diff -- become +0, so that the blob and the plan
  // agree and a later WeightAlign from the blob reproduces the pattern.  The bias histories are not touched.  A plan that
  // has a device side is pruned on the device in either brew (rule.score, if any, must then be a device pointer;
  // otherwise a host pointer).  Synchronises; not for a captured graph.  A layer that is not aligned yet aligns first.
  virtual void Prune(const escoin_prune_desc &rule) {
    ESC_CHECK(plan_ != nullptr);
    if (!aligned_ || (Caffe::mode() == Caffe::GPU && !aligned_on_device_)) WeightAlign();
    const long n = nnz();
    if (n == 0) return;
    const int mg = num_output_ / group_, kdim = (channels_ / group_) * desc_.KH * desc_.KW;
    vector<int> rowptr((size_t)group_ * (mg + 1)), colidx((size_t)n);
    ESCOIN_CHECK(escoin_plan_get_csr(plan_, rowptr.data(), colidx.data(), nullptr, 0));    // the OLD pattern
    vector<long> per_group(group_);
    for (int g = 0; g < group_; ++g) per_group[g] = escoin_plan_nnz(plan_, g);
    Blob<int> map(vector<int>(1, (int)n));
    long kept = 0;
    if (aligned_on_device_)
      ESCOIN_CHECK(escoin_plan_prune(plan_, &rule, map.mutable_gpu_data(), &kept, Caffe::stream()));
    else
      ESCOIN_CHECK(escoin_plan_prune_cpu(plan_, &rule, map.mutable_cpu_data(), &kept));
    if (kept == n) return;
    const int *m = map.cpu_data();
    for (size_t k = 0; k < history_.size() && k < 2; ++k) {
      shared_ptr<Blob<Dtype> > fresh(new Blob<Dtype>(vector<int>(1, (int)kept)));
      if (aligned_on_device_)
        ESCOIN_CHECK(escoin_compact_entries(map.gpu_data(), n, (int)sizeof(Dtype), history_[k]->gpu_data(), fresh->mutable_gpu_data(), 1, Caffe::stream()));
      else
        ESCOIN_CHECK(escoin_compact_entries(m, n, (int)sizeof(Dtype), history_[k]->cpu_data(), fresh->mutable_cpu_data(), 0, nullptr));
      history_[k] = fresh;     // (the old blob's release waits for the device)
    }
    Blob<Dtype> &w = *this->blobs_[0];
    Dtype *data = w.mutable_cpu_data(), *diff = w.mutable_cpu_diff();
    long e = 0;
    for (int g = 0; g < group_; ++g) {
      const int *rp = rowptr.data() + (size_t)g * (mg + 1);
      const long base = e;
      for (int r = 0; r < mg; ++r)
        for (int j = rp[r]; j < rp[r + 1]; ++j, ++e)
          if (m[e] < 0) {
            const size_t at = ((size_t)g * mg + r) * kdim + (size_t)colidx[(size_t)(base + j)];
            data[at] = (Dtype)0;
            diff[at] = (Dtype)0;
          }
      ESC_CHECK(e - base == per_group[g]);
    }
  }
  // Rewires the aligned plan in place (include/escoin.h, "Rewiring") -- drop and grow with ONE re-align -- and keeps
  // everything that is indexed by CSR entry in step: the weights' histories travel through the entry map into zeroed
  // arrays of the new size (kept entries keep their momentum, grown entries start at zero), the dropped positions of
  // blobs_[0] -- data and diff -- become +0, and the grown positions of blobs_[0]'s data take the grown values (+0, or
  // rule.init's), so that the blob and the plan agree; with nonzero grown values a later WeightAlign from the blob
  // reproduces the pattern.  The bias histories are not touched.  A plan that has a device side is rewired on the
  // device in either brew (rule.score, rule.init and rule.drop->score, if any, must then be device pointers; otherwise
  // host pointers).  Synchronises; not for a captured graph.  A layer that is not aligned yet aligns first.
  virtual void Rewire(const escoin_rewire_desc &rule) {
    ESC_CHECK(plan_ != nullptr);
    if (!aligned_ || (Caffe::mode() == Caffe::GPU && !aligned_on_device_)) WeightAlign();
    const long n = nnz();
    const int mg = num_output_ / group_, kdim = (channels_ / group_) * desc_.KH * desc_.KW;
    // the positions in blobs_[0] of a CSR's entries, in its order
    auto positions = [&](long count, vector<Dtype> *values) {
      vector<int> rowptr((size_t)group_ * (mg + 1)), colidx((size_t)count);
      if (values) values->resize((size_t)count);
      ESCOIN_CHECK(EscApi<Dtype>::get_csr(plan_, rowptr.data(), colidx.data(), values ? values->data() : nullptr));
      vector<size_t> pos;
      long base = 0;
      for (int g = 0; g < group_; ++g) {
        const int *rp = rowptr.data() + (size_t)g * (mg + 1);
        for (int r = 0; r < mg; ++r)
          for (int j = rp[r]; j < rp[r + 1]; ++j) pos.push_back(((size_t)g * mg + r) * kdim + (size_t)colidx[(size_t)(base + j)]);
        base += rp[mg];
      }
      ESC_CHECK((long)pos.size() == count);
      return pos;
    };
    const vector<size_t> old_pos = positions(n, nullptr);       // the OLD pattern
    Blob<int> map(vector<int>(1, (int)std::max<long>(n, 1))), grown(vector<int>(1, (int)std::max<long>(rule.grow, 1)));
    long new_nnz = 0, n_grown = 0;
    if (aligned_on_device_)
      ESCOIN_CHECK(escoin_plan_rewire(plan_, &rule, map.mutable_gpu_data(), grown.mutable_gpu_data(), &new_nnz, &n_grown, Caffe::stream()));
    else
      ESCOIN_CHECK(escoin_plan_rewire_cpu(plan_, &rule, map.mutable_cpu_data(), grown.mutable_cpu_data(), &new_nnz, &n_grown));
    if (escoin_plan_stat(plan_, "rewire_last_dropped") == 0 && n_grown == 0) return;       // the plan was left untouched
    for (size_t k = 0; k < history_.size() && k < 2; ++k) {
      shared_ptr<Blob<Dtype> > fresh(new Blob<Dtype>(vector<int>(1, (int)new_nnz)));       // (a new blob is zero-filled)
      if (n > 0 && new_nnz > 0) {
        if (aligned_on_device_)
          ESCOIN_CHECK(escoin_compact_entries(map.gpu_data(), n, (int)sizeof(Dtype), history_[k]->gpu_data(), fresh->mutable_gpu_data(), 1, Caffe::stream()));
        else
          ESCOIN_CHECK(escoin_compact_entries(map.cpu_data(), n, (int)sizeof(Dtype), history_[k]->cpu_data(), fresh->mutable_cpu_data(), 0, nullptr));
      }
      history_[k] = fresh;     // (the old blob's release waits for the device)
    }
    Blob<Dtype> &w = *this->blobs_[0];
    Dtype *data = w.mutable_cpu_data(), *diff = w.mutable_cpu_diff();
    const int *m = map.cpu_data();
    for (long e = 0; e < n; ++e)
      if (m[e] < 0) data[old_pos[(size_t)e]] = (Dtype)0, diff[old_pos[(size_t)e]] = (Dtype)0;
    if (n_grown > 0) {
      vector<Dtype> values;
      const vector<size_t> new_pos = positions(new_nnz, &values);
      const int *gr = grown.cpu_data();
      for (long i = 0; i < n_grown; ++i) {
        ESC_CHECK(gr[i] >= 0 && gr[i] < new_nnz);
        data[new_pos[(size_t)gr[i]]] = values[(size_t)gr[i]];
      }
    }
  }
  // The DENSE weight gradient of the layer's bottom / top pairs (include/escoin.h, "Dense weight gradient"; the
  // reference's weight_gpu_gemm result, base_conv_layer.cpp:877-889): `out` is reshaped like blobs_[0] and its DATA is
  // overwritten with the gradient at every position, inside and outside the pattern -- what escoin_rewire_desc.score
  // reads (out->gpu_data() for a plan with a device side, out->cpu_data() otherwise).  blobs_[0]'s diff is not touched.
  // Caffe::GPU, float: the matrix-core kernel on the device, asynchronous on Caffe::stream().  Caffe::GPU, double: the
  // library has no double kernel on the device, so this falls back to the CPU entry point on the blobs' cpu_data (a copy
  // of bottom, top and top's diff to the host).  Caffe::CPU: the CPU entry point.  A layer that is not aligned yet aligns
  // first.
  void DenseWeightDiff(const vector<Blob<Dtype> *> &top, const vector<Blob<Dtype> *> &bottom, Blob<Dtype> *out) {
    ESC_CHECK(plan_ != nullptr && out != nullptr);
    const bool gpu = Caffe::mode() == Caffe::GPU;
    if (!aligned_ || (gpu && !aligned_on_device_)) WeightAlign();
    out->Reshape(this->blobs_[0]->shape());
    const bool device = gpu && sizeof(Dtype) == 4;
    ESC_CHECK(!top.empty() && top.size() == bottom.size());
    for (size_t i = 0; i < top.size(); ++i) {
      if (device)
        ESCOIN_CHECK(EscApi<Dtype>::dense_wgrad(plan_, bottom[i]->gpu_data(), fuse_relu_ ? top[i]->gpu_data() : nullptr,
                                                top[i]->gpu_diff(), out->mutable_gpu_data(), num_, i > 0, Caffe::stream()));
      else
        ESCOIN_CHECK(EscApi<Dtype>::dense_wgrad_cpu(plan_, bottom[i]->cpu_data(), fuse_relu_ ? top[i]->cpu_data() : nullptr,
                                                    top[i]->cpu_diff(), out->mutable_cpu_data(), num_, i > 0,
                                                    Caffe::cpu_threads()));
    }
  }
  // SolverUpdate's histories, for snapshots and tests: {weights' h / m, weights' v, bias' h / m, bias' v}; empty before the
  // first SolverUpdate on an alignment
  const vector<shared_ptr<Blob<Dtype> > > &solver_history() const { return history_; }

  // The aligned form as one byte blob (CSR + channel deal + unit table + code object), and WeightAlign from such
  // a blob instead of from blobs_[0]: what a Net::CopyTrainedLayersFrom that finds "<model>.escoin/<layer>.bin"
  // next to the .caffemodel would call (the reference recomputes the aligned form at every load, net.cpp:819; here
  // it contains compiled code, so a deployment persists it once).  Returns true when the persisted code object was
  // loaded as it was; a blob written for other options / batch / device falls back to aligning from its CSR.
  vector<unsigned char> ExportAligned() const {
    ESC_CHECK(plan_ != nullptr && aligned_);
    size_t n = 0;
    ESCOIN_CHECK(escoin_plan_export_aligned(plan_, nullptr, 0, &n));
    vector<unsigned char> blob(n);
    ESCOIN_CHECK(escoin_plan_export_aligned(plan_, blob.data(), blob.size(), &n));
    blob.resize(n);
    return blob;
  }
  bool WeightAlignFrom(const vector<unsigned char> &blob) {
    ESC_CHECK(plan_ != nullptr);
    ESCOIN_CHECK(escoin_plan_set_option(plan_, "conv_mode", (int)Caffe::conv_mode()));
    aligned_mode_ = Caffe::conv_mode();
    ESCOIN_CHECK(escoin_plan_import_aligned(plan_, blob.data(), blob.size(), Caffe::stream()));
    aligned_ = true;
    aligned_on_device_ = true;
    history_.clear();
    return escoin_plan_stat(plan_, "import_fast") == 1;
  }

  virtual inline int MinBottomBlobs() const { return 1; }
  virtual inline int MinTopBlobs() const { return 1; }
  virtual inline bool EqualNumBottomTopBlobs() const { return true; }
  long nnz() const { return plan_ ? escoin_plan_nnz(plan_, -1) : 0; }
  // a stat of the layer's plan (include/escoin.h escoin_plan_stat), e.g. "wgrad_kernel" after a Backward in GPU mode
  long plan_stat(const char *key) const { return plan_ ? escoin_plan_stat(plan_, key) : -1; }
  const char *kernel_name() const {
    if (Caffe::mode() == Caffe::CPU) return escoin_cpu_kernel_name();
    return plan_ ? escoin_plan_kernel_name(plan_) : "";
  }

 protected:
  escoin_conv_desc desc(const Blob<Dtype> *b, const ConvolutionParameter &cp) const {
    escoin_conv_desc d;
    d.N = b->shape(0); d.C = b->shape(1); d.H = b->shape(2); d.W = b->shape(3);
    d.M = cp.num_output; d.KH = cp.kernel_h; d.KW = cp.kernel_w;
    d.pad_h = cp.pad_h; d.pad_w = cp.pad_w; d.stride_h = cp.stride_h; d.stride_w = cp.stride_w;
    d.dil_h = cp.dilation; d.dil_w = cp.dilation; d.group = cp.group;
    d.has_bias = cp.bias_term ? 1 : 0; d.fuse_relu = fuse_relu_ ? 1 : 0;
    return d;
  }
  // forward_gpu_sconv_par + forward_gpu_bias (base_conv_layer.cpp:800-856) for the whole batch
  void forward_gpu_sconv_par(const Dtype *input, const Dtype * /*weights*/, Dtype *output) {
    ESC_CHECK(aligned_);   // the reference silently computes zeros here
    if (!aligned_on_device_) {   // WeightAlign ran in CPU mode, the net was switched to GPU mode afterwards
      ESCOIN_CHECK(EscApi<Dtype>::weight_align(plan_, this->blobs_[0]->gpu_data(), 1, Caffe::stream()));
      aligned_on_device_ = true;
    }
    if (Caffe::conv_mode() != aligned_mode_) {   // `caffe test -conv_mode N` flipped after the load
      ESCOIN_CHECK(escoin_plan_set_option(plan_, "conv_mode", (int)Caffe::conv_mode()));
      aligned_mode_ = Caffe::conv_mode();
    }
    const Dtype *bias = bias_term_ ? this->blobs_[1]->gpu_data() : nullptr;
    ESCOIN_CHECK(EscApi<Dtype>::forward(plan_, input, bias, output, num_, Caffe::stream()));
  }
  // Forward_cpu's body for one bottom/top pair: the batch loop of conv_layer.cpp:44-61 (forward_cpu_sconv per image,
  // base_conv_layer.cpp:569-661, then forward_cpu_bias, :663-669) inside the library, on Caffe::cpu_threads() threads
  void forward_cpu_sconv_batch(const Dtype *input, Dtype *output) {
    ESC_CHECK(aligned_);
    const Dtype *bias = bias_term_ ? this->blobs_[1]->cpu_data() : nullptr;
    ESCOIN_CHECK(EscApi<Dtype>::forward_cpu(plan_, input, bias, output, num_, Caffe::cpu_threads()));
  }
  // Backward_gpu's body for one bottom/top pair (backward_gpu_gemm / weight_gpu_gemm / backward_gpu_bias,
  // base_conv_layer.cpp:859-897, pattern-preserving): a NULL output is not computed.  A plan aligned in CPU mode is
  // aligned on the device on the spot, as in forward_gpu_sconv_par.
  void backward_gpu_sconv(const Dtype *bottom, const Dtype *top, const Dtype *top_diff, Dtype *bottom_diff,
                          Dtype *weight_diff, Dtype *bias_diff) {
    ESC_CHECK(aligned_);
    if (!aligned_on_device_) {
      ESCOIN_CHECK(EscApi<Dtype>::weight_align(plan_, this->blobs_[0]->gpu_data(), 1, Caffe::stream()));
      aligned_on_device_ = true;
    }
    ESCOIN_CHECK(EscApi<Dtype>::backward(plan_, bottom, top, top_diff, bottom_diff, weight_diff, bias_diff, num_,
                                         Caffe::stream()));
  }
  void backward_cpu_sconv(const Dtype *bottom, const Dtype *top, const Dtype *top_diff, Dtype *bottom_diff,
                          Dtype *weight_diff, Dtype *bias_diff) {
    ESC_CHECK(aligned_);
    ESCOIN_CHECK(EscApi<Dtype>::backward_cpu(plan_, bottom, top, top_diff, bottom_diff, weight_diff, bias_diff, num_,
                                             Caffe::cpu_threads()));
  }
  escoin_plan *plan_;
  escoin_conv_desc desc_;
  bool aligned_ = false, aligned_on_device_ = false;
  vector<shared_ptr<Blob<Dtype> > > history_;   // SolverUpdate's: {weights' h / m, weights' v, bias' h / m, bias' v}
  Caffe::ConvMode aligned_mode_ = Caffe::SCONV_PAR;
  int num_, channels_, group_, num_output_;
  bool bias_term_, fuse_relu_;
  bool deconv_ = false;   // DeconvolutionLayer: the plan reads the descriptor as a Deconvolution layer's (option "deconv")
  int planned_num_;
  int bottom_dim_ = 0, top_dim_ = 0;
};

template <typename Dtype>
class ConvolutionLayer : public BaseConvolutionLayer<Dtype> {   // conv_layer.hpp:30-80
 public:
  explicit ConvolutionLayer(const LayerParameter &param) : BaseConvolutionLayer<Dtype>(param) {}
  virtual inline const char *type() const { return "Convolution"; }

 protected:
  // conv_layer.cpp:25-63.  Every Caffe::ConvMode takes the direct sparse host kernel (the reference's Forward_cpu
  // uses it for SCONV and the dense GEMM otherwise: same sums, escoin.h "Caffe::CPU mode").
  virtual void Forward_cpu(const vector<Blob<Dtype> *> &bottom, const vector<Blob<Dtype> *> &top) {
    for (size_t i = 0; i < bottom.size(); ++i) {
      const Dtype *bottom_data = bottom[i]->cpu_data();
      Dtype *top_data = top[i]->mutable_cpu_data();
      this->forward_cpu_sconv_batch(bottom_data, top_data);
    }
  }
  // conv_layer.cu:8-40.  SCONV and SCONV_PAR produce the same numbers; both go through one
  // batched launch per bottom (the per-image launches of SCONV are a reference artefact).
  virtual void Forward_gpu(const vector<Blob<Dtype> *> &bottom, const vector<Blob<Dtype> *> &top) {
    const Dtype *weight = this->blobs_[0]->gpu_data();
    for (size_t i = 0; i < bottom.size(); ++i) {
      const Dtype *bottom_data = bottom[i]->gpu_data();
      Dtype *top_data = top[i]->mutable_gpu_data();
      this->forward_gpu_sconv_par(bottom_data, weight, top_data);
    }
  }
  // conv_layer.cu:42-73 / conv_layer.cpp:65-99: per bottom/top pair the bias gradient (bias_term_ &&
  // param_propagate_down(1)), the weight gradient (param_propagate_down(0)) and the bottom gradient (propagate_down[i]),
  // each accumulated / written as there -- through the CSR's nonzeros only.  For ConvolutionReLU the forward's top
  // supplies the ReLU mask.
  virtual void Backward_gpu(const vector<Blob<Dtype> *> &top, const vector<bool> &propagate_down,
                            const vector<Blob<Dtype> *> &bottom) {
    for (size_t i = 0; i < top.size(); ++i) {
      Dtype *weight_diff = this->param_propagate_down(0) ? this->blobs_[0]->mutable_gpu_diff() : nullptr;
      Dtype *bias_diff = this->bias_term_ && this->param_propagate_down(1) ? this->blobs_[1]->mutable_gpu_diff() : nullptr;
      Dtype *bottom_diff = propagate_down.size() > i && propagate_down[i] ? bottom[i]->mutable_gpu_diff() : nullptr;
      if (!weight_diff && !bias_diff && !bottom_diff) continue;
      this->backward_gpu_sconv(weight_diff ? bottom[i]->gpu_data() : nullptr,
                               this->fuse_relu_ ? top[i]->gpu_data() : nullptr, top[i]->gpu_diff(), bottom_diff,
                               weight_diff, bias_diff);
    }
  }
  virtual void Backward_cpu(const vector<Blob<Dtype> *> &top, const vector<bool> &propagate_down,
                            const vector<Blob<Dtype> *> &bottom) {
    for (size_t i = 0; i < top.size(); ++i) {
      Dtype *weight_diff = this->param_propagate_down(0) ? this->blobs_[0]->mutable_cpu_diff() : nullptr;
      Dtype *bias_diff = this->bias_term_ && this->param_propagate_down(1) ? this->blobs_[1]->mutable_cpu_diff() : nullptr;
      Dtype *bottom_diff = propagate_down.size() > i && propagate_down[i] ? bottom[i]->mutable_cpu_diff() : nullptr;
      if (!weight_diff && !bias_diff && !bottom_diff) continue;
      this->backward_cpu_sconv(weight_diff ? bottom[i]->cpu_data() : nullptr,
                               this->fuse_relu_ ? top[i]->cpu_data() : nullptr, top[i]->cpu_diff(), bottom_diff,
                               weight_diff, bias_diff);
    }
  }
};

template <typename Dtype>
class ConvolutionReLULayer : public ConvolutionLayer<Dtype> {   // conv_relu_layer.hpp / .cu:8-30
  // Backward: ConvolutionLayer's, which hands the forward's top to the library for the ReLU mask
  // (G = top_diff x [top > 0]).  The reference's conv_relu_layer.cu:33-63 is the plain conv body and ignores the
  // ReLU -- a wrong gradient wherever the ReLU clipped; not copied.
 public:
  explicit ConvolutionReLULayer(const LayerParameter &param) : ConvolutionLayer<Dtype>(param) {
    this->fuse_relu_ = true;
  }
  virtual inline const char *type() const { return "ConvolutionReLU"; }
};

// inner_product_layer.hpp / .cpp / .cu: top = bottom (M_ x K_) * blobs_[0]^T (N_ x K_) + bias.  The layer is the 1x1
// convolution of M_ images of K_ channels and one pixel (include/escoin.h "Batch-to-space"), so it IS a ConvolutionLayer
// with another SetUp and Reshape: WeightAlign, Forward / Backward in both brews, WeightUpdate, SolverUpdate, Prune, Rewire,
// DenseWeightDiff and the persisted form are the convolution layer's code on the same C entry points.  With
// Caffe::set_b2s(true) a float layer in GPU mode runs on the pointwise kernels with the batch as the pixel axis; double
// and CPU mode run through the unchanged paths.  transpose = true (blobs_[0] as K_ x N_) aborts.
template <typename Dtype>
class InnerProductLayer : public ConvolutionLayer<Dtype> {
 public:
  explicit InnerProductLayer(const LayerParameter &param) : ConvolutionLayer<Dtype>(param), K_(0) {}
  virtual inline const char *type() const { return "InnerProduct"; }

  // inner_product_layer.cpp LayerSetUp: K_ is the count from `axis`; blobs_[0] is num_output x K_, blobs_[1] num_output
  virtual void LayerSetUp(const vector<Blob<Dtype> *> &bottom, const vector<Blob<Dtype> *> &) {
    const InnerProductParameter &ip = this->layer_param_.inner_product_param;
    if (ip.transpose) {
      fprintf(stderr, "InnerProductLayer %s: inner_product_param.transpose = true is not supported\n", this->layer_param_.name.c_str());
      abort();
    }
    ESC_CHECK(ip.num_output > 0);
    axis_ = canonical_axis(bottom[0], ip.axis);
    K_ = bottom[0]->count(axis_, bottom[0]->num_axes());
    ESC_CHECK(K_ > 0);
    this->channels_ = K_;
    this->num_output_ = ip.num_output;
    this->group_ = 1;
    this->bias_term_ = ip.bias_term;
    this->blobs_.resize(this->bias_term_ ? 2 : 1);
    vector<int> wshape(2);
    wshape[0] = this->num_output_; wshape[1] = K_;
    this->blobs_[0].reset(new Blob<Dtype>(wshape));
    if (this->bias_term_) this->blobs_[1].reset(new Blob<Dtype>(vector<int>(1, this->num_output_)));
    this->param_propagate_down_.resize(this->blobs_.size(), true);
  }

  // inner_product_layer.cpp Reshape: M_ = the count before `axis`; the top is the bottom's axes before `axis`, then num_output
  virtual void Reshape(const vector<Blob<Dtype> *> &bottom, const vector<Blob<Dtype> *> &top) {
    ESC_CHECK(bottom[0]->count(axis_, bottom[0]->num_axes()) == K_);     // "Input size incompatible with inner product parameters."
    this->num_ = bottom[0]->count(0, axis_);
    vector<int> tshape(bottom[0]->shape().begin(), bottom[0]->shape().begin() + axis_);
    tshape.push_back(this->num_output_);
    for (size_t i = 0; i < top.size(); ++i) top[i]->Reshape(tshape);
    this->bottom_dim_ = K_;
    this->top_dim_ = this->num_output_;
    escoin_conv_desc d;
    d.N = this->num_; d.C = K_; d.H = 1; d.W = 1; d.M = this->num_output_; d.KH = 1; d.KW = 1;
    d.pad_h = 0; d.pad_w = 0; d.stride_h = 1; d.stride_w = 1; d.dil_h = 1; d.dil_w = 1; d.group = 1;
    d.has_bias = this->bias_term_ ? 1 : 0; d.fuse_relu = 0;
    this->plan_for(d);
  }

 private:
  static int canonical_axis(const Blob<Dtype> *b, int axis) {     // blob.hpp CanonicalAxisIndex
    ESC_CHECK(axis >= -b->num_axes() && axis < b->num_axes());
    return axis < 0 ? axis + b->num_axes() : axis;
  }
  int K_, axis_ = 1;
};

// deconv_layer.hpp / .cpp / .cu: the transposed convolution (forward = the base layer's backward_*_gemm, backward =
// forward_*_gemm + weight_*_gemm).  blobs_[0] is channels x num_output / group x kernel_h x kernel_w (conv_out_channels_ is
// the bottom's channel count); the top is stride * (in - 1) + kernel - 2 * pad (compute_output_shape at dilation 1).  The
// layer runs through plan option "deconv" (include/escoin.h "Deconvolution") in both brews: WeightAlign, Forward, Backward,
// WeightUpdate and SolverUpdate are the convolution layer's code on the same C entry points; Prune, Rewire and
// DenseWeightDiff are refused by the library.  Dtype = double aborts in LayerSetUp with the library's message.
template <typename Dtype>
class DeconvolutionLayer : public ConvolutionLayer<Dtype> {
 public:
  explicit DeconvolutionLayer(const LayerParameter &param) : ConvolutionLayer<Dtype>(param) { this->deconv_ = true; }
  virtual inline const char *type() const { return "Deconvolution"; }

  virtual void LayerSetUp(const vector<Blob<Dtype> *> &bottom, const vector<Blob<Dtype> *> &top) {
    if (sizeof(Dtype) != 4) {
      fprintf(stderr, "DeconvolutionLayer %s: option \"deconv\": a double plan has no deconvolution (the inner kernels are fp32)\n",
              this->layer_param_.name.c_str());
      abort();
    }
    BaseConvolutionLayer<Dtype>::LayerSetUp(bottom, top);
    const ConvolutionParameter &cp = this->layer_param_.convolution_param;
    vector<int> wshape(4);      // deconv_layer: conv_out_channels_ = channels_, conv_in_channels_ = num_output_
    wshape[0] = this->channels_; wshape[1] = this->num_output_ / this->group_; wshape[2] = cp.kernel_h; wshape[3] = cp.kernel_w;
    this->blobs_[0].reset(new Blob<Dtype>(wshape));
  }

  virtual void Reshape(const vector<Blob<Dtype> *> &bottom, const vector<Blob<Dtype> *> &top) {
    const ConvolutionParameter &cp = this->layer_param_.convolution_param;
    this->num_ = bottom[0]->shape(0);
    ESC_CHECK(bottom[0]->shape(1) == this->channels_);
    for (size_t i = 1; i < bottom.size(); ++i) ESC_CHECK(bottom[0]->shape() == bottom[i]->shape());
    const escoin_conv_desc d = this->desc(bottom[0], cp);
    int oh = 0, ow = 0;
    compute_output_shape(d, &oh, &ow);
    for (size_t i = 0; i < top.size(); ++i) top[i]->Reshape(this->num_, this->num_output_, oh, ow);
    this->bottom_dim_ = bottom[0]->count(1, 4);
    this->top_dim_ = top[0]->count(1, 4);
    this->plan_for(d);
  }

  // deconv_layer.cpp:7-23
  static void compute_output_shape(const escoin_conv_desc &d, int *oh, int *ow) { ESCOIN_CHECK(escoin_deconv_out_shape(&d, oh, ow)); }
};

// layer_factory.hpp:53-110 / layer_factory.cpp:74: the creator registry `Net::Init` looks layer
// types up in (LayerRegistry<Dtype>::CreateLayer(param)), with the four creators this path owns.
template <typename Dtype>
class LayerRegistry {
 public:
  typedef shared_ptr<Layer<Dtype> > (*Creator)(const LayerParameter &);
  static shared_ptr<Layer<Dtype> > CreateLayer(const LayerParameter &param) {
    if (param.type == "Convolution") return shared_ptr<Layer<Dtype> >(new ConvolutionLayer<Dtype>(param));
    if (param.type == "ConvolutionReLU") return shared_ptr<Layer<Dtype> >(new ConvolutionReLULayer<Dtype>(param));
    if (param.type == "InnerProduct") return shared_ptr<Layer<Dtype> >(new InnerProductLayer<Dtype>(param));
    if (param.type == "Deconvolution") return shared_ptr<Layer<Dtype> >(new DeconvolutionLayer<Dtype>(param));
    fprintf(stderr, "Unknown layer type: %s (known types: Convolution, ConvolutionReLU, InnerProduct, Deconvolution)\n", param.type.c_str());
    abort();   // LOG(FATAL), layer_factory.hpp:79-80
  }
  static vector<string> LayerTypeList() {
    vector<string> v;
    v.push_back("Convolution");
    v.push_back("ConvolutionReLU");
    v.push_back("InnerProduct");
    v.push_back("Deconvolution");
    return v;
  }
};

}  // namespace caffe
#endif  // ESCOIN_CAFFE_SHIM_HPP_
