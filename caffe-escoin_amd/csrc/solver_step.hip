// solver_step.hip -- the solver's element-wise rule fused into the in-place weight update (include/escoin.h, "Solver
// step").  update_values.hip scatters values somebody else computed, one lane per DESTINATION word; here the value is
// computed in the launch, so the launch is entry-major: one lane per CSR entry reads w (the plan's value array), its
// gradient and its history, applies the rule once (solver_rule.h) and stores w' to every device word that holds that
// weight, through the entry-major view of the update state's list (UpdState::e_ptr; update_values.hip builds and owns it).
// A destination-major launch could not do this in one kernel: the lanes of an entry's other destinations would read
// gen.vals[e] while its own lane overwrites it.
#include <hip/hip_runtime.h>

#include <string>

#include "escoin_plan.h"
#include "solver_rule.h"

namespace escoin {

template <typename T>
struct SolverArgs {
  void *base[kUpdMaxBuffers];
  const int *e_ptr;          // nullptr: vals[e] is the only destination (the array step)
  const unsigned *e_off;
  const unsigned char *e_buf;
  const int *wpos;
  T *vals, *diff, *h, *h2, *dense_w;
  long n;
  SolverParams<T> s;
};

// One lane per entry.  Every word the lane reads (vals[e], diff, h, h2 at e or wpos[e]) is written by this lane alone;
// the stores to the destinations are plain vector stores and become visible to the next launch -- as weights, as
// weight lines read through the scalar cache, as literals in code -- exactly as the comment at
// escoin_update_values_kernel explains.  The arithmetic is IEEE operation by operation: no contraction (solver_rule.h),
// correctly rounded division and square root.
template <typename T, int Rule, int Reg>
__global__ void __launch_bounds__(256) escoin_solver_step_kernel(SolverArgs<T> a) {
#pragma clang fp contract(off)
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.n) return;
  const long at = a.wpos ? (long)a.wpos[e] : e;     // the entry's element of a blobs_[0]-shaped array
  const long gi = a.s.diff_is_dense ? at : e;
  const T rate = a.s.rate_ptr ? *a.s.rate_ptr : a.s.rate;
  T h = a.h[e], h2 = Rule == ESCOIN_SOLVER_ADAM ? a.h2[e] : (T)0;
  const T w = solver_rule<T, Rule, Reg>(a.s, rate, a.vals[e], a.diff[gi], &h, &h2);
  a.h[e] = h;
  if (Rule == ESCOIN_SOLVER_ADAM) a.h2[e] = h2;
  if (a.s.clear_diff) a.diff[gi] = (T)0;
  if (a.dense_w) a.dense_w[at] = w;
  if (!a.e_ptr) {
    a.vals[e] = w;
    return;
  }
  for (int k = a.e_ptr[e], end = a.e_ptr[e + 1]; k < end; ++k) static_cast<T *>(a.base[a.e_buf[k]])[a.e_off[k]] = w;
}

namespace {

template <typename T>
struct Launch {
  const SolverArgs<T> &a;
  hipStream_t stream;
  template <int Rule, int Reg> void operator()() const {
    hipLaunchKernelGGL((escoin_solver_step_kernel<T, Rule, Reg>), dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, stream, a);
  }
};

int require_device(const char *name) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) == hipSuccess && ndev >= 1) return ESCOIN_OK;
  return fail(ESCOIN_ENODEVICE, std::string(name) + ": no HIP device (the _cpu entry point is the host's)");
}

template <typename T>
int solver_step_t(escoin_plan *p, const escoin_solver_desc *d, T *diff, T *h, T *h2, T *dense_w, void *stream_v) {
  const char *name = "solver_step";     // (both Dtypes, as update_values.hip names its entry points in messages)
  if (!p) return fail(ESCOIN_EINVAL, std::string(name) + ": null argument");
  // a plan of 0 entries reads and writes nothing: its arrays (of 0 elements) may be NULL, as an empty tensor's pointer is
  const bool empty = plan_nnz(p) == 0;
  if (!empty && (!diff || !h)) return fail(ESCOIN_EINVAL, std::string(name) + ": null argument");
  if (const char *why = solver_desc_error(d, empty ? static_cast<const void *>(p) : h2)) return fail(ESCOIN_EINVAL, std::string(name) + ": " + why);
  hipStream_t stream = (hipStream_t)stream_v;
  SolverTargets t;
  if (const int rc = solver_begin<T>(p, name, stream, &t)) return rc;
  if (t.nnz == 0) return ESCOIN_OK;
  SolverArgs<T> a;
  for (int b = 0; b < kUpdMaxBuffers; ++b) a.base[b] = t.base[b];
  a.e_ptr = t.e_ptr, a.e_off = t.e_off, a.e_buf = t.e_buf;
  a.s = solver_params<T>(*d);
  a.wpos = (a.s.diff_is_dense || dense_w) ? t.wpos : nullptr;
  a.vals = static_cast<T *>(t.vals), a.diff = diff, a.h = h, a.h2 = h2, a.dense_w = dense_w;
  a.n = t.nnz;
  solver_dispatch(a.s.type, a.s.reg, Launch<T>{a, stream});
  ESCOIN_HIP_TRY(hipGetLastError());
  return solver_end<T>(p, t, stream);
}

template <typename T>
int array_step_t(const escoin_solver_desc *d, long n, T *data, T *diff, T *h, T *h2, void *stream_v) {
  const char *name = "solver_array_step";
  if (!data || !diff || !h || n < 0) return fail(ESCOIN_EINVAL, std::string(name) + ": null argument or n < 0");
  if (const char *why = solver_desc_error(d, h2)) return fail(ESCOIN_EINVAL, std::string(name) + ": " + why);
  if (const int rc = require_device(name)) return rc;
  if (n == 0) return ESCOIN_OK;
  if ((n + 255) / 256 > 0x7fffffffL) return fail(ESCOIN_EINVAL, std::string(name) + ": n is beyond one launch");
  SolverArgs<T> a = {};
  a.s = solver_params<T>(*d);
  a.s.diff_is_dense = 0;
  a.vals = data, a.diff = diff, a.h = h, a.h2 = h2;
  a.n = n;
  solver_dispatch(a.s.type, a.s.reg, Launch<T>{a, (hipStream_t)stream_v});
  ESCOIN_HIP_TRY(hipGetLastError());
  return ESCOIN_OK;
}

}  // namespace
}  // namespace escoin

using namespace escoin;

extern "C" {

int escoin_solver_step(escoin_plan *p, const escoin_solver_desc *d, float *diff, float *h, float *h2, float *dense_w, void *stream) {
  return guarded([&]() -> int { return solver_step_t<float>(p, d, diff, h, h2, dense_w, stream); });
}
int escoin_solver_step_f64(escoin_plan *p, const escoin_solver_desc *d, double *diff, double *h, double *h2, double *dense_w, void *stream) {
  return guarded([&]() -> int { return solver_step_t<double>(p, d, diff, h, h2, dense_w, stream); });
}
int escoin_solver_array_step(const escoin_solver_desc *d, long n, float *data, float *diff, float *h, float *h2, void *stream) {
  return guarded([&]() -> int { return array_step_t<float>(d, n, data, diff, h, h2, stream); });
}
int escoin_solver_array_step_f64(const escoin_solver_desc *d, long n, double *data, double *diff, double *h, double *h2, void *stream) {
  return guarded([&]() -> int { return array_step_t<double>(d, n, data, diff, h, h2, stream); });
}

}  // extern "C"
