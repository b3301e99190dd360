// solver_step_cpu.cpp -- the host twins of solver_step.hip (include/escoin.h, "Solver step"): plain loops over the host
// CSR's values with the arithmetic of solver_rule.h.  This unit is compiled with -ffp-contract=off (and the rule carries
// the pragma): its results are bit-equal to the device kernel's.  No HIP call.
#include <string>

#include "escoin_plan.h"
#include "solver_rule.h"

namespace escoin {
namespace {

template <typename T, int Rule, int Reg>
inline void step_one(const SolverParams<T> &s, T rate, T *w, T *g, T *h, T *h2) {
  T hh = *h, hh2 = Rule == ESCOIN_SOLVER_ADAM ? *h2 : (T)0;
  *w = solver_rule<T, Rule, Reg>(s, rate, *w, *g, &hh, &hh2);
  *h = hh;
  if (Rule == ESCOIN_SOLVER_ADAM) *h2 = hh2;
  if (s.clear_diff) *g = (T)0;
}

template <typename T>
struct PlanLoop {
  escoin_plan *p;
  const SolverParams<T> &s;
  T *diff, *h, *h2, *dense_w;
  template <int Rule, int Reg> void operator()() const {
    const Geometry &g = p->g;
    const T rate = s.rate_ptr ? *s.rate_ptr : s.rate;
    std::vector<std::vector<T>> &vals = plan_vals<T>(p);
    for_each_entry(csr_view(p), [&](const CsrEntry &c) {
      const size_t at = ((size_t)c.grp * g.Mg + c.m) * g.kdim + (size_t)c.col;
      step_one<T, Rule, Reg>(s, rate, &vals[c.grp][c.j], diff + (s.diff_is_dense ? at : (size_t)c.e), h + c.e, h2 ? h2 + c.e : nullptr);
      if (dense_w) dense_w[at] = vals[c.grp][c.j];
    });
  }
};

template <typename T>
struct ArrayLoop {
  const SolverParams<T> &s;
  long n;
  T *data, *diff, *h, *h2;
  template <int Rule, int Reg> void operator()() const {
    const T rate = s.rate_ptr ? *s.rate_ptr : s.rate;
    for (long e = 0; e < n; ++e) step_one<T, Rule, Reg>(s, rate, data + e, diff + e, h + e, h2 ? h2 + e : nullptr);
  }
};

template <typename T>
int solver_step_cpu(escoin_plan *p, const escoin_solver_desc *d, T *diff, T *h, T *h2, T *dense_w) {
  const std::string name = "solver_step_cpu";
  if (!p) return fail(ESCOIN_EINVAL, name + ": null argument");
  const bool empty = plan_nnz(p) == 0;      // (0 entries: nothing is read or written, the arrays may be NULL)
  if (!empty && (!diff || !h)) return fail(ESCOIN_EINVAL, name + ": null argument");
  if (const char *why = solver_desc_error(d, empty ? static_cast<const void *>(p) : h2)) return fail(ESCOIN_EINVAL, name + ": " + why);
  if (!p->host_aligned) return fail(ESCOIN_ESTATE, name + " called before weight_align_cpu");
  if (p->aligned)
    return fail(ESCOIN_ESTATE, name + ": the plan has a device side, which this entry point would leave behind; escoin_solver_step updates both sides");
  if (p->is_f64 != (sizeof(T) == 8))
    return fail(ESCOIN_ESTATE, name + (p->is_f64 ? ": the plan holds double weights (use the _f64 entry point)" : "_f64: the plan holds float weights"));
  const SolverParams<T> s = solver_params<T>(*d);
  solver_dispatch(s.type, s.reg, PlanLoop<T>{p, s, diff, h, h2, dense_w});
  ++p->upd_count;
  return ESCOIN_OK;
}

template <typename T>
int array_step_cpu(const escoin_solver_desc *d, long n, T *data, T *diff, T *h, T *h2) {
  const std::string name = "solver_array_step_cpu";
  if (!data || !diff || !h || n < 0) return fail(ESCOIN_EINVAL, name + ": null argument or n < 0");
  if (const char *why = solver_desc_error(d, h2)) return fail(ESCOIN_EINVAL, name + ": " + why);
  SolverParams<T> s = solver_params<T>(*d);
  s.diff_is_dense = 0;
  solver_dispatch(s.type, s.reg, ArrayLoop<T>{s, n, data, diff, h, h2});
  return ESCOIN_OK;
}

}  // namespace
}  // namespace escoin

using namespace escoin;

extern "C" {

int escoin_solver_step_cpu(escoin_plan *p, const escoin_solver_desc *d, float *diff, float *h, float *h2, float *dense_w) {
  return guarded([&]() -> int { return solver_step_cpu<float>(p, d, diff, h, h2, dense_w); });
}
int escoin_solver_step_cpu_f64(escoin_plan *p, const escoin_solver_desc *d, double *diff, double *h, double *h2, double *dense_w) {
  return guarded([&]() -> int { return solver_step_cpu<double>(p, d, diff, h, h2, dense_w); });
}
int escoin_solver_array_step_cpu(const escoin_solver_desc *d, long n, float *data, float *diff, float *h, float *h2) {
  return guarded([&]() -> int { return array_step_cpu<float>(d, n, data, diff, h, h2); });
}
int escoin_solver_array_step_cpu_f64(const escoin_solver_desc *d, long n, double *data, double *diff, double *h, double *h2) {
  return guarded([&]() -> int { return array_step_cpu<double>(d, n, data, diff, h, h2); });
}

}  // extern "C"
