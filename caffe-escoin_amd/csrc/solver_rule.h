// solver_rule.h -- the solver's element-wise rule (include/escoin.h "Solver step"), written once for the device kernel
// (solver_step.hip) and its host twin (solver_step_cpu.cpp) so that the two cannot drift apart.
#ifndef ESCOIN_SOLVER_RULE_H_
#define ESCOIN_SOLVER_RULE_H_

#include <cmath>

#include "escoin.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define ESCOIN_HD __host__ __device__
#else
#define ESCOIN_HD
#endif

namespace escoin {

// The hyper-parameters of one call in the plan's Dtype (converted once), and what the call does around the rule.
template <typename T>
struct SolverParams {
  T rate, momentum, momentum2, delta, decay, diff_scale;
  T one_plus_momentum, one_minus_beta1, one_minus_beta2;   // formed in T
  const T *rate_ptr;   // escoin_solver_desc::rate_dev, or nullptr
  int type, reg;       // reg is ESCOIN_REG_NONE when decay == 0
  int scale;           // diff_scale != 1
  int diff_is_dense, clear_diff;
};

// nullptr when the descriptor is usable, otherwise what is wrong with it
inline const char *solver_desc_error(const escoin_solver_desc *d, const void *history2) {
  if (!d) return "null desc";
  if (d->type != ESCOIN_SOLVER_SGD && d->type != ESCOIN_SOLVER_NESTEROV && d->type != ESCOIN_SOLVER_ADAM) return "unknown solver type";
  if (d->regularization != ESCOIN_REG_NONE && d->regularization != ESCOIN_REG_L2 && d->regularization != ESCOIN_REG_L1)
    return "unknown regularization";
  if (d->type == ESCOIN_SOLVER_ADAM && !history2) return "Adam needs history2";
  return nullptr;
}

template <typename T>
inline SolverParams<T> solver_params(const escoin_solver_desc &d) {
#pragma clang fp contract(off)
  SolverParams<T> s;
  s.rate = (T)d.rate, s.momentum = (T)d.momentum, s.momentum2 = (T)d.momentum2, s.delta = (T)d.delta, s.decay = (T)d.decay;
  s.diff_scale = (T)d.diff_scale;
  s.one_plus_momentum = (T)1 + s.momentum;
  s.one_minus_beta1 = (T)1 - s.momentum;
  s.one_minus_beta2 = (T)1 - s.momentum2;
  s.rate_ptr = static_cast<const T *>(d.rate_dev);
  s.type = d.type;
  s.reg = d.decay == 0.0 ? ESCOIN_REG_NONE : d.regularization;
  s.scale = d.diff_scale != 1.0;
  s.diff_is_dense = d.diff_is_dense != 0, s.clear_diff = d.clear_diff != 0;
  return s;
}

// One element: the weight w, its gradient g, its history h (Adam: m) and h2 (Adam: v; untouched otherwise).  Returns w';
// h and h2 receive their new values.  Every operation is one IEEE operation of T: no contraction, in the order written.
template <typename T, int Rule, int Reg>
ESCOIN_HD inline T solver_rule(const SolverParams<T> &s, T rate, T w, T g, T *h, T *h2) {
#pragma clang fp contract(off)
  if (s.scale) g = s.diff_scale * g;
  if (Reg == ESCOIN_REG_L2) {
    const T r = s.decay * w;
    g = g + r;
  } else if (Reg == ESCOIN_REG_L1) {
    const T sign = (T)((w > (T)0) - (w < (T)0));   // caffe_cpu_sign: 0 for +-0 and NaN
    const T r = s.decay * sign;
    g = g + r;
  }
  T u;
  if (Rule == ESCOIN_SOLVER_ADAM) {
    const T a = *h * s.momentum, b = g * s.one_minus_beta1;
    const T m = a + b;
    const T gg = g * g;
    const T c = *h2 * s.momentum2, d = gg * s.one_minus_beta2;
    const T v = c + d;
    const T num = rate * m;
    const T den = std::sqrt(v) + s.delta;
    u = num / den;
    *h = m, *h2 = v;
  } else {
    const T a = s.momentum * *h, b = rate * g;
    const T hn = a + b;
    if (Rule == ESCOIN_SOLVER_NESTEROV) {
      const T c = s.one_plus_momentum * hn;
      u = c - a;
    } else {
      u = hn;
    }
    *h = hn;
  }
  return w - u;
}

// dispatch over (type, reg) to f.template operator()<Rule, Reg>()
template <typename F>
inline void solver_dispatch(int type, int reg, F &&f) {
#define ESCOIN_SOLVER_REG(R)                                                      \
  switch (reg) {                                                                  \
    case ESCOIN_REG_L2: f.template operator()<R, ESCOIN_REG_L2>(); break;         \
    case ESCOIN_REG_L1: f.template operator()<R, ESCOIN_REG_L1>(); break;         \
    default: f.template operator()<R, ESCOIN_REG_NONE>(); break;                  \
  }
  switch (type) {
    case ESCOIN_SOLVER_ADAM: ESCOIN_SOLVER_REG(ESCOIN_SOLVER_ADAM) break;
    case ESCOIN_SOLVER_NESTEROV: ESCOIN_SOLVER_REG(ESCOIN_SOLVER_NESTEROV) break;
    default: ESCOIN_SOLVER_REG(ESCOIN_SOLVER_SGD) break;
  }
#undef ESCOIN_SOLVER_REG
}

}  // namespace escoin
#endif
