// dense_wgrad_cpu.cpp -- the dense weight gradient on the host (escoin_dense_wgrad_cpu[_f64]; the device twin and the
// contract are in dense_wgrad.hip / include/escoin.h): every position of blobs_[0], inside and outside the pattern.
// Plain loops, threaded over (output channel, input channel of its group); every element is one fma chain over its
// (n, oh, ow) pixels ascending from zero, then stored (or added once onto the blob): the bits do not depend on
// n_threads.  Reads the plan's geometry and fuse_relu only; works on any plan with a host CSR, in both Dtypes.
#include <cmath>
#include <thread>

#include "escoin_plan.h"
#include "parallel_for.h"

namespace escoin {
namespace cpu {

template <typename T>
static int dense_wgrad_cpu(escoin_plan *p, const T *bottom, const T *top, const T *top_diff, T *dense_diff, int n_images,
                           int accumulate, int n_threads) {
  if (!p) return fail(ESCOIN_EINVAL, "null plan");
  if (const int rc = refuse_deconv(p, "escoin_dense_wgrad_cpu")) return rc;
  if (!p->host_aligned) return fail(ESCOIN_ESTATE, "dense_wgrad_cpu called before weight_align / set_csr");
  if (p->is_f64 != (sizeof(T) == 8))
    return fail(ESCOIN_ESTATE, p->is_f64 ? "dense_wgrad_cpu: the plan holds double weights (use the _f64 entry point)"
                                         : "dense_wgrad_cpu_f64: the plan holds float weights");
  const Geometry &g = p->g;
  const escoin_conv_desc &d = g.d;
  if (!top_diff) return fail(ESCOIN_EINVAL, "dense_wgrad_cpu: top_diff is required");
  if (!bottom) return fail(ESCOIN_EINVAL, "dense_wgrad_cpu: bottom is required");
  if (!dense_diff) return fail(ESCOIN_EINVAL, "dense_wgrad_cpu: dense_diff is required");
  if (d.fuse_relu && !top) return fail(ESCOIN_EINVAL, "dense_wgrad_cpu: a fuse_relu plan needs the forward's top");
  if (n_images < 0) return fail(ESCOIN_EINVAL, "n_images must be >= 0");
  if (n_images == 0 && accumulate) return ESCOIN_OK;
  if (n_threads <= 0) {
    const unsigned hc = std::thread::hardware_concurrency();
    n_threads = hc ? (int)hc : 1;
  }
  const bool relu = d.fuse_relu != 0;
  const size_t plane = (size_t)d.H * d.W, opix = (size_t)g.OH * g.OW;
  const int kk = d.KH * d.KW;
  parallel_for((size_t)d.M * g.Cg, (size_t)n_threads, [&](size_t item) {
    const int oc = (int)(item / g.Cg), ic = (int)(item % g.Cg), grp = oc / g.Mg;
    T *out = dense_diff + (size_t)oc * g.kdim + (size_t)ic * kk;
    for (int kr = 0; kr < d.KH; ++kr)
      for (int kc = 0; kc < d.KW; ++kc) {
        T s = 0;
        for (int n = 0; n < n_images; ++n) {
          const size_t gbase = ((size_t)n * d.M + oc) * opix;
          const T *img = bottom + ((size_t)n * d.C + (size_t)grp * g.Cg + ic) * plane;
          for (int oh = 0; oh < g.OH; ++oh) {
            const int h = oh * d.stride_h - d.pad_h + kr * d.dil_h;
            if (h < 0 || h >= d.H) continue;
            for (int ow = 0; ow < g.OW; ++ow) {
              const int w = ow * d.stride_w - d.pad_w + kc * d.dil_w;
              if (w < 0 || w >= d.W) continue;
              const size_t gi = gbase + (size_t)oh * g.OW + ow;
              const T gv = relu && !(top[gi] > T(0)) ? T(0) : top_diff[gi];
              s = std::fma(gv, img[(size_t)h * d.W + w], s);
            }
          }
        }
        T &o = out[kr * d.KW + kc];
        o = accumulate ? o + s : s;
      }
  });
  return ESCOIN_OK;
}

}  // namespace cpu
}  // namespace escoin

using namespace escoin;

extern "C" {

int escoin_dense_wgrad_cpu(escoin_plan *plan, const float *bottom, const float *top, const float *top_diff, float *dense_diff,
                           int n_images, int accumulate, int n_threads) {
  return guarded([&]() -> int {
    return cpu::dense_wgrad_cpu<float>(plan, bottom, top, top_diff, dense_diff, n_images, accumulate, n_threads);
  });
}

int escoin_dense_wgrad_cpu_f64(escoin_plan *plan, const double *bottom, const double *top, const double *top_diff,
                               double *dense_diff, int n_images, int accumulate, int n_threads) {
  return guarded([&]() -> int {
    return cpu::dense_wgrad_cpu<double>(plan, bottom, top, top_diff, dense_diff, n_images, accumulate, n_threads);
  });
}

}  // extern "C"
