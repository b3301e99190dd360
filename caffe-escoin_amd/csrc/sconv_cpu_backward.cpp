// sconv_cpu_backward.cpp -- ConvolutionLayer::Backward_cpu (conv_layer.cpp:65-99) that keeps the sparsity pattern, on the
// host (escoin_backward_cpu[_f64]; the device twin and the contract are in sconv_backward.hip / include/escoin.h).
// Plain loops, no SIMD work: the CPU mode is the baseline the device is checked against.
//   data gradient    threaded over (image, input channel).  A channel's outputs start at 0 and take one fma per
//                    contributing entry of the channel's transposed-CSR row, in ascending (ocl, kr, kc) order: the rows
//                    are csr_tables.h's gather_transpose, the table the device gather kernel walks, so the two share
//                    their order by construction and are bit-identical;
//   weight / bias    threaded over CSR rows; every entry (and bias) is one sum over (n, oh, ow) in that order, then
//                    added into the gradient.
// Every output is summed in a fixed order: the bits do not depend on n_threads.  Works on any plan with a host CSR
// (escoin_weight_align_cpu, and every device align, which keeps the host CSR).
#include <algorithm>
#include <cmath>
#include <thread>
#include <vector>

#include "escoin_plan.h"
#include "parallel_for.h"

namespace escoin {
namespace cpu {

template <typename T>
static int backward_cpu(escoin_plan *p, const T *bottom, const T *top, const T *top_diff, T *bottom_diff, T *weight_diff,
                        T *bias_diff, int n_images, int n_threads, bool compact) {
  if (!p) return fail(ESCOIN_EINVAL, "null plan");
  if (!p->host_aligned) return fail(ESCOIN_ESTATE, "backward_cpu called before weight_align / set_csr");
  if (p->is_f64 != (sizeof(T) == 8))
    return fail(ESCOIN_ESTATE, p->is_f64 ? "backward_cpu: the plan holds double weights (use the _f64 entry point)"
                                         : "backward_cpu_f64: the plan holds float weights");
  const Geometry &g = p->g;
  const escoin_conv_desc &d = g.d;
  if (!top_diff) return fail(ESCOIN_EINVAL, "backward_cpu: top_diff is required");
  if (d.fuse_relu && !top) return fail(ESCOIN_EINVAL, "backward_cpu: a fuse_relu plan needs the forward's top");
  if (weight_diff && !bottom) return fail(ESCOIN_EINVAL, "backward_cpu: the weight gradient needs bottom");
  if (n_images < 0) return fail(ESCOIN_EINVAL, "n_images must be >= 0");
  if (n_images == 0) return ESCOIN_OK;
  if constexpr (sizeof(T) == 4)
    if (p->deconv) {     // (option "deconv": d2s_cpu.cpp)
      if (!g_d2s_cpu_hooks.backward) return fail(ESCOIN_EINVAL, "option \"deconv\": this build does not carry its CPU mode");
      return g_d2s_cpu_hooks.backward(p, bottom, top, top_diff, bottom_diff, weight_diff, bias_diff, n_images, n_threads, compact);
    }
  if (const int rcs = sync_host_values(p)) return rcs;     // (device-source weight updates: the values come back first)
  if (n_threads <= 0) {
    const unsigned hc = std::thread::hardware_concurrency();
    n_threads = hc ? (int)hc : 1;
  }
  const bool relu = d.fuse_relu != 0;
  const size_t plane = (size_t)d.H * d.W, opix = (size_t)g.OH * g.OW;
  const CsrView csr = csr_view(p);
  const auto &values = plan_vals<T>(p);
  // G at (n, oc, pixel)
  auto grad_at = [&](size_t gi) -> T { return relu && !(top[gi] > T(0)) ? T(0) : top_diff[gi]; };

  if (bottom_diff) {
    // transposed CSR: input channel c's entries are tsrc[trow[c] .. trow[c + 1]), in ascending (ocl, kr, kc)
    struct Ent { int ocl, kr, kc; T v; };
    std::vector<Ent> ents((size_t)csr.nnz());
    for_each_entry(csr, [&](const CsrEntry &c) {
      const Tap tap = decode_tap(c.col, d.KH, d.KW);
      ents[(size_t)c.e] = Ent{c.m, tap.kr, tap.kc, values[c.grp][c.j]};
    });
    const GatherTables gt = gather_transpose(csr);
    parallel_for((size_t)n_images * d.C, (size_t)n_threads, [&](size_t item) {
      const int n = (int)(item / d.C), c = (int)(item % d.C), grp = c / g.Cg;
      T *out = bottom_diff + ((size_t)n * d.C + c) * plane;
      std::fill(out, out + plane, T(0));
      const size_t gbase = ((size_t)n * d.M + (size_t)grp * g.Mg) * opix;
      // entry outer, pixel inner: every bottom pixel still takes its fmas in entry order (a tap maps distinct output
      // pixels to distinct bottom pixels)
      for (int k = gt.trow[c]; k < gt.trow[c + 1]; ++k) {
        const Ent &e = ents[(size_t)gt.tsrc[k]];
        for (int oh = 0; oh < g.OH; ++oh) {
          const int h = oh * d.stride_h - d.pad_h + e.kr * d.dil_h;
          if (h < 0 || h >= d.H) continue;
          for (int ow = 0; ow < g.OW; ++ow) {
            const int w = ow * d.stride_w - d.pad_w + e.kc * d.dil_w;
            if (w < 0 || w >= d.W) continue;
            const T gv = grad_at(gbase + (size_t)e.ocl * opix + (size_t)oh * g.OW + ow);
            out[(size_t)h * d.W + w] = std::fma(e.v, gv, out[(size_t)h * d.W + w]);
          }
        }
      }
    });
  }

  if (weight_diff || bias_diff) {
    parallel_for((size_t)d.M, (size_t)n_threads, [&](size_t oc_) {
      const int oc = (int)oc_, grp = oc / g.Mg, m = oc - grp * g.Mg;
      if (bias_diff) {
        T s = 0;
        for (int n = 0; n < n_images; ++n) {
          const size_t gbase = ((size_t)n * d.M + oc) * opix;
          for (size_t q = 0; q < opix; ++q) s += grad_at(gbase + q);
        }
        bias_diff[oc] = bias_diff[oc] + s;
      }
      if (!weight_diff) return;
      // compact (escoin_backward_values_cpu): weight_diff is the nnz-element array in get_csr order, groups concatenated
      const size_t base = compact ? (size_t)csr.group_base(grp) : (size_t)oc * g.kdim;
      for (int j = p->rowptr[grp][m]; j < p->rowptr[grp][m + 1]; ++j) {
        const int col = p->colidx[grp][j];
        const Tap tap = decode_tap(col, d.KH, d.KW);
        T s = 0;
        for (int n = 0; n < n_images; ++n) {
          const size_t gbase = ((size_t)n * d.M + oc) * opix;
          const T *img = bottom + ((size_t)n * d.C + (size_t)grp * g.Cg + tap.ic) * plane;
          for (int oh = 0; oh < g.OH; ++oh) {
            const int h = oh * d.stride_h - d.pad_h + tap.kr * d.dil_h;
            if (h < 0 || h >= d.H) continue;
            for (int ow = 0; ow < g.OW; ++ow) {
              const int w = ow * d.stride_w - d.pad_w + tap.kc * d.dil_w;
              if (w < 0 || w >= d.W) continue;
              s = std::fma(grad_at(gbase + (size_t)oh * g.OW + ow), img[(size_t)h * d.W + w], s);
            }
          }
        }
        const size_t pos = base + (size_t)(compact ? j : col);
        weight_diff[pos] = weight_diff[pos] + s;
      }
    });
  }
  return ESCOIN_OK;
}

}  // namespace cpu
}  // namespace escoin

using namespace escoin;

extern "C" {

int escoin_backward_cpu(escoin_plan *plan, const float *bottom, const float *top, const float *top_diff,
                        float *bottom_diff, float *weight_diff, float *bias_diff, int n_images, int n_threads) {
  return guarded([&]() -> int {
    return cpu::backward_cpu<float>(plan, bottom, top, top_diff, bottom_diff, weight_diff, bias_diff, n_images, n_threads, false);
  });
}

int escoin_backward_cpu_f64(escoin_plan *plan, const double *bottom, const double *top, const double *top_diff,
                            double *bottom_diff, double *weight_diff, double *bias_diff, int n_images, int n_threads) {
  return guarded([&]() -> int {
    return cpu::backward_cpu<double>(plan, bottom, top, top_diff, bottom_diff, weight_diff, bias_diff, n_images,
                                     n_threads, false);
  });
}

int escoin_backward_values_cpu(escoin_plan *plan, const float *bottom, const float *top, const float *top_diff,
                               float *bottom_diff, float *values_diff, float *bias_diff, int n_images, int n_threads) {
  return guarded([&]() -> int {
    return cpu::backward_cpu<float>(plan, bottom, top, top_diff, bottom_diff, values_diff, bias_diff, n_images, n_threads, true);
  });
}

int escoin_backward_values_cpu_f64(escoin_plan *plan, const double *bottom, const double *top, const double *top_diff,
                                   double *bottom_diff, double *values_diff, double *bias_diff, int n_images,
                                   int n_threads) {
  return guarded([&]() -> int {
    return cpu::backward_cpu<double>(plan, bottom, top, top_diff, bottom_diff, values_diff, bias_diff, n_images,
                                     n_threads, true);
  });
}

}  // extern "C"
