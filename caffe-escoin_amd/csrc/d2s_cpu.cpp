// d2s_cpu.cpp -- option "deconv" in Caffe::CPU mode (include/escoin.h "Deconvolution"): the decomposition the device runs
// (d2s.hip), with host loops for the pack and the unpack around the library's own CPU kernels.  The inner plan lives on the
// host only (escoin_plan::cpu_inner): the inner descriptor of align_rules.h d2s_plan on the CSR of csr_tables.h d2s_csr.  It
// is built by the first CPU call after an align and takes the plan's current values through the entry map at every call,
// so every route that changes values (escoin_update_values_cpu, escoin_solver_step_cpu, escoin_plan_set_values, a
// device-source update read back) reaches it without a second path.
#include <algorithm>
#include <vector>

#include "escoin_plan.h"
#include "parallel_for.h"

namespace escoin {
namespace cpu {

// The host inner plan, current: built where missing, its values refreshed from the plan's.
static int inner_plan_cpu(escoin_plan *p, D2sPlan *dp, escoin_plan **out) {
  if (!d2s_plan(p->user_desc, p->is_f64, dp)) return fail(ESCOIN_EINVAL, dp->error);
  if (const int rcs = sync_host_values(p)) return rcs;     // (device-source weight updates: the values come back first)
  DerivedPlan &in = p->cpu_inner;
  const std::vector<float> flat = flat_entries(p->values);
  if (!in.plan) {
    DerivedCsr csr = d2s_csr(csr_view(p), *dp);
    escoin_plan *q = nullptr;
    int rc = escoin_plan_create(&dp->inner, &q);
    in.plan.reset(q);
    if (rc != ESCOIN_OK) return rc;
    if ((rc = escoin_plan_set_option(q, "cpu_images_per_job", p->cpu_img_force)) != ESCOIN_OK) return rc;
    if ((rc = escoin_plan_set_option(q, "cpu_channel_block", p->cpu_blk_force)) != ESCOIN_OK) return rc;
    std::vector<float> vals(csr.src.size());
    for (size_t k = 0; k < vals.size(); ++k) vals[k] = flat[(size_t)csr.src[k]];
    if ((rc = set_csr_host<float>(q, csr.rowptr.data(), csr.colidx.data(), vals.data(), csr.nnz_g.data())) != ESCOIN_OK) {
      in.plan.reset();
      return rc;
    }
    in.src = std::move(csr.src);
  } else {
    if (in.src.size() != flat.size()) return fail(ESCOIN_EINVAL, "deconv: the CPU mode's inner plan does not match the CSR");
    escoin_plan *q = in.plan.get();
    size_t k = 0;
    for (auto &grp : q->values)
      for (float &v : grp) v = flat[(size_t)in.src[k++]];
  }
  *out = in.plan.get();
  return ESCOIN_OK;
}

static int d2s_forward_cpu(escoin_plan *p, const float *bottom, const float *bias, float *top, int n_images, int n_threads) {
  D2sPlan dp;
  escoin_plan *ip = nullptr;
  if (const int rc = inner_plan_cpu(p, &dp, &ip)) return rc;
  const escoin_conv_desc &d = p->user_desc;
  if (n_images > d.N) return fail(ESCOIN_EINVAL, "n_images outside [0, desc.N]");
  const size_t Hi = (size_t)d.H + dp.inner.KH - 1, Wi = (size_t)d.W + dp.inner.KW - 1, P = (size_t)dp.P;
  p->cpu_t.resize((size_t)dp.t_floats);
  float *t = p->cpu_t.data();
  if (const int rc = escoin_forward_cpu(ip, bottom, nullptr, t, n_images, n_threads)) return rc;
  p->cpu_img_last = ip->cpu_img_last;
  p->cpu_blk_cb = ip->cpu_blk_cb;
  const bool relu = d.fuse_relu != 0;
  const size_t threads = (size_t)std::max(n_threads, 1);
  parallel_for((size_t)n_images * d.M, threads, [&](size_t nm) {
    const float b = bias ? bias[nm % (size_t)d.M] : 0.f;
    for (int oh = 0; oh < dp.OH; ++oh) {
      const size_t hp = (size_t)oh + d.pad_h, i = hp / dp.sh, ph = hp % dp.sh;
      float *drow = top + (nm * dp.OH + oh) * (size_t)dp.OW;
      for (int ow = 0; ow < dp.OW; ++ow) {
        const size_t wp = (size_t)ow + d.pad_w, j = wp / dp.sw, pw = wp % dp.sw;
        float v = t[((nm * P + ph * dp.sw + pw) * Hi + i) * Wi + j];
        if (bias) v += b;
        drow[ow] = relu ? (v > 0.f ? v : 0.f) : v;
      }
    }
  });
  return ESCOIN_OK;
}

static int d2s_backward_cpu(escoin_plan *p, const float *bottom, const float *top, const float *top_diff, float *bottom_diff,
                     float *weight_diff, float *bias_diff, int n_images, int n_threads, bool compact) {
  D2sPlan dp;
  escoin_plan *ip = nullptr;
  if (const int rc = inner_plan_cpu(p, &dp, &ip)) return rc;
  const escoin_conv_desc &d = p->user_desc;
  if (n_images > d.N) return fail(ESCOIN_EINVAL, "n_images outside [0, desc.N]");
  const size_t Hi = (size_t)d.H + dp.inner.KH - 1, Wi = (size_t)d.W + dp.inner.KW - 1, P = (size_t)dp.P;
  const bool relu = d.fuse_relu != 0;
  p->cpu_t.resize((size_t)dp.t_floats);
  float *g = p->cpu_t.data();
  const size_t threads = (size_t)std::max(n_threads, 1);
  parallel_for((size_t)n_images * d.M * P, threads, [&](size_t q) {
    const size_t nm = q / P, phase = q % P, ph = phase / dp.sw, pw = phase % dp.sw;
    for (size_t i = 0; i < Hi; ++i) {
      const long oh = (long)(i * dp.sh + ph) - d.pad_h;
      float *drow = g + (q * Hi + i) * Wi;
      for (size_t j = 0; j < Wi; ++j) {
        const long ow = (long)(j * dp.sw + pw) - d.pad_w;
        float v = 0.f;
        if (oh >= 0 && oh < dp.OH && ow >= 0 && ow < dp.OW) {
          const size_t at = (nm * dp.OH + (size_t)oh) * dp.OW + (size_t)ow;
          v = relu ? (top[at] > 0.f ? top_diff[at] : 0.f) : top_diff[at];
        }
        drow[j] = v;
      }
    }
  });
  const size_t nnz = ip ? p->cpu_inner.src.size() : 0;
  const bool want_w = weight_diff && nnz > 0;
  if (want_w) p->cpu_wv.assign(nnz, 0.f);
  if (bias_diff) p->cpu_bv.assign((size_t)dp.inner.M, 0.f);
  if (const int rc = escoin_backward_values_cpu(ip, want_w ? bottom : nullptr, nullptr, g, bottom_diff, want_w ? p->cpu_wv.data() : nullptr,
                                                bias_diff ? p->cpu_bv.data() : nullptr, n_images, n_threads))
    return rc;
  if (want_w) {
    const std::vector<int> &src = p->cpu_inner.src;
    if (compact) {
      for (size_t k = 0; k < nnz; ++k) weight_diff[(size_t)src[k]] += p->cpu_wv[k];
    } else {
      const std::vector<int> at = dense_positions(csr_view(p), p->g.kdim);
      for (size_t k = 0; k < nnz; ++k) weight_diff[(size_t)at[(size_t)src[k]]] += p->cpu_wv[k];
    }
  }
  if (bias_diff)
    for (int m = 0; m < d.M; ++m) {
      float s = 0.f;
      for (size_t ph = 0; ph < P; ++ph) s += p->cpu_bv[(size_t)m * P + ph];
      bias_diff[m] += s;
    }
  return ESCOIN_OK;
}

namespace {
__attribute__((used)) const bool g_registered = (g_d2s_cpu_hooks = D2sCpuHooks{d2s_forward_cpu, d2s_backward_cpu}, true);
}  // namespace

}  // namespace cpu
}  // namespace escoin
