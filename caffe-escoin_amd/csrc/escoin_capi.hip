// escoin_capi.hip -- host side of the C ABI declared in include/escoin.h:
// plan life cycle, WeightAlign (dense -> CSR -> device weight streams), dispatch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "align_rules.h"
#include "aligned_form.h"
#include "escoin_plan.h"
#include "prune_rules.h"

namespace escoin {

static thread_local std::string g_last_error;

S2dHooks g_s2d_hooks = {nullptr, nullptr, nullptr};
S2bHooks g_s2b_hooks = {nullptr, nullptr, nullptr, nullptr};
B2sHooks g_b2s_hooks = {nullptr, nullptr, nullptr, nullptr};
D2sHooks g_d2s_hooks = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
D2sCpuHooks g_d2s_cpu_hooks = {nullptr, nullptr};

void set_error(const std::string &msg) { g_last_error = msg; }

int fail(int code, const std::string &msg) {
  g_last_error = msg;
  return code;
}

int check_plan_device(const escoin_plan *p, const std::string &who) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev != p->device)
    return fail(ESCOIN_ESTATE, who + ": the current device is not the device the plan was aligned on");
  return ESCOIN_OK;
}

int check_n_images(const escoin_plan *p, int n_images) {
  if (n_images < 0 || n_images > p->g.d.N) return fail(ESCOIN_EINVAL, "n_images outside [0, desc.N]");
  return ESCOIN_OK;
}

template <typename T>
int set_csr_host(escoin_plan *p, const int *rowptr, const int *colidx, const T *values, const int *nnz_per_group);

static int out_dim(int in, int k, int pad, int stride, int dil) {
  // conv_layer.cpp:16-19
  return (in + 2 * pad - (dil * (k - 1) + 1)) / stride + 1;
}

static int validate(const escoin_conv_desc *d, Geometry *g) {
  if (!d) return fail(ESCOIN_EINVAL, "null descriptor");
  if (d->N < 1 || d->C < 1 || d->H < 1 || d->W < 1 || d->M < 1 || d->KH < 1 || d->KW < 1)
    return fail(ESCOIN_EINVAL, "non-positive dimension");
  if (d->pad_h < 0 || d->pad_w < 0 || d->stride_h < 1 || d->stride_w < 1 || d->dil_h < 1 ||
      d->dil_w < 1 || d->group < 1)
    return fail(ESCOIN_EINVAL, "bad pad/stride/dilation/group");
  // base_conv_layer.cpp:393-396: channels_ % group_ == 0, num_output_ % group_ == 0
  if (d->C % d->group != 0) return fail(ESCOIN_EINVAL, "channels not divisible by group");
  if (d->M % d->group != 0) return fail(ESCOIN_EINVAL, "num_output not divisible by group");
  if (d->KH > 255 || d->KW > 255 || d->C / d->group > 32767)
    return fail(ESCOIN_EINVAL, "kernel > 255 or > 32767 channels per group not supported");
  const int oh = out_dim(d->H, d->KH, d->pad_h, d->stride_h, d->dil_h);
  const int ow = out_dim(d->W, d->KW, d->pad_w, d->stride_w, d->dil_w);
  if (oh < 1 || ow < 1) return fail(ESCOIN_EINVAL, "empty output (kernel larger than padded input)");
  if (g) {
    g->d = *d;
    g->OH = oh;
    g->OW = ow;
    g->Cg = d->C / d->group;
    g->Mg = d->M / d->group;
    g->kdim = g->Cg * d->KH * d->KW;
  }
  return ESCOIN_OK;
}

DeviceBytes device_bytes(const escoin_plan *p) {
  const TiledArrays &t = p->tiled_dev;
  const DenseArrays &dn = p->dense;
  DeviceBytes b{p->gen.rowptr.bytes() + p->gen.taps.bytes() + p->gen.vals.bytes() + t.stream.bytes() + t.unit_hdr.bytes() +
                    t.chan.bytes() + t.jit.code_bytes + dn.w.bytes() + dn.ktab.bytes() + dn.sk_ws.bytes() + p->col.bytes(),
                0, 0, 0};
  if (const DenseWgradState *w = p->dwg.get()) b.dwg = w->ktab.bytes() + w->part.bytes();
  if (const UpdState *u = p->upd.get())
    b.upd = u->src.bytes() + u->off.bytes() + u->buf.bytes() + u->wpos.bytes() + u->stage.bytes() + u->e_ptr.bytes() + u->e_off.bytes() + u->e_buf.bytes();
  if (const BwdState *s = p->bwd.get())
    b.bwd = s->gather.bytes() + s->stg.bytes() + s->wgm.bytes() + s->pw.bytes() + s->dgm.bytes() + s->wpos.bytes() + s->slab.bytes() + s->g.bytes() +
            (s->transposed.plan ? device_bytes(s->transposed.plan.get()).fwd : 0);
  if (const S2dState *sd = p->s2d_state.get()) {
    // the X' / dX' scratch and the inner plan's own owners (its update state is never built: the plan's list reaches its copies)
    const DeviceBytes in = device_bytes(sd->inner.plan.get());
    b.fwd += sd->x.bytes() + in.fwd;
    b.bwd += in.bwd;
  }
  if (const S2bState *sb = p->s2b_state.get()) {
    // the X' / dX' and T' / G' scratches and the inner plan's own owners, as for "s2d"
    const DeviceBytes in = device_bytes(sb->inner.plan.get());
    b.fwd += sb->x.bytes() + sb->t.bytes() + in.fwd;
    b.bwd += in.bwd;
  }
  if (const B2sState *bs = p->b2s_state.get()) {
    // the X', T' / G' and dX' scratches and the inner plan's own owners, as for "s2d"
    const DeviceBytes in = device_bytes(bs->inner.plan.get());
    b.fwd += bs->x.bytes() + bs->t.bytes() + bs->dx.bytes() + in.fwd;
    b.bwd += in.bwd;
    b.dwg += in.dwg;      // (escoin_dense_wgrad runs on the inner plan)
  }
  if (const D2sState *ds = p->d2s_state.get()) {
    // the T' / G' scratch, the gradients' scratches and maps, and the inner plan's own owners, as for "s2d"
    const DeviceBytes in = device_bytes(ds->inner.plan.get());
    b.fwd += ds->scratch_bytes() + in.fwd;
    b.bwd += in.bwd;
  }
  return b;
}

long bwd_stat(const escoin_plan *p, const char *key) {
  // option "b2s": the whole backward is the inner plan's, and so are its facts -- but for the bytes, which device_bytes sums
  if (p->b2s_state && strcmp(key, "bwd_device_bytes") != 0) return bwd_stat(p->b2s_state->inner.plan.get(), key);
  if (p->d2s_state && strcmp(key, "bwd_device_bytes") != 0) return bwd_stat(p->d2s_state->inner.plan.get(), key);   // (option "deconv": likewise)
  const BwdState *s = p->bwd.get();
  if (!strcmp(key, "bwd_data_kernel")) {
    if (!s) return fail(ESCOIN_ESTATE, "bwd_data_kernel: no backward has run on this alignment");
    if (s->data == kBwdInner) return bwd_stat(p->inner_plan()->plan.get(), key);
    if (s->data == kBwdTransposed) return escoin_plan_stat(s->transposed.plan.get(), "kernel_choice");
    return s->data == kBwdMfma ? ESCOIN_BWD_MFMA : ESCOIN_KERNEL_GENERIC;
  }
  if (!strcmp(key, "bwd_device_bytes")) return (long)device_bytes(p).bwd;
  if (!strcmp(key, "bwd_chunks")) return s ? s->last_chunks : 0;
  if (!strcmp(key, "wgrad_kernel")) {
    if (!s || !s->last_wgrad) return fail(ESCOIN_ESTATE, "wgrad_kernel: no weight / bias gradient has run on this alignment");
    return s->last_wgrad;
  }
  if (!strcmp(key, "wgrad_lds_bytes")) {
    if (s && s->wgrad == ESCOIN_WGRAD_MFMA) return (long)s->wgm.lds_bytes;
    if (s && s->wgrad == ESCOIN_WGRAD_POINTWISE) return (long)s->pw.lds_bytes;
    return s && s->wgrad == ESCOIN_WGRAD_STAGED ? (long)s->stg.lds_bytes : 0;
  }
  if (!strcmp(key, "dgrad_lds_bytes")) return s && s->data == kBwdMfma ? (long)s->dgm.lds_bytes : 0;
  if (!strcmp(key, "bwd_align_us")) return s ? (long)(s->align_ms * 1e3) : 0;
  return fail(ESCOIN_EINVAL, std::string("unknown stat: ") + key);
}

int sync_host_values(escoin_plan *p) {
  if (!p || !p->dev_authoritative || !p->sync_host_fn) return ESCOIN_OK;
  return p->sync_host_fn(p);
}

long upd_stat(const escoin_plan *p, const char *key) {
  if (!strcmp(key, "update_fast")) return p->upd_last_fast;
  if (!strcmp(key, "update_count")) return p->upd_count;
  if (!strcmp(key, "update_destinations")) return p->upd ? p->upd->n_dst : 0;
  if (!strcmp(key, "upd_device_bytes")) return (long)device_bytes(p).upd;
  return fail(ESCOIN_EINVAL, std::string("unknown stat: ") + key);
}

long dwg_stat(const escoin_plan *p, const char *key) {
  // (option "b2s": the state is the inner plan's)
  const DenseWgradState *w = p->b2s_state ? p->b2s_state->inner.plan->dwg.get() : p->dwg.get();
  if (!strcmp(key, "dwg_device_bytes")) return (long)device_bytes(p).dwg;
  if (!strcmp(key, "dwg_splits")) return w ? w->splits : 0;
  if (!strcmp(key, "dwg_lds_bytes")) return w ? (long)w->lds_bytes : 0;
  if (!strcmp(key, "dwg_count")) return p->dwg_count;
  return fail(ESCOIN_EINVAL, std::string("unknown stat: ") + key);
}

// (the dense weight gradient's state, p->dwg, is a function of the descriptor alone: no align frees it)
static void free_device(escoin_plan *p) {
  p->upd.reset();
  p->dev_authoritative = false;
  p->bwd.reset();
  p->s2d_state.reset();
  p->s2b_state.reset();
  p->b2s_state.reset();
  p->d2s_state.reset();
  p->gen = GenericArrays();
  tiled_release(p);
  p->col.reset();
  p->dense = DenseArrays();
}

// The generic kernel's device CSR (p->gen) from the host CSR: rowptr, packed taps and values of the plan's Dtype.
template <typename T>
static int upload_generic(escoin_plan *p, hipStream_t stream) {
  const GenericTables t = generic_tables(csr_view(p));
  const std::vector<T> vals = flat_entries(plan_vals<T>(p), 1);
  ESCOIN_HIP_TRY(p->gen.rowptr.upload(t.rowptr, stream));
  ESCOIN_HIP_TRY(p->gen.taps.upload(t.taps, stream));
  ESCOIN_HIP_TRY(p->gen.vals.upload(vals, stream));
  ESCOIN_HIP_TRY(hipStreamSynchronize(stream));  // host vectors die at scope exit
  return ESCOIN_OK;
}

int build_derived_plan(const escoin_plan *owner, const escoin_conv_desc &desc, int kernel, int backward_kernel,
                       DerivedCsr csr, hipStream_t stream, DerivedPlan *out, int tiling_batch, bool wgrad_options) {
  escoin_plan *q = nullptr;
  int rc = escoin_plan_create(&desc, &q);
  out->plan.reset(q);
  if (rc != ESCOIN_OK) return rc;
  // what a derived plan inherits, and all of it ("body_variant", "code_touchers" and "stream_stores" are not handed down, the "wgrad_*"
  // options only where the derived plan computes the weight gradient)
  if ((rc = escoin_plan_set_option(q, "kernel", kernel)) != ESCOIN_OK) return rc;
  if ((rc = escoin_plan_set_option(q, "backward_kernel", backward_kernel)) != ESCOIN_OK) return rc;
  if ((rc = escoin_plan_set_option(q, "tiling_batch", tiling_batch < 0 ? owner->tiling_batch : tiling_batch)) != ESCOIN_OK) return rc;
  if ((rc = escoin_plan_set_option(q, "max_launch_bytes", (int)std::min<long>(owner->max_launch_bytes, 0x7fffffff))) != ESCOIN_OK) return rc;
  if ((rc = escoin_plan_set_option(q, "dense_threshold_pct", owner->dense_threshold_pct)) != ESCOIN_OK) return rc;
  if ((rc = escoin_plan_set_option(q, "dense_gate", owner->dense_gate)) != ESCOIN_OK) return rc;
  if ((rc = escoin_plan_set_option(q, "code_loader", owner->code_loader)) != ESCOIN_OK) return rc;
  if (wgrad_options) {
    if ((rc = escoin_plan_set_option(q, "wgrad_kernel", owner->wgrad_kernel)) != ESCOIN_OK) return rc;
    if ((rc = escoin_plan_set_option(q, "wgrad_channel_block", owner->wgrad_channel_block)) != ESCOIN_OK) return rc;
    if ((rc = escoin_plan_set_option(q, "wgrad_pointwise", owner->wgrad_pointwise)) != ESCOIN_OK) return rc;
    if ((rc = escoin_plan_set_option(q, "wgrad_pointwise_tile_entries", owner->wgrad_pw_tile_entries)) != ESCOIN_OK) return rc;
  }
  const std::vector<float> flat = flat_entries(owner->values);
  std::vector<float> vals(csr.src.size());
  for (size_t k = 0; k < vals.size(); ++k) vals[k] = flat[(size_t)csr.src[k]];
  if ((rc = escoin_plan_set_csr(q, csr.rowptr.data(), csr.colidx.data(), vals.data(), csr.nnz_g.data(), stream)) != ESCOIN_OK) return rc;
  out->src = std::move(csr.src);
  return ESCOIN_OK;
}

// Option "s2d" (include/escoin.h "Space-to-depth"): the inner stride-1 plan with the plan's kernel options, aligned on the
// inner CSR, and the X' scratch.  The plan itself keeps the generic arrays alone (the weight gradient walks them, and
// gen.vals is the value array of the in-place updates).
static int s2d_build(escoin_plan *p, const S2dPlan &sp, hipStream_t stream) {
  if (!g_s2d_hooks.pack || !g_s2d_hooks.unpack) return fail(ESCOIN_EINVAL, "option \"s2d\": this build does not carry the space-to-depth kernels");
  p->s2d_state.reset(new S2dState());
  S2dState *sd = p->s2d_state.get();
  sd->sp = sp;
  // the data gradient's kernel: GENERIC and BWD_MFMA stay with this plan (its gather / MFMA kernels), the others go to the inner plan
  const int ibwd = p->bwd_kernel == ESCOIN_KERNEL_GENERIC || p->bwd_kernel == ESCOIN_BWD_MFMA ? ESCOIN_KERNEL_AUTO : p->bwd_kernel;
  const int rc = build_derived_plan(p, sp.inner, p->kernel_choice, ibwd, s2d_csr(csr_view(p), sp), stream, &sd->inner);
  if (rc != ESCOIN_OK) return rc;
  escoin_plan *ip = sd->inner.plan.get();
  ESCOIN_HIP_TRY(sd->x.alloc(sizeof(float) * (size_t)sp.x_floats));
  p->n_dense_groups = 0; p->n_sparse_groups = p->g.d.group; p->use_dense = false;
  p->dense_mask = 0; p->sparse_mask = ~0ull; p->small_rule = 0; p->import_fast = false;
  p->kernel_name = std::string(g_s2d_hooks.pack_kernel_name) + " + " + escoin_plan_kernel_name(ip);
  p->aligned = true;
  return ESCOIN_OK;
}

// Option "s2b" (include/escoin.h "Space-to-batch"): the inner undilated plan of N * P images with the plan's kernel options,
// aligned on the plan's own CSR (the entry map is the identity), and the X' and T' scratches.  The plan itself keeps the
// generic arrays alone, as under "s2d".
static int s2b_build(escoin_plan *p, const S2bPlan &sp, hipStream_t stream) {
  if (!g_s2b_hooks.pack || !g_s2b_hooks.unpack) return fail(ESCOIN_EINVAL, "option \"s2b\": this build does not carry the space-to-batch kernels");
  p->s2b_state.reset(new S2bState());
  S2bState *sb = p->s2b_state.get();
  sb->sp = sp;
  const int ibwd = p->bwd_kernel == ESCOIN_KERNEL_GENERIC || p->bwd_kernel == ESCOIN_BWD_MFMA ? ESCOIN_KERNEL_AUTO : p->bwd_kernel;
  DerivedCsr csr;
  for (int grp = 0; grp < p->g.d.group; ++grp) {
    csr.rowptr.insert(csr.rowptr.end(), p->rowptr[grp].begin(), p->rowptr[grp].end());
    csr.colidx.insert(csr.colidx.end(), p->colidx[grp].begin(), p->colidx[grp].end());
    csr.nnz_g.push_back((int)p->colidx[grp].size());
  }
  csr.src.resize(csr.colidx.size());
  for (size_t k = 0; k < csr.src.size(); ++k) csr.src[k] = (int)k;
  // "tiling_batch" counts outer images: an outer image is P inner ones
  const long tb = (long)p->tiling_batch * sp.eh * sp.ew;
  if (tb > 0x7fffffffL) return fail(ESCOIN_EINVAL, "option \"s2b\": tiling_batch times the residue classes exceeds 2^31");
  const int rc = build_derived_plan(p, sp.inner, p->kernel_choice, ibwd, std::move(csr), stream, &sb->inner, (int)tb);
  if (rc != ESCOIN_OK) return rc;
  ESCOIN_HIP_TRY(sb->x.alloc(sizeof(float) * (size_t)sp.x_floats));
  ESCOIN_HIP_TRY(sb->t.alloc(sizeof(float) * (size_t)sp.t_floats));
  p->n_dense_groups = 0; p->n_sparse_groups = p->g.d.group; p->use_dense = false;
  p->dense_mask = 0; p->sparse_mask = ~0ull; p->small_rule = 0; p->import_fast = false;
  p->kernel_name = std::string(g_s2b_hooks.pack_kernel_name) + " + " + escoin_plan_kernel_name(sb->inner.plan.get()) + " + " +
                   g_s2b_hooks.unpack_kernel_name;
  p->aligned = true;
  return ESCOIN_OK;
}

// Option "b2s" (include/escoin.h "Batch-to-space"): the inner pointwise plan of ceil(N / B) images of 1 x B with the plan's
// kernel, backward and weight-gradient options, aligned on the plan's own CSR (the entry map is the identity), and the X',
// T' / G' and dX' scratches.  The plan itself keeps the generic arrays alone, as under "s2d".
static int b2s_build(escoin_plan *p, const B2sPlan &bp, hipStream_t stream) {
  if (!g_b2s_hooks.pack || !g_b2s_hooks.unpack) return fail(ESCOIN_EINVAL, "option \"b2s\": this build does not carry the batch-to-space kernels");
  p->b2s_state.reset(new B2sState());
  B2sState *bs = p->b2s_state.get();
  bs->bp = bp;
  DerivedCsr csr;
  for (int grp = 0; grp < p->g.d.group; ++grp) {
    csr.rowptr.insert(csr.rowptr.end(), p->rowptr[grp].begin(), p->rowptr[grp].end());
    csr.colidx.insert(csr.colidx.end(), p->colidx[grp].begin(), p->colidx[grp].end());
    csr.nnz_g.push_back((int)p->colidx[grp].size());
  }
  csr.src.resize(csr.colidx.size());
  for (size_t k = 0; k < csr.src.size(); ++k) csr.src[k] = (int)k;
  // "tiling_batch" counts outer images: B of them are one inner image
  const int tb = (int)(((long)p->tiling_batch + bp.B - 1) / bp.B);
  const int rc = build_derived_plan(p, bp.inner, p->kernel_choice, p->bwd_kernel, std::move(csr), stream, &bs->inner, tb, true);
  if (rc != ESCOIN_OK) return rc;
  ESCOIN_HIP_TRY(bs->x.alloc(sizeof(float) * (size_t)bp.x_floats));
  ESCOIN_HIP_TRY(bs->t.alloc(sizeof(float) * (size_t)bp.t_floats));
  ESCOIN_HIP_TRY(bs->dx.alloc(sizeof(float) * (size_t)bp.x_floats));
  p->n_dense_groups = 0; p->n_sparse_groups = p->g.d.group; p->use_dense = false;
  p->dense_mask = 0; p->sparse_mask = ~0ull; p->small_rule = 0; p->import_fast = false;
  p->kernel_name = std::string(g_b2s_hooks.pack_kernel_name) + " + " + escoin_plan_kernel_name(bs->inner.plan.get()) + " + " +
                   g_b2s_hooks.unpack_kernel_name;
  p->aligned = true;
  return ESCOIN_OK;
}

// What every align of an option "deconv" plan asks first (the device aligns, and escoin_weight_align_cpu): whether d2s_plan
// serves the layer for this Dtype, and that no other derived-plan option is set.  ESCOIN_OK on other plans.
int deconv_precheck(const escoin_plan *p, bool is_f64) {
  if (!p->deconv) return ESCOIN_OK;
  D2sPlan dp;
  if (!d2s_plan(p->user_desc, is_f64, &dp)) return fail(ESCOIN_EINVAL, dp.error);
  if (p->s2d || p->s2b || p->b2s) return fail(ESCOIN_EINVAL, "option \"deconv\" does not combine with \"s2d\", \"s2b\" or \"b2s\"");
  return ESCOIN_OK;
}

// Option "deconv" (include/escoin.h "Deconvolution"): the inner stride-1 plan of M * P output channels with the plan's kernel,
// backward and weight-gradient options, aligned on d2s_csr of the plan's CSR, the T' / G' scratch, and what the backward's
// tail needs: the two gradient scratches and the entry map and blobs_[0] positions on the device.  The plan itself keeps the
// generic arrays alone, as under "s2d" (gen.vals is the value array of the in-place updates); no kernel reads them.
static int d2s_build(escoin_plan *p, const D2sPlan &dp, hipStream_t stream) {
  if (!g_d2s_hooks.pack || !g_d2s_hooks.unpack) return fail(ESCOIN_EINVAL, "option \"deconv\": this build does not carry the depth-to-space kernels");
  p->d2s_state.reset(new D2sState());
  D2sState *ds = p->d2s_state.get();
  ds->dp = dp;
  int rc = build_derived_plan(p, dp.inner, p->kernel_choice, p->bwd_kernel, d2s_csr(csr_view(p), dp), stream, &ds->inner, -1, true);
  if (rc != ESCOIN_OK) return rc;
  escoin_plan *ip = ds->inner.plan.get();
  if (p->conv_mode != ip->conv_mode && (rc = escoin_plan_set_option(ip, "conv_mode", p->conv_mode)) != ESCOIN_OK) return rc;
  const size_t nz = (size_t)std::max<long>(plan_nnz(p), 1);
  ESCOIN_HIP_TRY(ds->t.alloc(sizeof(float) * (size_t)dp.t_floats));
  ESCOIN_HIP_TRY(ds->wv.alloc(sizeof(float) * nz));
  ESCOIN_HIP_TRY(ds->bv.alloc(sizeof(float) * (size_t)dp.inner.M));
  std::vector<int> src(ds->inner.src), wpos(nz, 0);
  const std::vector<int> at = dense_positions(csr_view(p), p->g.kdim);
  for (size_t k = 0; k < src.size(); ++k) wpos[k] = at[(size_t)src[k]];
  src.resize(nz, 0);
  ESCOIN_HIP_TRY(ds->src.upload(src, stream));
  ESCOIN_HIP_TRY(ds->wpos.upload(wpos, stream));
  ESCOIN_HIP_TRY(hipStreamSynchronize(stream));  // host vectors die at scope exit
  p->n_dense_groups = 0; p->n_sparse_groups = p->g.d.group; p->use_dense = false;
  p->dense_mask = 0; p->sparse_mask = ~0ull; p->small_rule = 0; p->import_fast = false;
  p->kernel_name = std::string(escoin_plan_kernel_name(ip)) + " + " + g_d2s_hooks.unpack_kernel_name;
  p->aligned = true;
  return ESCOIN_OK;
}

// Uploads the CSR held in p->rowptr/colidx/values and builds the kernel-specific
// streams.  Shared tail of escoin_weight_align and escoin_plan_set_csr.
//   jit_blob: the generated-code section of a persisted aligned form (escoin_plan_import_aligned), tried
//   where the generator would otherwise run.
static int upload(escoin_plan *p, hipStream_t stream, const char *jit_blob = nullptr, size_t jit_blob_bytes = 0) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail(ESCOIN_ENODEVICE, "no HIP device: escoin_weight_align / set_csr / import_aligned prepare the GPU path (Caffe::CPU mode has its own entry points: escoin_weight_align_cpu, escoin_forward_cpu)");
  ESCOIN_HIP_TRY(hipGetDevice(&p->device));
  free_device(p);
  if (const int rc = deconv_precheck(p, p->is_f64)) return rc;
  const Geometry &g = p->g;
  const int rc_gen = p->is_f64 ? upload_generic<double>(p, stream) : upload_generic<float>(p, stream);
  if (rc_gen != ESCOIN_OK) return rc_gen;
  if (p->is_f64) {
    // Dtype = double: the order-preserving generic kernel is the only device kernel a double plan runs, in every
    // conv_mode (fp64 vector FMA is native on gfx950; the LDS-tiled, generated-code and MFMA kernels are fp32: north_star
    // measures fp32, double is boundary completeness, conv_layer.cu:75).
    p->n_dense_groups = 0; p->n_sparse_groups = g.d.group; p->use_dense = false;
    p->dense_mask = 0; p->sparse_mask = ~0ull; p->small_rule = 0; p->import_fast = false;
    p->kernel_name = generic_kernel_name_f64(g.d.fuse_relu != 0);
    p->aligned = true;
    return ESCOIN_OK;
  }
  // option "deconv": the layer runs through the stride-1 inner plan in every conv_mode (the inner plan takes the mode); there
  // is no kernel of the plan's own to fall back to
  if (p->deconv) {
    D2sPlan d2p;
    d2s_plan(p->user_desc, false, &d2p);      // (deconv_precheck has asked)
    const int rc = d2s_build(p, d2p, stream);
    if (rc != ESCOIN_OK) p->d2s_state.reset();
    return rc;
  }
  const bool direct_mode = p->conv_mode == ESCOIN_CONV_MODE_SCONV || p->conv_mode == ESCOIN_CONV_MODE_SCONV_PAR;
  // option "b2s": an inner-product layer runs through a pointwise inner plan whose pixel axis is the batch.  Asked first: a
  // one-pixel layer whose descriptor names a stride or a dilation is this option's, whatever "s2d" / "s2b" say
  B2sPlan b2p;
  if (p->b2s && direct_mode && b2s_plan(g, false, p->b2s_block, tiled_device_cus(), &b2p)) {
    const int rc = b2s_build(p, b2p, stream);
    if (rc != ESCOIN_OK) p->b2s_state.reset();
    return rc;
  }
  // option "s2d": the layer runs through a stride-1 inner plan, which alone decides dense or sparse, tiled or generic,
  // on its own geometry (the 4 % rule of dense_groups() for layers without a fast kernel is what the option removes)
  S2dPlan s2p;
  if (p->s2d && (p->conv_mode == ESCOIN_CONV_MODE_SCONV || p->conv_mode == ESCOIN_CONV_MODE_SCONV_PAR) && s2d_plan(g, false, &s2p)) {
    const int rc = s2d_build(p, s2p, stream);
    if (rc != ESCOIN_OK) p->s2d_state.reset();
    return rc;
  }
  // option "s2b": likewise for a dilated stride-1 layer, through an undilated inner plan of N * P images
  S2bPlan s2bp;
  if (p->s2b && (p->conv_mode == ESCOIN_CONV_MODE_SCONV || p->conv_mode == ESCOIN_CONV_MODE_SCONV_PAR) && s2b_plan(g, false, &s2bp)) {
    const int rc = s2b_build(p, s2bp, stream);
    if (rc != ESCOIN_OK) p->s2b_state.reset();
    return rc;
  }
  // A forced TILED / JIT on a layer that "s2d" / "s2b" serves in the direct modes names the INNER plan's kernel: the layer's own
  // geometry (a stride, a dilation) has no tiled kernel.  Here the plan stands in a lowered mode, which runs on that geometry
  // without the inner plan, and aligns as under KERNEL_AUTO instead of refusing -- a conv_mode flip left such a plan unaligned.
  int kernel = p->kernel_choice;
  if ((kernel == ESCOIN_KERNEL_TILED || kernel == ESCOIN_KERNEL_JIT) && !tiled_supported(g) &&
      ((p->s2d && s2d_plan(g, false, &s2p)) || (p->s2b && s2b_plan(g, false, &s2bp)) ||
       (p->b2s && b2s_plan(g, false, p->b2s_block, tiled_device_cus(), &b2p))))
    kernel = ESCOIN_KERNEL_AUTO;
  // which conv groups go to the dense (fp32 MFMA) kernel (align_rules.h)
  const int G = g.d.group;
  std::vector<long> nnz_per_group(G);
  for (int grp = 0; grp < G; ++grp) nnz_per_group[grp] = (long)p->colidx[grp].size();
  const GroupSplit split = group_split(dense_groups(
      g, nnz_per_group, SplitOptions{kernel, p->conv_mode, p->dense_gate, p->dense_threshold_pct, p->tiling_batch},
      tiled_device_cus()));
  p->n_dense_groups = split.n_dense;
  p->n_sparse_groups = split.n_sparse;
  p->use_dense = split.use_dense;
  p->dense_mask = split.dense_mask;
  p->sparse_mask = split.sparse_mask;
  if (p->n_dense_groups > 0) {
    const size_t lda = (size_t)dense_lda(g.kdim);
    std::vector<float> dw(((size_t)g.d.M + dense_spare_rows()) * lda, 0.f);
    const std::vector<int> at = dense_positions(csr_view(p), (int)lda);
    const std::vector<float> vals = flat_entries(p->values);
    for (size_t e = 0; e < vals.size(); ++e) dw[(size_t)at[e]] = vals[e];
    ESCOIN_HIP_TRY(p->dense.w.upload(dw, stream));
    ESCOIN_HIP_TRY(hipStreamSynchronize(stream));
    const int rc = dense_build_ktab(p, stream);
    if (rc != ESCOIN_OK) return rc;
  }
  if (p->use_dense) {
    p->kernel_name = dense_kernel_name();
    p->aligned = true;
    return ESCOIN_OK;
  }
  p->small_rule = 0;
  const bool explicit_tiled = kernel == ESCOIN_KERNEL_TILED || kernel == ESCOIN_KERNEL_JIT;
  const bool want_tiled = explicit_tiled || (kernel == ESCOIN_KERNEL_AUTO && tiled_supported(g));
  if (want_tiled) {
    if (!tiled_supported(g))
      return fail(ESCOIN_EINVAL, "tiled kernel requested for a geometry it does not support");
    // AUTO: generated code (jit_codegen.h) wherever the sparse path runs.  Round 3 cut it off at 18 %
    // density (25 % for layers of at most 100 k nonzeros) because AlexNet's 13 x 13 layers lost 9-14 % to
    // the stream kernel at 80 % sparsity and below; that loss was the eight L2s each streaming every
    // column's code, and grouping the workgroup columns by XCD (sconv_tiled.hip, xcd_q) removed it:
    // over 50-95 % sparsity on every BASELINE 3x3 / 5x5 / 1x1 shape generated code is now ahead of the
    // stream kernel at every point (profiles/r04_crossover.md; the worst point, alex_conv2 @50 %, by 14 %).
    // Code beyond kMaxJitBytes (geometry.h) falls back to the stream kernel by itself.
    const bool try_jit = kernel == ESCOIN_KERNEL_JIT || kernel == ESCOIN_KERNEL_AUTO;
    int rc = ESCOIN_OK;
    p->import_fast = false;
    p->small_rule = 0;     // (set by tiled_build / tiled_import from the tiling, before any code is generated or loaded)
    if (try_jit && jit_blob && jit_blob_bytes > 0) {
      rc = tiled_import(p, jit_blob, jit_blob_bytes, stream);     // (leaves tiled.enabled false when the blob does not fit)
      if (rc != ESCOIN_OK) return rc;
      p->import_fast = p->tiled.enabled;
    }
    if (try_jit && !p->tiled.enabled && p->small_rule != 2) {
      rc = tiled_build(p, stream, true);
      if (rc != ESCOIN_OK && kernel == ESCOIN_KERNEL_JIT) return rc;
      if (!p->tiled.enabled && kernel == ESCOIN_KERNEL_JIT)
        return fail(ESCOIN_EINVAL, "generated-code kernel requested but the layer does not fit it");
      if (rc != ESCOIN_OK) {
        // KERNEL_AUTO: a failure of the code path (code object manager, module load, an allocation)
        // is not the layer's failure -- the stream kernel runs it.  Whatever the attempt left on the
        // device is released first, and the reason is not lost.
        if (getenv("ESCOIN_VERBOSE"))
          fprintf(stderr, "[escoin] generated code unavailable for this layer (%s): falling back to the stream kernel\n",
                  g_last_error.c_str());
        const float dens = p->tiled.density;
        tiled_release(p);
        p->tiled.density = dens;
        rc = ESCOIN_OK;
      }
    }
    if (!p->tiled.enabled && p->small_rule != 2) {
      rc = tiled_build(p, stream, false);   // leaves tiled.enabled false when the stream does not fit LDS
      if (rc != ESCOIN_OK) return rc;
    }
    if (!p->tiled.enabled && kernel == ESCOIN_KERNEL_TILED)
      return fail(ESCOIN_EINVAL, "tiled kernel requested but its weight stream does not fit the LDS budget");
  }
  p->kernel_name = p->tiled.enabled ? tiled_kernel_name(p) : generic_kernel_name(g.d.fuse_relu != 0);
  if (p->n_dense_groups > 0) p->kernel_name += std::string(" + ") + dense_kernel_name();
  p->aligned = true;
  return ESCOIN_OK;
}


int realign_from_host_csr(escoin_plan *p, hipStream_t stream) { return upload(p, stream); }

template <typename T>
void csr_from_dense(escoin_plan *p, const T *w) {
  const Geometry &g = p->g;
  // caffe_cpu_sparse_dense2csr, math_functions.cpp:92-105: row-major scan, keep != 0
  const size_t weight_offset = (size_t)g.Mg * g.kdim;  // base_conv_layer.cpp:60
  p->aligned = false;
  p->host_aligned = false;
  free_device(p);
  p->is_f64 = sizeof(T) == 8;
  std::vector<std::vector<T>> &vals = plan_vals<T>(p);
  for (int grp = 0; grp < g.d.group; ++grp) {
    std::vector<int> &rp = p->rowptr[grp];
    std::vector<int> &ci = p->colidx[grp];
    std::vector<T> &va = vals[grp];
    rp.assign(g.Mg + 1, 0);
    ci.clear();
    va.clear();
    p->values[grp].clear();
    p->values64[grp].clear();
    const T *A = w + weight_offset * grp;
    for (int i = 0; i < g.Mg; ++i) {
      for (int j = 0; j < g.kdim; ++j) {
        const T v = A[(size_t)i * g.kdim + j];
        if (v != 0) {
          va.push_back(v);
          ci.push_back(j);
        }
      }
      rp[i + 1] = (int)ci.size();
    }
  }
  p->cpu_off_valid = false;
  p->cpu_inner.plan.reset();
  p->host_aligned = true;
}
template void csr_from_dense<float>(escoin_plan *, const float *);
template void csr_from_dense<double>(escoin_plan *, const double *);

template <typename T>
static int weight_align_t(escoin_plan *p, const T *dense_w, int w_on_device, void *stream) {
  if (!p || !dense_w) return fail(ESCOIN_EINVAL, "null argument");
  if (const int rc = deconv_precheck(p, sizeof(T) == 8)) return rc;     // (before anything is read through the geometry)
  const auto t_start = std::chrono::steady_clock::now();
  const Geometry &g = p->g;
  const size_t count = (size_t)g.d.M * g.kdim;
  std::vector<T> host;
  const T *w = dense_w;
  if (w_on_device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
      return fail(ESCOIN_ENODEVICE, "no HIP device: cannot read device weights");
    host.resize(count);
    ESCOIN_HIP_TRY(hipMemcpyAsync(host.data(), dense_w, sizeof(T) * count, hipMemcpyDeviceToHost, (hipStream_t)stream));
    ESCOIN_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    w = host.data();
  }
  csr_from_dense<T>(p, w);
  const int rc = upload(p, (hipStream_t)stream);
  p->align_ms = ms_since(t_start);
  return rc;
}

template <typename T>
static int set_csr_t(escoin_plan *p, const int *rowptr, const int *colidx, const T *values, const int *nnz_per_group,
                     void *stream) {
  const auto t_start = std::chrono::steady_clock::now();
  if (p)
    if (const int rc = deconv_precheck(p, sizeof(T) == 8)) return rc;
  const int rc = set_csr_host<T>(p, rowptr, colidx, values, nnz_per_group);
  if (rc != ESCOIN_OK) return rc;
  const int rc2 = upload(p, (hipStream_t)stream);
  p->align_ms = ms_since(t_start);
  return rc2;
}

template <typename T>
static int get_csr_t(const escoin_plan *p, int *rowptr, int *colidx, T *values, int stretched) {
  if (!p || !rowptr) return fail(ESCOIN_EINVAL, "null argument");
  if (values && p->host_aligned && p->is_f64 != (sizeof(T) == 8))
    return fail(ESCOIN_ESTATE, p->is_f64 ? "get_csr: the plan holds double values (use escoin_plan_get_csr_f64)"
                                         : "get_csr_f64: the plan holds float values (use escoin_plan_get_csr)");
  if (const int rc = sync_host_values(const_cast<escoin_plan *>(p))) return rc;
  const Geometry &g = p->g;
  const std::vector<std::vector<T>> &vals = plan_vals<T>(const_cast<escoin_plan *>(p));
  long base = 0;
  for (int grp = 0; grp < g.d.group; ++grp) {
    memcpy(rowptr + (size_t)grp * (g.Mg + 1), p->rowptr[grp].data(), sizeof(int) * (g.Mg + 1));
    const long n_g = (long)p->colidx[grp].size();
    for (long j = 0; j < n_g; ++j) {
      int col = p->colidx[grp][j];
      if (stretched) col = stretched_col(col, g.d);
      if (colidx) colidx[base + j] = col;
      if (values) values[base + j] = vals[grp][j];
    }
    base += n_g;
  }
  return ESCOIN_OK;
}

}  // namespace escoin

using namespace escoin;

extern "C" {

const char *escoin_last_error(void) { return g_last_error.c_str(); }

int escoin_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int escoin_out_shape(const escoin_conv_desc *desc, int *out_h, int *out_w) {
  Geometry g;
  int rc = validate(desc, &g);
  if (rc != ESCOIN_OK) return rc;
  if (out_h) *out_h = g.OH;
  if (out_w) *out_w = g.OW;
  return ESCOIN_OK;
}

int escoin_deconv_out_shape(const escoin_conv_desc *desc, int *out_h, int *out_w) {
  if (!desc) return fail(ESCOIN_EINVAL, "null descriptor");
  if (desc->N < 1 || desc->C < 1 || desc->H < 1 || desc->W < 1 || desc->M < 1 || desc->KH < 1 || desc->KW < 1)
    return fail(ESCOIN_EINVAL, "non-positive dimension");
  if (desc->pad_h < 0 || desc->pad_w < 0 || desc->stride_h < 1 || desc->stride_w < 1 || desc->dil_h < 1 || desc->dil_w < 1 || desc->group < 1)
    return fail(ESCOIN_EINVAL, "bad pad/stride/dilation/group");
  // deconv_layer.cpp compute_output_shape: stride * (in - 1) + dilation * (kernel - 1) + 1 - 2 * pad
  const long oh = (long)desc->stride_h * (desc->H - 1) + (long)desc->dil_h * (desc->KH - 1) + 1 - 2L * desc->pad_h;
  const long ow = (long)desc->stride_w * (desc->W - 1) + (long)desc->dil_w * (desc->KW - 1) + 1 - 2L * desc->pad_w;
  if (oh < 1 || ow < 1 || oh > 0x7fffffffL || ow > 0x7fffffffL) return fail(ESCOIN_EINVAL, "empty or oversized output");
  if (out_h) *out_h = (int)oh;
  if (out_w) *out_w = (int)ow;
  return ESCOIN_OK;
}

long escoin_padded_len(const escoin_conv_desc *d) {
  if (!d) return fail(ESCOIN_EINVAL, "null descriptor");
  // base_conv_layer.cpp:71, plus the pad_w floats that formula forgets when pad_h == 0 < pad_w: the last row's right
  // padding is read out of the floats that follow the row, and without a bottom padding row nothing follows the last
  // channel's last row (the reference's kernels read past its allocation there; none of its models has such a layer).
  // A buffer of this length, zeroed once, is safe for every entry point of this library.
  return (long)d->C * (d->H + d->pad_h) * (d->W + d->pad_w) + (long)d->pad_h * (d->W + 2 * d->pad_w) +
         (d->pad_h == 0 ? d->pad_w : 0);
}

int escoin_plan_create(const escoin_conv_desc *desc, escoin_plan **plan) {
  return guarded([&]() -> int {
    if (!plan) return fail(ESCOIN_EINVAL, "null plan pointer");
    *plan = nullptr;
    Geometry g;
    int rc = validate(desc, &g);
    if (rc != ESCOIN_OK) return rc;
    escoin_plan *p = new (std::nothrow) escoin_plan();
    if (!p) return fail(ESCOIN_ENOMEM, "out of host memory");
    p->g = g;
    p->user_desc = *desc;
    p->rowptr.assign(g.d.group, std::vector<int>(g.Mg + 1, 0));
    p->colidx.assign(g.d.group, std::vector<int>());
    p->values.assign(g.d.group, std::vector<float>());
    p->values64.assign(g.d.group, std::vector<double>());
    *plan = p;
    return ESCOIN_OK;
  });
}

int escoin_plan_destroy(escoin_plan *plan) {
  delete plan;
  return ESCOIN_OK;
}

int escoin_plan_set_option(escoin_plan *p, const char *key, int value) {
  return guarded([&]() -> int {
    if (!p || !key) return fail(ESCOIN_EINVAL, "null argument");
    // ("wgrad_kernel" and "wgrad_pointwise" on an aligned plan: read when the next backward state is built -- after a refused forced kernel, or
    //  after the next align; a state that exists keeps its kernel)
    if (!strcmp(key, "s2d")) {
      if (value < 0 || value > 1) return fail(ESCOIN_EINVAL, "s2d must be 0 or 1");
      if (p->aligned || p->host_aligned) return fail(ESCOIN_ESTATE, "s2d must be set before weight_align / weight_align_cpu / set_csr");
      p->s2d = value;
      return ESCOIN_OK;
    }
    if (!strcmp(key, "s2b")) {
      if (value < 0 || value > 1) return fail(ESCOIN_EINVAL, "s2b must be 0 or 1");
      if (p->aligned || p->host_aligned) return fail(ESCOIN_ESTATE, "s2b must be set before weight_align / weight_align_cpu / set_csr");
      p->s2b = value;
      return ESCOIN_OK;
    }
    if (!strcmp(key, "b2s")) {
      if (value < 0 || value > 1) return fail(ESCOIN_EINVAL, "b2s must be 0 or 1");
      if (p->aligned || p->host_aligned) return fail(ESCOIN_ESTATE, "b2s must be set before weight_align / weight_align_cpu / set_csr");
      p->b2s = value;
      return ESCOIN_OK;
    }
    if (!strcmp(key, "deconv")) {
      if (value < 0 || value > 1) return fail(ESCOIN_EINVAL, "deconv must be 0 or 1");
      if (p->aligned || p->host_aligned) return fail(ESCOIN_ESTATE, "deconv must be set before weight_align / weight_align_cpu / set_csr");
      // With the option set the plan's geometry is the mirror convolution's (M <-> C, H x W <-> OH x OW), whose weight matrix
      // is this layer's C x Mg*KH*KW one.  A layer the rule refuses keeps the descriptor's geometry: every align refuses it.
      D2sPlan dp;
      const escoin_conv_desc &want = value && d2s_plan(p->user_desc, false, &dp) ? dp.mirror : p->user_desc;
      Geometry g;
      if (const int rc = validate(&want, &g)) return rc;
      p->deconv = value;
      p->g = g;
      p->rowptr.assign(g.d.group, std::vector<int>(g.Mg + 1, 0));
      return ESCOIN_OK;
    }
    if (!strcmp(key, "b2s_block")) {
      if (value != 0 && (value < kB2sMinBlock || value > kB2sMaxBlock || value % 4 != 0))
        return fail(ESCOIN_EINVAL, "b2s_block must be 0 (the rule) or a multiple of 4 in 4..256");
      if (p->aligned || p->host_aligned) return fail(ESCOIN_ESTATE, "b2s_block must be set before weight_align / weight_align_cpu / set_csr");
      p->b2s_block = value;
      return ESCOIN_OK;
    }
    if (p->aligned && strcmp(key, "conv_mode") != 0 && strcmp(key, "cpu_channel_block") != 0 && strcmp(key, "cpu_images_per_job") != 0 &&
        strcmp(key, "wgrad_kernel") != 0 && strcmp(key, "wgrad_pointwise") != 0)
      return fail(ESCOIN_ESTATE, "this option must be set before weight_align/set_csr");
    if (!strcmp(key, "tiling_batch")) {
      if (value < 0) return fail(ESCOIN_EINVAL, "tiling_batch must be >= 0");
      p->tiling_batch = value;
      return ESCOIN_OK;
    }
    if (!strcmp(key, "max_launch_bytes")) {
      if (value < 0) return fail(ESCOIN_EINVAL, "max_launch_bytes must be >= 0");
      p->max_launch_bytes = value;
      return ESCOIN_OK;
    }
    if (!strcmp(key, "dense_threshold_pct")) {
      if (value < -1 || value > 100) return fail(ESCOIN_EINVAL, "dense_threshold_pct must be in [-1, 100]");
      p->dense_threshold_pct = value;
      return ESCOIN_OK;
    }
    if (!strcmp(key, "cpu_images_per_job")) {
      if (value < 0) return fail(ESCOIN_EINVAL, "cpu_images_per_job must be >= 0");
      p->cpu_img_force = value;
      return ESCOIN_OK;
    }
    if (!strcmp(key, "cpu_channel_block")) {
      if (value < 0) return fail(ESCOIN_EINVAL, "cpu_channel_block must be >= 0");
      p->cpu_blk_force = value;
      p->cpu_blk_cb = -1;
      return ESCOIN_OK;
    }
    if (!strcmp(key, "code_loader")) {
      if (value < 0 || value > 1) return fail(ESCOIN_EINVAL, "code_loader must be 0 or 1");
      p->code_loader = value;
      return ESCOIN_OK;
    }
    if (!strcmp(key, "backward_kernel")) {
      if (value < ESCOIN_KERNEL_AUTO || value > ESCOIN_BWD_MFMA) return fail(ESCOIN_EINVAL, "backward_kernel must be a kernel id (0..4) or 5 (the MFMA data-gradient kernel)");
      p->bwd_kernel = value;
      return ESCOIN_OK;
    }
    if (!strcmp(key, "wgrad_kernel")) {
      if (value < ESCOIN_WGRAD_AUTO || value > ESCOIN_WGRAD_MFMA) return fail(ESCOIN_EINVAL, "wgrad_kernel must be 0 (auto), 1 (entry), 2 (staged) or 3 (mfma)");
      p->wgrad_kernel = value;
      // (options "b2s" and "deconv": the weight gradient is the inner plan's, which reads the option as this plan would)
      if (p->b2s_state) return escoin_plan_set_option(p->b2s_state->inner.plan.get(), key, value);
      if (p->d2s_state) return escoin_plan_set_option(p->d2s_state->inner.plan.get(), key, value);
      return ESCOIN_OK;
    }
    if (!strcmp(key, "wgrad_pointwise")) {
      if (value < 0 || value > 1) return fail(ESCOIN_EINVAL, "wgrad_pointwise must be 0 or 1");
      p->wgrad_pointwise = value;
      // (options "b2s" and "deconv": handed on as "wgrad_kernel" is)
      if (p->b2s_state) return escoin_plan_set_option(p->b2s_state->inner.plan.get(), key, value);
      if (p->d2s_state) return escoin_plan_set_option(p->d2s_state->inner.plan.get(), key, value);
      return ESCOIN_OK;
    }
    if (!strcmp(key, "wgrad_pointwise_tile_entries")) {
      if (value < 0) return fail(ESCOIN_EINVAL, "wgrad_pointwise_tile_entries must be >= 0");
      p->wgrad_pw_tile_entries = value;
      return ESCOIN_OK;
    }
    if (!strcmp(key, "wgrad_channel_block")) {
      if (value < 0) return fail(ESCOIN_EINVAL, "wgrad_channel_block must be >= 0");
      p->wgrad_channel_block = value;
      return ESCOIN_OK;
    }
    if (!strcmp(key, "dense_wgrad_splits")) {
      if (value < 0) return fail(ESCOIN_EINVAL, "dense_wgrad_splits must be >= 0");
      p->dense_wgrad_splits = value;
      return ESCOIN_OK;
    }
    if (!strcmp(key, "body_variant")) {
      if (value < -1 || value > 0) return fail(ESCOIN_EINVAL, "body_variant must be -1 (automatic) or 0 (generic)");
      p->body_variant = value;
      return ESCOIN_OK;
    }
    if (!strcmp(key, "code_touchers")) {
      if (value < 0) return fail(ESCOIN_EINVAL, "code_touchers must be 0 (the rule) or a stride >= 1");
      p->code_touchers = value;
      return ESCOIN_OK;
    }
    if (!strcmp(key, "stream_stores")) {
      if (value < -1 || value > 1) return fail(ESCOIN_EINVAL, "stream_stores must be -1, 0 or 1");
      p->stream_stores = value;
      return ESCOIN_OK;
    }
    if (!strcmp(key, "kernel")) {
      if (value < ESCOIN_KERNEL_AUTO || value > ESCOIN_KERNEL_JIT)
        return fail(ESCOIN_EINVAL, "unknown kernel id");
      p->kernel_choice = value;
    } else if (!strcmp(key, "conv_mode")) {
      if (value < ESCOIN_CONV_MODE_LOWERED_GEMM || value > ESCOIN_CONV_MODE_SCONV_PAR)
        return fail(ESCOIN_EINVAL, "conv_mode must be one of Caffe::ConvMode's four values (0..3)");
      // (an "s2d" / "s2b" plan also rebuilds between the lowered modes, which run on the original geometry, and SCONV / SCONV_PAR)
      auto direct = [](int m) { return m == ESCOIN_CONV_MODE_SCONV || m == ESCOIN_CONV_MODE_SCONV_PAR; };
      const bool regroup = p->aligned && ((value == ESCOIN_CONV_MODE_LOWERED_GEMM) != (p->conv_mode == ESCOIN_CONV_MODE_LOWERED_GEMM) ||
                                          ((p->s2d || p->s2b || p->b2s) && !p->is_f64 && direct(value) != direct(p->conv_mode)));
      // (option "deconv": the mode is the inner plan's, which rebuilds itself where it has to)
      if (p->aligned && p->d2s_state) {
        if (const int rcs = sync_host_values(p)) return rcs;
        const int rci = escoin_plan_set_option(p->d2s_state->inner.plan.get(), key, value);
        if (rci != ESCOIN_OK) return rci;
        p->conv_mode = value;
        p->upd.reset();      // (the inner plan may have rebuilt its copies)
        p->kernel_name = std::string(escoin_plan_kernel_name(p->d2s_state->inner.plan.get())) + " + " + g_d2s_hooks.unpack_kernel_name;
        return ESCOIN_OK;
      }
      p->conv_mode = value;
      // to or from LOWERED_GEMM on an aligned plan: the dense / sparse device structures are rebuilt
      // from the CSR the plan holds (the other three modes share theirs).  The plan is not aligned
      // while that happens: if an allocation fails, the next forward reports ESCOIN_ESTATE instead of
      // launching on freed pointers.  The rebuild must happen on the device the plan lives on.
      if (regroup) {
        int dev = -1;
        if (hipGetDevice(&dev) != hipSuccess || dev != p->device)
          return fail(ESCOIN_ESTATE, "conv_mode flip on an aligned plan: the current device is not the plan's device");
        // (after device-source updates the host CSR the rebuild reads is stale: the values come back first)
        if (const int rcs = sync_host_values(p)) return rcs;
        p->aligned = false;
        return upload(p, nullptr);
      }
    } else if (!strcmp(key, "dense_gate")) {
      p->dense_gate = value != 0;
    } else {
      return fail(ESCOIN_EINVAL, std::string("unknown option: ") + key);
    }
    return ESCOIN_OK;
  });
}

int escoin_weight_align(escoin_plan *p, const float *dense_w, int w_on_device, void *stream) {
  return guarded([&]() -> int { return weight_align_t<float>(p, dense_w, w_on_device, stream); });
}

int escoin_weight_align_f64(escoin_plan *p, const double *dense_w, int w_on_device, void *stream) {
  return guarded([&]() -> int { return weight_align_t<double>(p, dense_w, w_on_device, stream); });
}

int escoin_plan_set_csr(escoin_plan *p, const int *rowptr, const int *colidx, const float *values,
                        const int *nnz_per_group, void *stream) {
  return guarded([&]() -> int { return set_csr_t<float>(p, rowptr, colidx, values, nnz_per_group, stream); });
}

int escoin_plan_set_csr_f64(escoin_plan *p, const int *rowptr, const int *colidx, const double *values,
                            const int *nnz_per_group, void *stream) {
  return guarded([&]() -> int { return set_csr_t<double>(p, rowptr, colidx, values, nnz_per_group, stream); });
}

}  // extern "C"

namespace escoin {
// Validates a CSR and copies it into the plan's host vectors (shared by set_csr and import_aligned); fixes the plan's
// Dtype like a WeightAlign does.
template <typename T>
int set_csr_host(escoin_plan *p, const int *rowptr, const int *colidx, const T *values, const int *nnz_per_group) {
  if (!p || !rowptr || !nnz_per_group) return fail(ESCOIN_EINVAL, "null argument");
  const Geometry &g = p->g;
  long base = 0;
  for (int grp = 0; grp < g.d.group; ++grp) {
    const int n_g = nnz_per_group[grp];
    const int *rp = rowptr + (size_t)grp * (g.Mg + 1);
    if (n_g < 0 || rp[0] != 0 || rp[g.Mg] != n_g)
      return fail(ESCOIN_EINVAL, "set_csr: rowptr does not match nnz_per_group");
    if (n_g > 0 && (!colidx || !values)) return fail(ESCOIN_EINVAL, "set_csr: null colidx/values");
    for (int m = 0; m < g.Mg; ++m)
      if (rp[m + 1] < rp[m]) return fail(ESCOIN_EINVAL, "set_csr: rowptr not monotone");
    for (int j = 0; j < n_g; ++j)
      if (colidx[base + j] < 0 || colidx[base + j] >= g.kdim)
        return fail(ESCOIN_EINVAL, "set_csr: column index out of range");
    // caffe_cpu_sparse_dense2csr scans a row left to right (math_functions.cpp:92-105): columns are
    // strictly ascending within a row.  The stream builder's row grouping and the reference-order
    // kernels (bit-exact summation order) rely on it, so anything else is refused, not repaired.
    for (int m = 0; m < g.Mg; ++m)
      for (int j = rp[m] + 1; j < rp[m + 1]; ++j)
        if (colidx[base + j] <= colidx[base + j - 1])
          return fail(ESCOIN_EINVAL, "set_csr: column indices must be strictly ascending within a row");
    base += n_g;
  }
  // (validated as a whole first: a refused CSR leaves the plan as it was)
  p->aligned = false;
  p->host_aligned = false;
  p->is_f64 = sizeof(T) == 8;
  std::vector<std::vector<T>> &vals = plan_vals<T>(p);
  base = 0;
  for (int grp = 0; grp < g.d.group; ++grp) {
    const int n_g = nnz_per_group[grp];
    const int *rp = rowptr + (size_t)grp * (g.Mg + 1);
    p->rowptr[grp].assign(rp, rp + g.Mg + 1);
    p->colidx[grp].assign(colidx + base, colidx + base + n_g);
    p->values[grp].clear();
    p->values64[grp].clear();
    vals[grp].assign(values + base, values + base + n_g);
    base += n_g;
  }
  p->cpu_off_valid = false;
  p->cpu_inner.plan.reset();
  p->host_aligned = true;
  return ESCOIN_OK;
}
template int set_csr_host<float>(escoin_plan *, const int *, const int *, const float *, const int *);
template int set_csr_host<double>(escoin_plan *, const int *, const int *, const double *, const int *);
}  // namespace escoin

extern "C" {

// ---- the persisted aligned form (its byte layout, writer and parser: aligned_form.h) --------------------------------

int escoin_plan_export_aligned(const escoin_plan *p, void *buf, size_t capacity, size_t *bytes) {
  return guarded([&]() -> int {
    if (!p || !bytes) return fail(ESCOIN_EINVAL, "null argument");
    if (!p->aligned) return fail(ESCOIN_ESTATE, "export_aligned before weight_align / set_csr");
    if (p->is_f64) return fail(ESCOIN_ESTATE, "export_aligned: the aligned form is defined for float plans (a double plan has no generated code to persist; hand its CSR over with escoin_plan_get_csr_f64 / set_csr_f64)");
    if (const int rcs = sync_host_values(const_cast<escoin_plan *>(p))) return rcs;
    std::vector<char> jit;
    const int rc = tiled_export(p, &jit);
    if (rc != ESCOIN_OK) return rc;
    const size_t need = aligned_bytes(p->g, (uint64_t)plan_nnz(p), jit.size());
    *bytes = need;
    if (!buf) return ESCOIN_OK;                       // size query
    if (capacity < need) return fail(ESCOIN_EINVAL, "export_aligned: buffer too small");
    aligned_write(p->g, p->rowptr, p->colidx, p->values, jit, buf);
    return ESCOIN_OK;
  });
}

int escoin_plan_import_aligned(escoin_plan *p, const void *buf, size_t bytes, void *stream) {
  return guarded([&]() -> int {
    if (!p || !buf) return fail(ESCOIN_EINVAL, "null argument");
    if (const int rc = deconv_precheck(p, false)) return rc;
    const auto t_start = std::chrono::steady_clock::now();
    const AlignedForm f = aligned_parse(buf, bytes, p->g);
    if (f.rc != ESCOIN_OK) return fail(f.rc, f.error);
    const double ms_parse = ms_since(t_start);
    const int rc = set_csr_host<float>(p, f.rowptr.data(), f.colidx.data(), f.values.data(), f.nnz_per_group.data());
    if (rc != ESCOIN_OK) return rc;
    p->aligned = false;
    const double ms_csr = ms_since(t_start);
    const bool code = f.same_geom && f.code_section_bytes > 0;
    const int rc2 = upload(p, (hipStream_t)stream, code ? f.code_section : nullptr, f.same_geom ? f.code_section_bytes : 0);
    p->align_ms = ms_since(t_start);
    if (getenv("ESCOIN_VERBOSE"))
      fprintf(stderr, "[escoin] import_aligned: %zu bytes (code %zu): tags + parse %.2f ms, CSR checks %.2f ms, upload + code load %.2f ms\n",
              bytes, f.code_section_bytes, ms_parse, ms_csr - ms_parse, p->align_ms - ms_csr);
    return rc2;
  });
}

// The same from a DEVICE buffer (where an RCCL broadcast leaves the blob): one copy into a host staging area that the
// calling thread keeps between calls (grow-only; pageable -- pinning 13 MB costs more than the copy saves), then the
// host import: the CSR and the code object are parsed and loaded from host memory either way (hipModuleLoadData takes a
// host image).
namespace {
thread_local std::vector<char> g_stage;
}  // namespace

int escoin_plan_import_aligned_dev(escoin_plan *p, const void *dev_buf, size_t bytes, void *stream) {
  return guarded([&]() -> int {
    if (!p || !dev_buf) return fail(ESCOIN_EINVAL, "null argument");
    if (bytes < sizeof(AlignedHdr) || bytes > (size_t)1 << 36) return fail(ESCOIN_EINVAL, "import_aligned: implausible blob size");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(ESCOIN_ENODEVICE, "no HIP device");
    if (g_stage.size() < bytes) g_stage.resize(bytes + (bytes >> 2));     // (grows by a quarter: layers come in rising sizes)
    ESCOIN_HIP_TRY(hipMemcpyAsync(g_stage.data(), dev_buf, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    ESCOIN_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return escoin_plan_import_aligned(p, g_stage.data(), bytes, stream);
  });
}

long escoin_plan_stat(const escoin_plan *p, const char *key) {
  if (!p || !key) return fail(ESCOIN_EINVAL, "null argument");
  if (!strcmp(key, "s2d")) return p->s2d_state ? 1 : 0;
  if (!strcmp(key, "s2d_scratch_bytes")) return p->s2d_state ? (long)p->s2d_state->x.bytes() : 0;
  if (!strcmp(key, "s2b")) return p->s2b_state ? 1 : 0;
  if (!strcmp(key, "s2b_scratch_bytes")) return p->s2b_state ? (long)(p->s2b_state->x.bytes() + p->s2b_state->t.bytes()) : 0;
  if (!strcmp(key, "deconv")) return p->d2s_state ? 1 : 0;
  if (!strcmp(key, "deconv_scratch_bytes")) return p->d2s_state ? (long)p->d2s_state->t.bytes() : 0;
  if (!strcmp(key, "b2s")) return p->b2s_state ? 1 : 0;
  if (!strcmp(key, "b2s_block")) return p->b2s_state ? p->b2s_state->bp.B : 0;
  if (!strcmp(key, "b2s_scratch_bytes"))
    return p->b2s_state ? (long)(p->b2s_state->x.bytes() + p->b2s_state->t.bytes() + p->b2s_state->dx.bytes()) : 0;
  if (p->inner_plan()) {
    // what describes the forward's kernel is the inner plan's
    static const char *const inner_keys[] = {"kernel_choice", "code_bytes", "code_direct", "small_launch_rule", "jit_rows", "jit_records",
                                             "deal_slowest_over_mean_x1000", "deal_worst_block_x1000", "lds_bytes", "body_variant",
                                             "code_touchers", "touch_lines_per_launch",
                                             "workgroup_columns", "streamk_gave_up", "streamk", "dense_variant"};
    for (const char *k : inner_keys)
      if (!strcmp(key, k)) return escoin_plan_stat(p->inner_plan()->plan.get(), key);
  }
  if (!strcmp(key, "align_us")) return (long)(p->align_ms * 1e3);
  if (!strcmp(key, "code_bytes")) return (long)(p->tiled.enabled && p->tiled.jit ? p->tiled_dev.jit.code_bytes : 0);
  if (!strcmp(key, "device_bytes")) return (long)device_bytes(p).fwd;
  if (!strcmp(key, "import_fast")) return p->import_fast ? 1 : 0;
  if (!strcmp(key, "cpu_images_per_job")) return p->cpu_img_last;   // images per job of the last escoin_forward_cpu
  if (!strcmp(key, "cpu_channel_block")) return p->cpu_blk_cb;     // channels per block of the last escoin_forward_cpu (0: unblocked, -1: none yet)
  if (!strcmp(key, "code_direct")) return p->tiled_dev.jit.direct ? 1 : 0;     // the plan's code sits in executable memory the library filled itself
  if (!strcmp(key, "small_launch_rule")) return p->small_rule;
  if (!strcmp(key, "jit_rows")) return p->tiled.jit ? p->tiled.jit_rows : 0;
  if (!strcmp(key, "jit_records")) return p->tiled.jit ? p->tiled.jit_records : 0;
  // balance of the channel deal, x 1000 (1000 = every wave of every block costs the same; generated-code plans
  // built from weights -- 0 for an imported code object, which does not carry the figure)
  if (!strcmp(key, "deal_slowest_over_mean_x1000")) return p->tiled.jit ? (long)(p->tiled.deal_slowest_over_mean * 1000.f + 0.5f) : 0;
  if (!strcmp(key, "deal_worst_block_x1000")) return p->tiled.jit ? (long)(p->tiled.deal_worst_block * 1000.f + 0.5f) : 0;
  if (!strcmp(key, "lds_bytes")) return p->tiled.enabled ? (long)p->tiled.lds_bytes : 0;
  if (!strcmp(key, "body_variant")) return p->tiled.enabled ? p->tiled.body_variant_last : 0;
  if (!strcmp(key, "code_touchers")) return p->tiled.enabled ? p->tiled.touch_stride_last : 1;
  if (!strcmp(key, "touch_lines_per_launch"))     // (counted on the host from the last launch's shape and stride)
    return p->tiled.enabled && p->tiled.jit ? touch_lines(p->tiled.launch_shape_last, p->tiled.tiling, p->tiled.jit_pref, p->tiled.touch_stride_last) : 0;
  if (!strcmp(key, "workgroup_columns")) return p->tiled.enabled ? p->tiled.tiling.n_ocblk : 0;
  if (!strcmp(key, "streamk_gave_up")) {
    // dense kernel, stream-K launches: 1 if a workgroup's bounded wait for another one's partial sums ran out in
    // the last launch (its results are then wrong); synchronises with the device.  0 for plans that never split K.
    const DenseArrays &dn = p->dense;
    if (!dn.sk_ws.get<void>() || dn.sk_flag_words < 1 || !dn.sk_used) return 0;
    if (dn.sk_fail.host() && *(volatile unsigned *)dn.sk_fail.host() != 0u) return 1;      // (sticky: any launch since WeightAlign)
    unsigned v = 0;
    if (hipMemcpy(&v, dn.sk_ws.get<const unsigned>() + (dn.sk_flag_words - 1), 4, hipMemcpyDeviceToHost) != hipSuccess)
      return fail(ESCOIN_EHIP, "streamk_gave_up: device read failed");
    return (long)v;
  }
  if (!strcmp(key, "streamk")) return p->dense.sk_used ? 1 : 0;
  if (!strcmp(key, "dense_variant")) return p->dense.variant_last;
  if (!strncmp(key, "bwd_", 4) || !strncmp(key, "wgrad_", 6) || !strncmp(key, "dgrad_", 6)) return bwd_stat(p, key);
  if (!strncmp(key, "upd", 3)) return upd_stat(p, key);
  if (!strncmp(key, "dwg_", 4)) return dwg_stat(p, key);
  if (!strcmp(key, "prune_count")) return p->prune_count;
  if (!strcmp(key, "prune_last_dropped")) return p->prune_last_dropped;
  if (!strcmp(key, "prune_tile_entries")) return prune::kTileEntries;
  if (!strcmp(key, "prune_kernels_us")) return (long)(p->prune_kernels_ms * 1e3);
  if (!strcmp(key, "prune_map_us")) return (long)(p->prune_map_ms * 1e3);
  if (!strcmp(key, "prune_realign_us")) return (long)(p->prune_realign_ms * 1e3);
  if (!strcmp(key, "rewire_count")) return p->rewire_count;
  if (!strcmp(key, "rewire_last_dropped")) return p->rewire_last_dropped;
  if (!strcmp(key, "rewire_last_grown")) return p->rewire_last_grown;
  if (!strcmp(key, "rewire_kernels_us")) return (long)(p->rewire_kernels_ms * 1e3);
  if (!strcmp(key, "rewire_map_us")) return (long)(p->rewire_map_ms * 1e3);
  if (!strcmp(key, "rewire_realign_us")) return (long)(p->rewire_realign_ms * 1e3);
  if (!strcmp(key, "is_f64")) return p->is_f64 ? 1 : 0;
  if (!strcmp(key, "host_aligned")) return p->host_aligned ? 1 : 0;
  if (!strcmp(key, "kernel_choice")) {
    if (!p->aligned) return fail(ESCOIN_ESTATE, "kernel_choice before weight_align / set_csr");
    if (p->is_f64) return ESCOIN_KERNEL_GENERIC;
    if (p->use_dense) return ESCOIN_KERNEL_DENSE;
    if (!p->tiled.enabled) return ESCOIN_KERNEL_GENERIC;
    return p->tiled.jit ? ESCOIN_KERNEL_JIT : ESCOIN_KERNEL_TILED;
  }
  return fail(ESCOIN_EINVAL, std::string("unknown stat: ") + key);
}

long escoin_plan_nnz(const escoin_plan *p, int group) {
  if (!p) return fail(ESCOIN_EINVAL, "null plan");
  if (group >= p->g.d.group) return fail(ESCOIN_EINVAL, "group out of range");
  if (group >= 0) return (long)p->colidx[group].size();
  return plan_nnz(p);
}

int escoin_plan_get_csr(const escoin_plan *p, int *rowptr, int *colidx, float *values, int stretched) {
  return guarded([&]() -> int { return get_csr_t<float>(p, rowptr, colidx, values, stretched); });
}

int escoin_plan_get_csr_f64(const escoin_plan *p, int *rowptr, int *colidx, double *values, int stretched) {
  return guarded([&]() -> int { return get_csr_t<double>(p, rowptr, colidx, values, stretched); });
}

size_t escoin_plan_workspace_bytes(const escoin_plan *p) {
  if (!p) return 0;
  const DeviceBytes b = device_bytes(p);
  return b.fwd + b.bwd + b.upd + b.dwg;
}

const char *escoin_plan_kernel_name(const escoin_plan *p) {
  if (p && p->aligned && p->d2s_state) return p->kernel_name.c_str();      // (option "deconv": the inner plan's name, whatever the mode, + the unpack kernel)
  if (p && p->aligned && !p->is_f64 && p->conv_mode == ESCOIN_CONV_MODE_LOWERED_SPARSE &&
      p->kernel_choice != ESCOIN_KERNEL_DENSE)
    return lowered_kernel_name();
  return p ? p->kernel_name.c_str() : "";
}

const char *escoin_plan_tiling_info(const escoin_plan *p) {
  if (p && p->aligned && p->inner_plan()) return escoin_plan_tiling_info(p->inner_plan()->plan.get());
  return (p && p->aligned && p->tiled.enabled) ? p->tiled.info.c_str() : "";
}

int escoin_plan_s2d_pack(escoin_plan *p, const float *bottom_dev, int n_images, void *stream) {
  return guarded([&]() -> int {
    if (!p || !bottom_dev) return fail(ESCOIN_EINVAL, "null argument");
    if (!p->aligned || !p->s2d_state) return fail(ESCOIN_ESTATE, "s2d_pack: option \"s2d\" is not active on this plan");
    if (const int rc = check_n_images(p, n_images)) return rc;
    if (n_images == 0) return ESCOIN_OK;
    if (const int rc = check_plan_device(p, "s2d_pack")) return rc;
    return g_s2d_hooks.pack(p, bottom_dev, p->s2d_state->x.get<float>(), n_images, (hipStream_t)stream);
  });
}

int escoin_plan_s2b_pack(escoin_plan *p, const float *bottom_dev, int n_images, void *stream) {
  return guarded([&]() -> int {
    if (!p || !bottom_dev) return fail(ESCOIN_EINVAL, "null argument");
    if (!p->aligned || !p->s2b_state) return fail(ESCOIN_ESTATE, "s2b_pack: option \"s2b\" is not active on this plan");
    if (const int rc = check_n_images(p, n_images)) return rc;
    if (n_images == 0) return ESCOIN_OK;
    if (const int rc = check_plan_device(p, "s2b_pack")) return rc;
    return g_s2b_hooks.pack(p, bottom_dev, nullptr, p->s2b_state->x.get<float>(), false, n_images, (hipStream_t)stream);
  });
}

int escoin_plan_s2b_unpack(escoin_plan *p, float *top_dev, int n_images, void *stream) {
  return guarded([&]() -> int {
    if (!p || !top_dev) return fail(ESCOIN_EINVAL, "null argument");
    if (!p->aligned || !p->s2b_state) return fail(ESCOIN_ESTATE, "s2b_unpack: option \"s2b\" is not active on this plan");
    if (const int rc = check_n_images(p, n_images)) return rc;
    if (n_images == 0) return ESCOIN_OK;
    if (const int rc = check_plan_device(p, "s2b_unpack")) return rc;
    return g_s2b_hooks.unpack(p, p->s2b_state->t.get<const float>(), top_dev, true, p->g.d.fuse_relu != 0, n_images, (hipStream_t)stream);
  });
}

int escoin_plan_d2s_unpack(escoin_plan *p, const float *t_dev, const float *bias_dev, float *top_dev, int n_images, void *stream) {
  return guarded([&]() -> int {
    if (!p || !top_dev) return fail(ESCOIN_EINVAL, "null argument");
    if (!p->aligned || !p->d2s_state) return fail(ESCOIN_ESTATE, "d2s_unpack: option \"deconv\" is not active on this plan");
    if (const int rc = check_n_images(p, n_images)) return rc;
    if (n_images == 0) return ESCOIN_OK;
    if (const int rc = check_plan_device(p, "d2s_unpack")) return rc;
    return g_d2s_hooks.unpack(p, t_dev ? t_dev : p->d2s_state->t.get<const float>(), bias_dev, top_dev, p->g.d.fuse_relu != 0, n_images,
                              (hipStream_t)stream);
  });
}

int escoin_plan_d2s_pack(escoin_plan *p, const float *top_diff_dev, const float *top_dev, float *g_dev, int n_images, void *stream) {
  return guarded([&]() -> int {
    if (!p || !top_diff_dev) return fail(ESCOIN_EINVAL, "null argument");
    if (!p->aligned || !p->d2s_state) return fail(ESCOIN_ESTATE, "d2s_pack: option \"deconv\" is not active on this plan");
    if (p->g.d.fuse_relu && !top_dev) return fail(ESCOIN_EINVAL, "d2s_pack: a fuse_relu plan needs the forward's top");
    if (const int rc = check_n_images(p, n_images)) return rc;
    if (n_images == 0) return ESCOIN_OK;
    if (const int rc = check_plan_device(p, "d2s_pack")) return rc;
    return g_d2s_hooks.pack(p, top_diff_dev, p->g.d.fuse_relu ? top_dev : nullptr, g_dev ? g_dev : p->d2s_state->t.get<float>(), n_images,
                            (hipStream_t)stream);
  });
}

int escoin_plan_b2s_pack(escoin_plan *p, const float *src_dev, const float *mask_dev, float *dst_dev, int top_side, int n_images,
                         void *stream) {
  return guarded([&]() -> int {
    if (!p) return fail(ESCOIN_EINVAL, "null argument");
    if (!p->aligned || !p->b2s_state) return fail(ESCOIN_ESTATE, "b2s_pack: option \"b2s\" is not active on this plan");
    if (!src_dev || !dst_dev) return fail(ESCOIN_EINVAL, "null argument");
    if (const int rc = check_n_images(p, n_images)) return rc;
    if (n_images == 0) return ESCOIN_OK;
    if (const int rc = check_plan_device(p, "b2s_pack")) return rc;
    return g_b2s_hooks.pack(p, src_dev, mask_dev, dst_dev, top_side != 0, n_images, (hipStream_t)stream);
  });
}

int escoin_plan_b2s_unpack(escoin_plan *p, const float *src_dev, float *dst_dev, int top_side, int relu, int n_images, void *stream) {
  return guarded([&]() -> int {
    if (!p) return fail(ESCOIN_EINVAL, "null argument");
    if (!p->aligned || !p->b2s_state) return fail(ESCOIN_ESTATE, "b2s_unpack: option \"b2s\" is not active on this plan");
    if (!src_dev || !dst_dev) return fail(ESCOIN_EINVAL, "null argument");
    if (const int rc = check_n_images(p, n_images)) return rc;
    if (n_images == 0) return ESCOIN_OK;
    if (const int rc = check_plan_device(p, "b2s_unpack")) return rc;
    return g_b2s_hooks.unpack(p, src_dev, dst_dev, top_side != 0, relu != 0, n_images, (hipStream_t)stream);
  });
}

int escoin_forward(escoin_plan *p, const float *bottom_dev, const float *bias_dev, float *top_dev,
                   int n_images, void *stream) {
  return guarded([&]() -> int {
    if (!p || !bottom_dev || !top_dev) return fail(ESCOIN_EINVAL, "null argument");
    if (!p->aligned) return fail(ESCOIN_ESTATE, "forward called before weight_align / set_csr");
    if (p->is_f64) return fail(ESCOIN_ESTATE, "forward: the plan holds double weights (use escoin_forward_f64)");
    if (const int rc = check_n_images(p, n_images)) return rc;
    if (n_images == 0) return ESCOIN_OK;
    if (const int rc = check_plan_device(p, "forward")) return rc;
    // dense kernel, stream-K: a fix-up wait that ran out in an EARLIER launch of this plan left wrong results in that
    // launch's top blob.  The word lives in pinned host memory (no synchronisation here) and stays set until the
    // next WeightAlign: the caller hears about it at the next call at the latest (dense_mfma.hip).
    if (p->dense.sk_fail.host() && *(volatile unsigned *)p->dense.sk_fail.host() != 0u)
      return fail(ESCOIN_EHIP, "dense kernel (stream-K): a workgroup gave up waiting for another one's partial sums in an "
                               "earlier launch of this plan; that launch's results are wrong");
    hipStream_t s = (hipStream_t)stream;
    // option "s2d": the bottom's stride phases become channels of X', then the inner stride-1 plan (bias and ReLU in its epilogue)
    if (S2dState *sd = p->s2d_state.get()) {
      const int rc = g_s2d_hooks.pack(p, bottom_dev, sd->x.get<float>(), n_images, s);
      if (rc != ESCOIN_OK) return rc;
      return escoin_forward(sd->inner.plan.get(), sd->x.get<const float>(), bias_dev, top_dev, n_images, stream);
    }
    // option "s2b": the padded bottom's residue classes become images of X', then the inner undilated plan (bias in its
    // epilogue) into T', then the classes' tops interleaved into the top blob (ReLU there)
    if (S2bState *sb = p->s2b_state.get()) {
      const int P = sb->sp.eh * sb->sp.ew;
      int rc = g_s2b_hooks.pack(p, bottom_dev, nullptr, sb->x.get<float>(), false, n_images, s);
      if (rc != ESCOIN_OK) return rc;
      rc = escoin_forward(sb->inner.plan.get(), sb->x.get<const float>(), bias_dev, sb->t.get<float>(), n_images * P, stream);
      if (rc != ESCOIN_OK) return rc;
      return g_s2b_hooks.unpack(p, sb->t.get<const float>(), top_dev, true, p->g.d.fuse_relu != 0, n_images, s);
    }
    // option "b2s": the bottom transposed into X' (the batch becomes the pixel axis), then the inner pointwise plan (bias in
    // its epilogue) into T', then T' transposed into the top blob (ReLU there)
    if (B2sState *bs = p->b2s_state.get()) {
      const int n_inner = (n_images + bs->bp.B - 1) / bs->bp.B;
      int rc = g_b2s_hooks.pack(p, bottom_dev, nullptr, bs->x.get<float>(), false, n_images, s);
      if (rc != ESCOIN_OK) return rc;
      rc = escoin_forward(bs->inner.plan.get(), bs->x.get<const float>(), bias_dev, bs->t.get<float>(), n_inner, stream);
      if (rc != ESCOIN_OK) return rc;
      return g_b2s_hooks.unpack(p, bs->t.get<const float>(), top_dev, true, p->g.d.fuse_relu != 0, n_images, s);
    }
    // option "deconv": the inner stride-1 plan on the caller's bottom itself into T' (no bias: it is not constant over a
    // phase's crop, and one more rounding in the unpack on the device and in CPU mode alike), then the interleave, the
    // crop, the bias and the ReLU in the unpack kernel
    if (D2sState *ds = p->d2s_state.get()) {
      const int rc = escoin_forward(ds->inner.plan.get(), bottom_dev, nullptr, ds->t.get<float>(), n_images, stream);
      if (rc != ESCOIN_OK) return rc;
      return g_d2s_hooks.unpack(p, ds->t.get<const float>(), bias_dev, top_dev, p->g.d.fuse_relu != 0, n_images, s);
    }
    // LOWERED_SPARSE lowers every group, whatever AUTO decided for the direct path
    if (p->conv_mode == ESCOIN_CONV_MODE_LOWERED_SPARSE && p->kernel_choice != ESCOIN_KERNEL_DENSE)
      return launch_lowered(p, bottom_dev, bias_dev, top_dev, n_images, s);
    if (p->n_dense_groups > 0) {
      // dense and sparse groups: what the sparse half's launch refuses for sizes is asked first, so that a refused call
      // has written nothing (the dense half's own refusals come before its launch anyway)
      if (!p->use_dense) {
        if (p->tiled.enabled) {
          if (const int rc = tiled_precheck(p, n_images)) return rc;
        } else if (const LaunchVerdict v = generic_call_limits(p->g, n_images); !v.ok()) {
          return fail(v.rc, v.error);
        }
      }
      const int rc = launch_dense(p, bottom_dev, bias_dev, top_dev, n_images, s);
      if (rc != ESCOIN_OK || p->use_dense) return rc;
    }
    if (p->tiled.enabled) return launch_tiled(p, bottom_dev, bias_dev, top_dev, n_images, s);
    return launch_generic(p, bottom_dev, bias_dev, top_dev, n_images, s);
  });
}

// Forward_gpu for Dtype = double (conv_layer.cu:75 instantiates the layer for both types): the order-preserving
// generic kernel in fp64, whatever the conv_mode.
int escoin_forward_f64(escoin_plan *p, const double *bottom_dev, const double *bias_dev, double *top_dev, int n_images,
                       void *stream) {
  return guarded([&]() -> int {
    if (!p || !bottom_dev || !top_dev) return fail(ESCOIN_EINVAL, "null argument");
    if (!p->aligned) return fail(ESCOIN_ESTATE, "forward called before weight_align / set_csr");
    if (!p->is_f64) return fail(ESCOIN_ESTATE, "forward_f64: the plan holds float weights (use escoin_forward)");
    if (const int rc = check_n_images(p, n_images)) return rc;
    if (n_images == 0) return ESCOIN_OK;
    if (const int rc = check_plan_device(p, "forward")) return rc;
    return launch_generic_f64(p, bottom_dev, bias_dev, top_dev, n_images, (hipStream_t)stream);
  });
}

int escoin_gpu_sparse_csrmm(int M, int N, int K, int nnz, float alpha, const float *values,
                            const int *rowptr, const int *colidx, const float *B, float beta, float *C,
                            void *stream) {
  if (M < 0 || N < 0 || K < 0 || nnz < 0) return fail(ESCOIN_EINVAL, "negative dimension");
  if (M == 0 || N == 0) return ESCOIN_OK;
  if (!rowptr || !C || (nnz > 0 && (!values || !colidx || !B))) return fail(ESCOIN_EINVAL, "null argument");
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return fail(ESCOIN_ENODEVICE, "no HIP device (this entry point is the GPU one)");
  return csrmm(M, N, K, alpha, values, rowptr, colidx, B, beta, C, (hipStream_t)stream);
}

int escoin_gpu_sparse_csrmm_f64(int M, int N, int K, int nnz, double alpha, const double *values, const int *rowptr,
                                const int *colidx, const double *B, double beta, double *C, void *stream) {
  if (M < 0 || N < 0 || K < 0 || nnz < 0) return fail(ESCOIN_EINVAL, "negative dimension");
  if (M == 0 || N == 0) return ESCOIN_OK;
  if (!rowptr || !C || (nnz > 0 && (!values || !colidx || !B))) return fail(ESCOIN_EINVAL, "null argument");
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return fail(ESCOIN_ENODEVICE, "no HIP device (this entry point is the GPU one)");
  return csrmm_f64(M, N, K, alpha, values, rowptr, colidx, B, beta, C, (hipStream_t)stream);
}

}  // extern "C"
