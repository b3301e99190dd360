// update_values.hip -- in-place weight updates: the second half of a training step (include/escoin.h, "Weight updates").
//
// Everything WeightAlign decides is a function of the sparsity PATTERN and the options; a value enters the device side
// as a full 32-bit (64-bit: double plans) word at a position the builders record (jit::Program::val_word,
// WeightStream::val_word; tests/cpp/value_map_check.cpp proves that nothing else depends on a value).  For an unchanged
// pattern a weight update is therefore a scatter of the nnz values into every device word that holds one.  One rule
// (for_each_copy) finds them: a plan, its backward state's copy and its derived plans, recursively.
//   a plan's forward side       gen.vals (the generic kernel's and the LOWERED_SPARSE comparator's values), dense.w (the MFMA
//                               kernel's padded matrix), the generated code / the weight stream of a tiled plan's sparse groups
//   its backward state's copy   by BwdState::data one of: the transposed plan (a derived plan), gather.tval through
//                               gather.tsrc, dgm.mat through dgm.pos -- or none (the inner plan's state holds it)
//   its derived plans           (escoin_plan.h DerivedPlan: the transposed plan, the inner plan of option "s2d" or "s2b") plans like
//                               any other, whose copies are reached through the maps on the way composed (compose_maps)
// The first update on an alignment builds that list (UpdState); later updates launch one kernel and nothing else.
// The list's device facts (buffers, their sizes, the bounds checks) are collected here; the indices derived from the CSR
// alone -- dense positions, the entry-major view -- come from the host-only builders of csr_tables.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "escoin_plan.h"

namespace escoin {

struct UpdArgs {
  void *base[kUpdMaxBuffers];
  const int *src;
  const unsigned *off;
  const unsigned char *buf;
  const int *wpos;
  long n_dst;
};

// One lane per destination, one plain vector store each.  The list is sorted by (buffer, CSR entry): the lanes of a wave
// read ascending addresses of the source (CSR order ascends in blobs_[0]) and, for gen.vals, write consecutive ones.
//
// Patched CODE becomes visible the way freshly filled code does (code_memory.hip, escoin_code_copy_kernel, and the
// comment at the generated-code kernel's first jump, sconv_tiled.hip): these are ordinary vector stores, which reach L2 /
// memory when this kernel ends; the scalar cache -- through which the walk reads its weight lines -- is invalidated at
// every dispatch; literals are fetched by the instruction cache, which wave 0 of every workgroup of the generated-code
// kernel drops before the first jump, so the next launch refetches them from L2.  No cache instruction is needed here.
template <typename T, bool FromDense>
__global__ void __launch_bounds__(256) escoin_update_values_kernel(UpdArgs a, const T *__restrict__ in) {
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= a.n_dst) return;
  const int e = a.src[k];
  const T v = FromDense ? in[a.wpos[e]] : in[e];
  static_cast<T *>(a.base[a.buf[k]])[a.off[k]] = v;
}

namespace {

struct Dst { unsigned char buf; int src; unsigned off; };

// The destinations of one plan's forward side (the plan itself or a derived plan at any level): entry e of q's
// CSR (groups concatenated) is a copy of entry src_of[e] of the updated plan's (nullptr: the identity).  Every offset is
// checked against the size of the buffer it indexes: a list that would write out of bounds is refused, never launched.
// (Out of line: inlined into the walk below, the per-entry loop came out 2 % slower on the first update of a 3x3 layer.)
template <typename T>
__attribute__((noinline)) int collect(const escoin_plan *q, const int *src_of, UpdState *u, std::vector<Dst> *out) {
  const Geometry &g = q->g;
  auto add_buffer = [&](void *ptr) -> int {
    if (u->n_buffers >= kUpdMaxBuffers) return -1;
    u->base[u->n_buffers] = ptr;
    return u->n_buffers++;
  };
  const long nnz = plan_nnz(q);
  if (nnz == 0) return ESCOIN_OK;
  const int b_gen = add_buffer(q->gen.vals.get<void>());
  const bool have_dense = q->n_dense_groups > 0 && q->dense.w.get<void>();
  const int b_dense = have_dense ? add_buffer(q->dense.w.get<void>()) : -1;
  const bool tiled = q->tiled.enabled;
  void *tiled_ptr = tiled ? (q->tiled.jit ? reinterpret_cast<void *>(q->tiled_dev.jit.code_base) : q->tiled_dev.stream.get<void>()) : nullptr;
  const size_t tiled_words = tiled ? (q->tiled.jit ? q->tiled_dev.jit.code_bytes / 4 : q->tiled_dev.stream.bytes() / 4) : 0;
  const int b_tiled = tiled ? add_buffer(tiled_ptr) : -1;
  if (b_gen < 0 || (have_dense && b_dense < 0) || (tiled && b_tiled < 0)) return fail(ESCOIN_EINVAL, "update_values: too many buffers");
  if (q->gen.vals.bytes() < sizeof(T) * (size_t)nnz) return fail(ESCOIN_EINVAL, "update_values: the plan's value array is shorter than its CSR");
  std::vector<char> sparse_here(g.d.group, 0);
  for (int grp = 0; grp < g.d.group; ++grp) {
    sparse_here[grp] = tiled && !group_is_dense(q, grp);
    if (sparse_here[grp] && (grp >= (int)q->tiled_dev.val_word.size() || q->tiled_dev.val_word[grp].size() != q->colidx[grp].size()))
      return fail(ESCOIN_EINVAL, "update_values: the plan's value map does not match its CSR");
  }
  // (the padded matrix holds every group's rows, whichever kernel runs them)
  const std::vector<int> dense_at = have_dense ? dense_positions(csr_view(q), dense_lda(g.kdim)) : std::vector<int>();
  const char *refused = nullptr;
  for_each_entry(csr_view(q), [&](const CsrEntry &c) {
    if (refused) return;
    const int s = src_of ? src_of[c.e] : (int)c.e;
    out->push_back({(unsigned char)b_gen, s, (unsigned)c.e});
    if (have_dense) {
      const size_t at = (size_t)dense_at[(size_t)c.e];
      if ((at + 1) * sizeof(T) > q->dense.w.bytes()) { refused = "update_values: dense destination out of range"; return; }
      out->push_back({(unsigned char)b_dense, s, (unsigned)at});
    }
    if (sparse_here[c.grp]) {
      const unsigned w = q->tiled_dev.val_word[c.grp][(size_t)c.j];
      if ((size_t)w >= tiled_words) { refused = "update_values: code / stream destination out of range"; return; }
      out->push_back({(unsigned char)b_tiled, s, w});
    }
  });
  return refused ? fail(ESCOIN_EINVAL, refused) : ESCOIN_OK;
}

// Whether the in-place path exists for plan q: generated code must sit in memory the library filled itself and carry a
// value map (a plan restored by the fast import has code but no map).
bool in_place_ok(const escoin_plan *q) {
  if (!(q->tiled.enabled && q->tiled.jit)) return true;
  return q->tiled_dev.jit.direct != nullptr && !q->tiled_dev.val_word.empty();
}

// The walk: every copy of the values of the plan the walk began at (the root), as reached from plan q, whose entry j
// holds the value of the root's entry (*outer)[j] (null: q is the root).  In this order:
//   q's own forward side                  on_plan(q, map)
//   q's derived plan of option "s2d" / "s2b"   this walk, through its map
//   the copy of q's backward state        its derived plan: this walk; an array: on_array(buf, elem_size, elem, map, n) -- for
//                                         k < n, element (elem ? elem[k] : k) of buf, elem_size bytes each, is a copy
// map[k] is the root's entry whose value the visited plan's entry k, or the array copy's k, holds (null: the identity).
// with_maps = false visits the plans alone: nothing is checked or composed, every map is null.  A visitor's nonzero
// return ends the walk and is returned; so is the refusal of a map that does not fit the CSR it indexes.
// (The "s2d" plan comes before the backward state's copy so that the list's buffers keep the order they always had: the
// plan, the inner plan, then the data gradient's copy, which either of the two may hold.)
template <typename Plan, typename OnPlan, typename OnArray>
int for_each_copy(Plan *q, const std::vector<int> *outer, bool with_maps, OnPlan &on_plan, OnArray &on_array) {
  const long nnz = plan_nnz(q);
  auto mismatch = [&](const char *what) {   // (outer: q is a derived plan)
    return fail(ESCOIN_EINVAL, std::string("update_values: ") + what + (outer ? " of a derived plan" : "") + " does not match the CSR");
  };
  if (outer && (long)outer->size() != nnz) return mismatch("the entry map");
  int rc = on_plan(q, outer ? outer->data() : nullptr);
  if (rc != ESCOIN_OK) return rc;
  std::vector<int> composed;
  // the map of a copy that holds q's entries in the order m (null, and nothing checked, without maps)
  auto through = [&](const std::vector<int> &m, const std::vector<int> **out) {
    *out = !with_maps ? nullptr : !outer ? &m : &composed;
    return !with_maps || ((long)m.size() == nnz && (!outer || compose_maps(outer, &m, nnz, &composed)));
  };
  const std::vector<int> *map = nullptr;
  if (const S2dState *sd = q->s2d_state.get()) {
    if (!through(sd->inner.src, &map)) return mismatch("the inner plan");
    if ((rc = for_each_copy<Plan>(sd->inner.plan.get(), map, with_maps, on_plan, on_array)) != ESCOIN_OK) return rc;
  }
  if (const S2bState *sb = q->s2b_state.get()) {   // (the identity map; a plan has one of the two states at most)
    if (!through(sb->inner.src, &map)) return mismatch("the inner plan");
    if ((rc = for_each_copy<Plan>(sb->inner.plan.get(), map, with_maps, on_plan, on_array)) != ESCOIN_OK) return rc;
  }
  if (const B2sState *bs = q->b2s_state.get()) {   // (the identity map; the backward state is the inner plan's alone)
    if (!through(bs->inner.src, &map)) return mismatch("the inner plan");
    if ((rc = for_each_copy<Plan>(bs->inner.plan.get(), map, with_maps, on_plan, on_array)) != ESCOIN_OK) return rc;
  }
  if (const D2sState *ds = q->d2s_state.get()) {   // (option "deconv": d2s_csr's map; the backward state is the inner plan's alone)
    if (!through(ds->inner.src, &map)) return mismatch("the inner plan");
    if ((rc = for_each_copy<Plan>(ds->inner.plan.get(), map, with_maps, on_plan, on_array)) != ESCOIN_OK) return rc;
  }
  const BwdState *s = q->bwd.get();
  if (!s) return ESCOIN_OK;
  switch (s->data) {
    case kBwdInner:   // the data gradient is the inner plan's, whose backward state the walk has just visited: no copy here
      break;
    case kBwdTransposed:
      if (!through(s->transposed.src, &map)) return mismatch("the backward state");
      return for_each_copy<Plan>(s->transposed.plan.get(), map, with_maps, on_plan, on_array);
    case kBwdMfma:
      if (!with_maps) break;
      // the phase matrices, always float: element pos[e] holds the value of q's entry e (csr_tables.h dgrad_mfma_tables)
      if ((long)s->dgm.pos.size() != nnz) return mismatch("the backward state");
      return on_array(s->dgm.mat, sizeof(float), s->dgm.pos.data(), outer ? outer->data() : nullptr, nnz);
    case kBwdGather:
      if (!with_maps) break;
      if (!through(s->gather.tsrc, &map)) return mismatch("the backward state");
      return on_array(s->gather.tval, q->is_f64 ? sizeof(double) : sizeof(float), nullptr, map->data(), nnz);
  }
  return ESCOIN_OK;
}

// Whether a backward state exists that holds a copy of p's values: p's own, or under options "b2s" / "deconv" the inner plan's.
bool has_bwd_state(const escoin_plan *p) {
  return p->bwd || (p->b2s_state && p->b2s_state->inner.plan->bwd) || (p->d2s_state && p->d2s_state->inner.plan->bwd);
}

const auto skip_arrays = [](const DeviceBuffer &, size_t, const int *, const int *, long) { return ESCOIN_OK; };

// entry_view: also the entry-major form of the list (UpdState::e_ptr), for the solver step.  vals_only: the plan has no
// in-place path -- the list is the value array alone, which a solver step writes before the plan is rebuilt from it.
template <typename T>
int build_state(escoin_plan *p, hipStream_t stream, bool entry_view, bool vals_only = false) {
  std::unique_ptr<UpdState> u(new UpdState());
  std::vector<Dst> dst;
  u->nnz = plan_nnz(p);
  if (vals_only) {
    if (u->nnz > 0 && p->gen.vals.bytes() < sizeof(T) * (size_t)u->nnz) return fail(ESCOIN_EINVAL, "solver_step: the plan's value array is shorter than its CSR");
    u->base[u->n_buffers++] = p->gen.vals.get<void>();
    for (long k = 0; k < u->nnz; ++k) dst.push_back({(unsigned char)0, (int)k, (unsigned)k});
    u->vals_only = true;
  } else {
    auto on_plan = [&](const escoin_plan *q, const int *map) { return collect<T>(q, map, u.get(), &dst); };
    // an array copy: one buffer, one destination per element, each checked against the array's size
    auto on_array = [&](const DeviceBuffer &buf, size_t elem_size, const int *elem, const int *map, long n) -> int {
      if (n == 0) return ESCOIN_OK;
      if (u->n_buffers >= kUpdMaxBuffers || elem_size != sizeof(T)) return fail(ESCOIN_EINVAL, "update_values: bad backward value array");
      const int b = u->n_buffers++;
      u->base[b] = buf.get<void>();
      for (long k = 0; k < n; ++k) {
        const size_t at = (size_t)(elem ? elem[k] : k);
        if ((at + 1) * sizeof(T) > buf.bytes()) return fail(ESCOIN_EINVAL, "update_values: backward destination out of range");
        dst.push_back({(unsigned char)b, map ? map[k] : (int)k, (unsigned)at});
      }
      return ESCOIN_OK;
    };
    const int rc = for_each_copy(p, nullptr, true, on_plan, on_array);
    if (rc != ESCOIN_OK) return rc;
    u->has_bwd = has_bwd_state(p);
  }
  std::stable_sort(dst.begin(), dst.end(), [](const Dst &a, const Dst &b) { return a.buf != b.buf ? a.buf < b.buf : a.src < b.src; });
  u->n_dst = (long)dst.size();
  const size_t n = std::max<size_t>(dst.size(), 1), nz = std::max<size_t>((size_t)u->nnz, 1);
  std::vector<int> src(dst.size());
  std::vector<unsigned> off(dst.size());
  std::vector<unsigned char> buf(dst.size());
  for (size_t k = 0; k < dst.size(); ++k) src[k] = dst[k].src, off[k] = dst[k].off, buf[k] = dst[k].buf;
  // the (bounds-checked) list by CSR entry; within an entry the buffers ascend
  EntryMajor em;
  if (entry_view && !entry_major(src, off, buf, u->nnz, &em)) return fail(ESCOIN_EINVAL, "solver_step: a destination names no CSR entry");
  src.resize(n, 0), off.resize(n, 0), buf.resize(n, 0);   // (an empty list still uploads one element)
  u->h_wpos = dense_positions(csr_view(p), p->g.kdim);
  ESCOIN_HIP_TRY(u->src.upload(src, stream));
  ESCOIN_HIP_TRY(u->off.upload(off, stream));
  ESCOIN_HIP_TRY(u->buf.upload(buf, stream));
  ESCOIN_HIP_TRY(u->wpos.upload(u->h_wpos, stream));
  ESCOIN_HIP_TRY(u->stage.alloc(sizeof(T) * nz));
  u->h_stage.assign(sizeof(T) * nz, 0);
  if (entry_view) {
    ESCOIN_HIP_TRY(u->e_ptr.upload(em.e_ptr, stream));
    ESCOIN_HIP_TRY(u->e_off.upload(em.e_off, stream));
    ESCOIN_HIP_TRY(u->e_buf.upload(em.e_buf, stream));
    u->entry_view = true;
  }
  ESCOIN_HIP_TRY(hipStreamSynchronize(stream));   // host vectors die at scope exit
  p->upd = std::move(u);
  return ESCOIN_OK;
}

// New values (compact, the plan's CSR order) into every HOST copy plan q keeps: the CSR's values and the kept copy of the
// generated code.  src_of as in collect().
template <typename T>
void patch_host(escoin_plan *q, const T *vals, const int *src_of) {
  std::vector<std::vector<T>> &hv = plan_vals<T>(q);
  const bool code = q->tiled.enabled && q->tiled.jit && !q->tiled_dev.jit_code.empty() && !q->tiled_dev.val_word.empty();
  long e = 0;
  for (int grp = 0; grp < q->g.d.group; ++grp) {
    const bool in_code = code && !group_is_dense(q, grp) && q->tiled_dev.val_word[grp].size() == q->colidx[grp].size();
    for (size_t j = 0; j < q->colidx[grp].size(); ++j, ++e) {
      const T v = vals[src_of ? src_of[e] : e];
      hv[grp][j] = v;
      if constexpr (sizeof(T) == 4)
        if (in_code) std::memcpy(&q->tiled_dev.jit_code[q->tiled_dev.val_word[grp][j]], &v, 4);
    }
  }
}

// ... into every plan copy of the walk; the array copies have no host mirror.  (A double plan has neither a backward
// state's derived plan nor an inner plan: the walk visits p alone.)
template <typename T>
void patch_host_all(escoin_plan *p, const T *vals) {
  auto on_plan = [&](escoin_plan *q, const int *map) { patch_host<T>(q, vals, map); return ESCOIN_OK; };
  for_each_copy(p, nullptr, true, on_plan, skip_arrays);   // (a map that does not fit was refused when the list was built)
}

// The fallback: the device side rebuilt from the host CSR with the new values, exactly as set_csr would.
template <typename T>
int update_by_rebuild(escoin_plan *p, const T *in, bool from_dense, bool on_device, hipStream_t stream) {
  const Geometry &g = p->g;
  const long nnz = plan_nnz(p);
  std::vector<T> host;
  const T *src = in;
  if (on_device) {
    const size_t count = from_dense ? (size_t)g.d.M * g.kdim : (size_t)nnz;
    host.resize(std::max<size_t>(count, 1));
    if (count) ESCOIN_HIP_TRY(hipMemcpyAsync(host.data(), in, sizeof(T) * count, hipMemcpyDeviceToHost, stream));
    ESCOIN_HIP_TRY(hipStreamSynchronize(stream));
    src = host.data();
  }
  std::vector<std::vector<T>> &hv = plan_vals<T>(p);
  const std::vector<int> wpos = from_dense ? dense_positions(csr_view(p), g.kdim) : std::vector<int>();
  for_each_entry(csr_view(p), [&](const CsrEntry &c) { hv[c.grp][c.j] = from_dense ? src[wpos[(size_t)c.e]] : src[c.e]; });
  p->aligned = false;
  const int rc = realign_from_host_csr(p, stream);     // (ends a device-authoritative state like any align)
  p->upd_last_fast = 0;
  return rc;
}

int sync_host(escoin_plan *p);

// What every device entry point that changes a plan's values checks first.
template <typename T>
int check_updatable(const escoin_plan *p, const char *name) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail(ESCOIN_ENODEVICE, std::string(name) + ": no HIP device (a plan aligned by escoin_weight_align_cpu is updated by escoin_update_values_cpu)");
  if (!p->aligned) return fail(ESCOIN_ESTATE, std::string(name) + " called before weight_align / set_csr");
  if (p->is_f64 != (sizeof(T) == 8))
    return fail(ESCOIN_ESTATE, std::string(name) + (p->is_f64 ? ": the plan holds double weights (use the _f64 entry point)" : "_f64: the plan holds float weights"));
  return check_plan_device(p, name);
}

// Whether the in-place path exists for p: in_place_ok of every plan copy of the walk.
bool plan_in_place_ok(const escoin_plan *p) {
  auto on_plan = [](const escoin_plan *q, const int *) { return in_place_ok(q) ? ESCOIN_OK : 1; };
  return for_each_copy(p, nullptr, false, on_plan, skip_arrays) == ESCOIN_OK;
}

template <typename T>
int update_t(escoin_plan *p, const T *in, bool from_dense, int on_device, void *stream_v) {
  const char *name = from_dense ? "update_values" : "set_values";
  if (!p || !in) return fail(ESCOIN_EINVAL, std::string(name) + ": null argument");
  if (const int rc = check_updatable<T>(p, name)) return rc;
  hipStream_t stream = (hipStream_t)stream_v;
  ++p->upd_count;
  if (!plan_in_place_ok(p)) return update_by_rebuild<T>(p, in, from_dense, on_device != 0, stream);
  if (!p->upd || p->upd->vals_only || (has_bwd_state(p) && !p->upd->has_bwd)) {
    const bool entry_view = p->upd && p->upd->entry_view && !p->upd->vals_only;
    p->upd.reset();
    const int rc = build_state<T>(p, stream, entry_view);
    if (rc != ESCOIN_OK) return rc;
  }
  UpdState *u = p->upd.get();
  p->upd_last_fast = 1;
  if (u->n_dst == 0) return ESCOIN_OK;
  UpdArgs a;
  for (int b = 0; b < kUpdMaxBuffers; ++b) a.base[b] = u->base[b];
  a.src = u->src.get<int>(); a.off = u->off.get<unsigned>(); a.buf = u->buf.get<unsigned char>(); a.wpos = u->wpos.get<int>();
  a.n_dst = u->n_dst;
  const dim3 grid((unsigned)((u->n_dst + 255) / 256)), block(256);
  if (on_device) {
    if (from_dense) hipLaunchKernelGGL((escoin_update_values_kernel<T, true>), grid, block, 0, stream, a, in);
    else hipLaunchKernelGGL((escoin_update_values_kernel<T, false>), grid, block, 0, stream, a, in);
    ESCOIN_HIP_TRY(hipGetLastError());
    // the plan cannot see a graph replay: from here until the next align the device holds the values
    p->dev_authoritative = true;
    p->sync_host_fn = sync_host;
    p->upd_stream = stream;
    return ESCOIN_OK;
  }
  // host source: compact values -> the host mirrors directly, and through the staging buffer into the same kernel
  T *hs = reinterpret_cast<T *>(u->h_stage.data());
  for (long e = 0; e < u->nnz; ++e) hs[e] = from_dense ? in[u->h_wpos[(size_t)e]] : in[e];
  patch_host_all<T>(p, hs);
  p->dev_authoritative = false;      // (every value was just replaced on both sides)
  ESCOIN_HIP_TRY(hipMemcpyAsync(u->stage.get<T>(), hs, sizeof(T) * (size_t)u->nnz, hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL((escoin_update_values_kernel<T, false>), grid, block, 0, stream, a, u->stage.get<const T>());
  ESCOIN_HIP_TRY(hipGetLastError());
  ESCOIN_HIP_TRY(hipStreamSynchronize(stream));   // the staging area is reused by the next host-source update
  return ESCOIN_OK;
}

template <typename T>
int sync_host_t(escoin_plan *p) {
  const long nnz = plan_nnz(p);
  if (nnz > 0) {
    // gen.vals is the device's value array in CSR order (every plan kind keeps it)
    std::vector<T> vals((size_t)nnz);
    ESCOIN_HIP_TRY(hipMemcpyAsync(vals.data(), p->gen.vals.get<T>(), sizeof(T) * (size_t)nnz, hipMemcpyDeviceToHost, p->upd_stream));
    ESCOIN_HIP_TRY(hipStreamSynchronize(p->upd_stream));
    patch_host_all<T>(p, vals.data());
  }
  p->dev_authoritative = false;
  return ESCOIN_OK;
}

int sync_host(escoin_plan *p) { return p->is_f64 ? sync_host_t<double>(p) : sync_host_t<float>(p); }

}  // namespace

template <typename T>
int solver_begin(escoin_plan *p, const char *name, hipStream_t stream, SolverTargets *t) {
  if (const int rc = check_updatable<T>(p, name)) return rc;
  ++p->upd_count;
  *t = SolverTargets();
  t->in_place = plan_in_place_ok(p);
  t->nnz = plan_nnz(p);
  if (t->nnz == 0) return ESCOIN_OK;      // (nothing is launched: "update_fast" keeps what the last real update left)
  const UpdState *have = p->upd.get();
  if (!have || !have->entry_view || have->vals_only != !t->in_place || (t->in_place && has_bwd_state(p) && !have->has_bwd)) {
    p->upd.reset();
    const int rc = build_state<T>(p, stream, true, !t->in_place);
    if (rc != ESCOIN_OK) return rc;
  }
  const UpdState *u = p->upd.get();
  if (u->nnz != t->nnz || p->gen.vals.bytes() < sizeof(T) * (size_t)t->nnz) return fail(ESCOIN_EINVAL, std::string(name) + ": the update state does not match the CSR");
  for (int b = 0; b < kUpdMaxBuffers; ++b) t->base[b] = u->base[b];
  t->e_ptr = u->e_ptr.get<int>(), t->e_off = u->e_off.get<unsigned>(), t->e_buf = u->e_buf.get<unsigned char>(), t->wpos = u->wpos.get<int>();
  t->vals = p->gen.vals.get<void>();
  p->upd_last_fast = t->in_place ? 1 : 0;   // (as in update_t: only once the state exists)
  return ESCOIN_OK;
}

template <typename T>
int solver_end(escoin_plan *p, const SolverTargets &t, hipStream_t stream) {
  if (t.nnz == 0) return ESCOIN_OK;
  if (!t.in_place) {
    // the value array holds the new values: read back, everything rebuilt from them as set_csr would (this drops p->upd)
    return update_by_rebuild<T>(p, static_cast<const T *>(t.vals), false, true, stream);
  }
  // the plan cannot see a graph replay: from here until the next align the device holds the values
  p->dev_authoritative = true;
  p->sync_host_fn = sync_host;
  p->upd_stream = stream;
  return ESCOIN_OK;
}
template int solver_begin<float>(escoin_plan *, const char *, hipStream_t, SolverTargets *);
template int solver_begin<double>(escoin_plan *, const char *, hipStream_t, SolverTargets *);
template int solver_end<float>(escoin_plan *, const SolverTargets &, hipStream_t);
template int solver_end<double>(escoin_plan *, const SolverTargets &, hipStream_t);

}  // namespace escoin

using namespace escoin;

extern "C" {

int escoin_update_values(escoin_plan *p, const float *dense_w, int w_on_device, void *stream) {
  return guarded([&]() -> int { return update_t<float>(p, dense_w, true, w_on_device, stream); });
}
int escoin_update_values_f64(escoin_plan *p, const double *dense_w, int w_on_device, void *stream) {
  return guarded([&]() -> int { return update_t<double>(p, dense_w, true, w_on_device, stream); });
}
int escoin_plan_set_values(escoin_plan *p, const float *values, int on_device, void *stream) {
  return guarded([&]() -> int { return update_t<float>(p, values, false, on_device, stream); });
}
int escoin_plan_set_values_f64(escoin_plan *p, const double *values, int on_device, void *stream) {
  return guarded([&]() -> int { return update_t<double>(p, values, false, on_device, stream); });
}

}  // extern "C"
