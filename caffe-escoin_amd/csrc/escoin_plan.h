// Internal plan structure of libescoin_hip.so (not part of the C ABI).
#ifndef ESCOIN_PLAN_H_
#define ESCOIN_PLAN_H_

#include <hip/hip_runtime.h>

#include <chrono>
#include <memory>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "csr_tables.h"
#include "device_buffer.h"
#include "align_rules.h"
#include "escoin.h"
#include "geometry.h"
#include "jit_module.h"
#include "stream_builder.h"

namespace escoin {

// Thread-local error message behind escoin_last_error().
void set_error(const std::string &msg);
int fail(int code, const std::string &msg);
// Two checks of the device entry points (escoin_capi.hip): the current device is the one the plan was aligned on (`who`
// begins the message), and n_images lies in [0, desc.N].  ESCOIN_OK or the failure's code, the message set.
int check_plan_device(const escoin_plan *p, const std::string &who);
int check_n_images(const escoin_plan *p, int n_images);

#define ESCOIN_HIP_TRY(expr)                                                          \
  do {                                                                                \
    hipError_t e__ = (expr);                                                          \
    if (e__ != hipSuccess)                                                            \
      return ::escoin::fail(ESCOIN_EHIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
  } while (0)

// Milliseconds of wall time since t0 (the "*_ms" fields of a plan)
inline double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// No exception may cross the C ABI (std::bad_alloc from the host vectors, std::system_error from a thread team):
// every entry point that allocates runs its body through this.
template <typename F>
inline int guarded(F &&body) {
  try {
    return body();
  } catch (const std::bad_alloc &) {
    return fail(ESCOIN_ENOMEM, "out of host memory");
  } catch (const std::exception &e) {
    return fail(ESCOIN_EINVAL, std::string("internal error: ") + e.what());
  } catch (...) {
    return fail(ESCOIN_EINVAL, "internal error");
  }
}

// Parameters of the tiled kernel chosen in weight_align (see sconv_tiled.hip).
struct TiledConfig {
  bool enabled = false;
  size_t lds_bytes = 0;
  int lds_budget = 0;  // plane-buffer budget the tiling was chosen with
  float density = 0.f; // nonzero fraction of the weights the tiling was chosen with
  Tiling tiling;       // the tiling itself (chosen once in WeightAlign; launches only read it)
  int stage_bytes = 0; // LDS bytes of one wave's weight-stream staging area
  int nbuf = 2;        // plane / staging buffers per workgroup
  bool jit = false;    // the walk is generated code (jit_codegen.h) instead of the LDS-staged stream
  long jit_rows = 0, jit_records = 0;
  bool jit_dma = false;      // ... and its units stage the next block's planes themselves (jit_codegen.h DmaPlan)
  int dma_period = 0;        // quads covered by the quad table (lcm of the plane size and 64)
  int jit_pref = 0;          // code touches at the start of every unit
  bool jit_chain = false;    // a tile's units run as one chain (jit_codegen.h ChainPlan)
  float deal_slowest_over_mean = 1.f, deal_worst_block = 1.f;   // balance of the channel deal (jit_codegen.h Program)
  std::string info;          // escoin_plan_tiling_info
  mutable int body_variant_last = 0;   // stat "body_variant": the compiled body of the last tiled launch (0 generic, 1 chained)
  mutable int touch_stride_last = 1;   // stat "code_touchers": the code-touch stride of the last tiled launch (align_rules.h touch_election)
  mutable TiledLaunchShape launch_shape_last;   // ... and its shape: stat "touch_lines_per_launch" counts from the two
};

// One host thread's buffers of the CPU mode (sconv_cpu.cpp): the shared-halo padded image and the store scratch.
struct CpuWorkspace {
  std::vector<char> pad, scratch, partial;   // padded image, one tile for the stores, parked sums of channel blocking
  const void *src = nullptr;     // the bottom image the padded buffer currently holds ...
  unsigned long call = 0;        // ... as of this escoin_forward_cpu call
};

// A derived plan: a second plan that its owner builds for itself (build_derived_plan), whose CSR entries are copies of
// the owner's.  A change of the owner's values reaches them through the map (update_values.hip for_each_copy); a change of
// its pattern drops the state that holds the derived plan (free_device).
struct DerivedPlan {
  std::unique_ptr<escoin_plan, int (*)(escoin_plan *)> plan{nullptr, escoin_plan_destroy};
  std::vector<int> src;   // host: this plan's entry k holds the value of the owner's entry src[k] (flat index, groups concatenated)
};

// What the first escoin_backward on an alignment builds (sconv_backward.hip, as align_rules.h bwd_choice decides); reset
// with the device side.  One sub-struct per kernel, each with the device bytes of its own buffers, and what the kernels
// share.  The state holds at most one copy of the plan's values for the data gradient, and `data` says which.

// The gather kernel (kBwdGather): the transposed CSR (csr_tables.h gather_transpose)
struct GatherDgrad {
  DeviceBuffer trow;   // [C + 1] absolute offsets into ttap / tval
  DeviceBuffer ttap;   // per transposed entry: ocl << 16 | kr << 8 | kc
  DeviceBuffer tval;   // float or double values, in the transposed order
  // host: element k of tval (and of ttap) holds the value of the plan's CSR entry tsrc[k] (flat index, groups
  // concatenated).  Not transposed.src: the gather kernel's order is another than the transposed plan's.
  std::vector<int> tsrc;
  size_t bytes() const { return trow.bytes() + ttap.bytes() + tval.bytes(); }
};

// The LDS-staged weight-gradient kernel (ESCOIN_WGRAD_STAGED; align_rules.h StgPlan, csr_tables.h staged_tables)
struct StagedWgrad {
  int icb = 0, nblk = 0;       // input channels per staged block, blocks per conv group
  int rows = 0;                // padded rows of the LDS tile (the longest chunk's span)
  int osplit = 1;              // workgroups a conv group's output channels are dealt over
  size_t lds_bytes = 0;
  DeviceBuffer blk;  // [M][nblk + 1] absolute entry index where output channel oc's entries of block b begin
  DeviceBuffer off;  // [nnz] per CSR entry: its tap's float offset inside the staged block's LDS tile
  size_t bytes() const { return blk.bytes() + off.bytes(); }
};

// The fp32-MFMA weight-gradient kernel (ESCOIN_WGRAD_MFMA; wgrad_mfma.hip; the tables: csr_tables.h wgrad_mfma_tables)
struct WgmState {
  int mtiles = 0, ktiles = 0;  // tiles per conv group along the output channels / the columns
  size_t lds_bytes = 0;
  DeviceBuffer ent;   // [M * kdim] (row, column) -> CSR entry, -1: none
  DeviceBuffer cnt;   // [group * mtiles * ktiles] entries per tile
  DeviceBuffer ktab;  // [4 * ktiles * tile_k] the im2col decode of a column
  size_t bytes() const { return ent.bytes() + cnt.bytes() + ktab.bytes(); }
};

// The pointwise weight-gradient kernel (ESCOIN_WGRAD_POINTWISE; wgrad_pointwise.hip; the tiling: align_rules.h pw_plan on
// the plan's CSR; the tables: csr_tables.h pw_tables)
struct PwWgrad {
  int tiles = 0, bias_tiles = 0;   // workgroups per chunk; the leading ones that sum the bias
  int lane_entries = 1;            // E: the kernel instantiation
  size_t lds_bytes = 0;
  DeviceBuffer tile;  // [tiles][kPwTileWords]
  DeviceBuffer ent;   // per item: the CSR entry
  DeviceBuffer pk;    // per item: (G row << 16) | bottom row of the tile's LDS image
  size_t bytes() const { return tile.bytes() + ent.bytes() + pk.bytes(); }
};

// The fp32-MFMA data-gradient kernel (kBwdMfma; dgrad_mfma.hip; the tables: csr_tables.h dgrad_mfma_tables)
struct DgmState {
  int phases = 0, ctiles = 0, cols_total = 0;
  size_t lds_bytes = 0;
  DeviceBuffer mat;    // the phase matrices: the weights transposed, columns permuted by phase, zero outside the pattern
  DeviceBuffer phase;  // [phases][8] a phase's pixels, columns and place in col / mat
  DeviceBuffer col;    // [4 * cols_total] the decode of a column: {G offset of ocl, dh, dw, valid}
  DeviceBuffer lptr;   // [group * phases * ctiles + 1] into live
  DeviceBuffer live;   // the live steps of every (group, phase, channel tile), ascending
  std::vector<int> ppix;   // host: [phases] a phase's pixels per image (the launch's grid)
  std::vector<int> pos;    // host: [nnz] the element of mat that holds CSR entry e -- how weight updates reach it
  size_t bytes() const { return mat.bytes() + phase.bytes() + col.bytes() + lptr.bytes() + live.bytes(); }
};

struct BwdState {
  // who computes the data gradient, and with it where the state's copy of the values is: the inner plan's backward state
  // (kBwdInner: option "s2d" or "s2b", the inner plan's backward followed by the unpack kernel -- this state then holds the weight
  // gradient's side only), `transposed`, gather.tval, dgm.mat
  BwdDataPath data = kBwdGather;
  DerivedPlan transposed;   // kBwdTransposed: the data gradient as a stride-1 forward of top_diff; plan null on the other paths
  GatherDgrad gather;
  DgmState dgm;
  DeviceBuffer wpos;   // per CSR entry: oc * kdim + colidx (its position in weight_diff)
  DeviceBuffer slab;   // [chunks_max][nnz] weight partials, then [chunks_max][M] bias partials
  DeviceBuffer g;      // fuse_relu + kBwdTransposed: top_diff * [top > 0], desc.N x M x OH x OW
  long nnz = 0;
  int chunks_max = 0, last_chunks = 0;
  // weight gradient (option "wgrad_kernel"): wgrad = what the option resolved to on this alignment, last_wgrad = what the
  // last weight / bias gradient ran (0: none yet)
  int wgrad = ESCOIN_WGRAD_ENTRY, last_wgrad = 0;
  StagedWgrad stg;
  WgmState wgm;
  PwWgrad pw;
  double align_ms = 0.0;
};

// What upload() builds for a plan that option "s2d" serves (escoin_capi.hip; the rules: align_rules.h s2d_plan, csr_tables.h
// s2d_csr; the kernels: s2d.hip); reset with the device side.
struct S2dState {
  S2dPlan sp;
  DerivedPlan inner;           // the stride-1 plan; its own backward state may hold a derived plan of this derived plan
  DeviceBuffer x;              // X' for the forward, dX' for the data gradient: sp.x_floats floats
};

// What upload() builds for a plan that option "s2b" serves (escoin_capi.hip; the rule: align_rules.h s2b_plan; the kernels:
// s2b.hip); reset with the device side.  A plan has at most one of the two states: the options serve disjoint geometries.
struct S2bState {
  S2bPlan sp;
  DerivedPlan inner;           // the undilated plan of N * P images on the outer CSR (src: the identity)
  DeviceBuffer x, t;           // X' / dX': sp.x_floats floats; T' / G': sp.t_floats floats
};

// What upload() builds for a plan that option "b2s" serves (escoin_capi.hip; the rule: align_rules.h b2s_plan; the kernels:
// b2s.hip); reset with the device side.  A plan has at most one of the three states.  The whole backward is the inner
// plan's: the plan itself builds no BwdState.
struct B2sState {
  B2sPlan bp;
  DerivedPlan inner;           // the pointwise plan of ceil(N / B) images of 1 x B on the outer CSR (src: the identity)
  DeviceBuffer x, t, dx;       // X': bp.x_floats floats; T' / G': bp.t_floats floats; dX': bp.x_floats floats (X' is the
                               // weight gradient's operand in the same inner call)
};

// What upload() builds for a plan with option "deconv" (escoin_capi.hip; the rules: align_rules.h d2s_plan, csr_tables.h
// d2s_csr; the kernels: d2s.hip); reset with the device side.  A plan has at most one of the four states.  The whole
// backward is the inner plan's, around the pack kernel and the gradients' carry: the plan itself builds no BwdState.
struct D2sState {
  D2sPlan dp;
  DerivedPlan inner;           // the stride-1 plan of M * P output channels on the caller's bottom; holds the only forward copy of the weights
  DeviceBuffer t;              // T' (forward) / G' (backward): dp.t_floats floats
  DeviceBuffer wv, bv;         // the inner compact weight gradient [nnz] and the inner bias gradient [M * P], zeroed per call
  DeviceBuffer src, wpos;      // [nnz] inner entry k -> outer entry (inner.src), -> its position in blobs_[0] (C x Mg x KH x KW)
  size_t scratch_bytes() const { return t.bytes() + wv.bytes() + bv.bytes() + src.bytes() + wpos.bytes(); }
};

// What the first escoin_dense_wgrad on a plan builds (dense_wgrad.hip).  A function of the descriptor, the device's CU
// count and option "dense_wgrad_splits" alone -- not of the pattern or the values -- so no align resets it: it lives until
// the plan is destroyed (or until a call finds the plan aligned on another device, which builds it anew there).
struct DenseWgradState {
  int device = -1;
  int mtiles = 0, ktiles = 0;          // tiles per conv group along the output channels / the columns
  int span = 0, splits = 0;            // chunks per split, splits of the full batch (align_rules.h dwg_plan)
  long positions = 0;                  // D = M * Cg * KH * KW
  size_t lds_bytes = 0;
  DeviceBuffer ktab;                   // [4 * ktiles * tile_k] the im2col decode of a column (csr_tables.h im2col_ktab)
  DeviceBuffer part;                   // [splits][D] partial sums
};

// What the first escoin_update_values on an alignment builds (update_values.hip); reset with the device side.  One flat
// scatter list over every device word that holds a weight of this alignment: destination k receives the value of CSR
// entry src[k] at element off[k] (elements of the plan's Dtype) of buffer buf[k].
constexpr int kUpdMaxBuffers = 8;
struct UpdState {
  DeviceBuffer src, off, buf;   // [n_dst] int32 / uint32 / uint8, sorted by (buffer, CSR entry)
  DeviceBuffer wpos;            // [nnz] per CSR entry: its position in blobs_[0] (oc * kdim + colidx)
  DeviceBuffer stage;           // [nnz] compact values of a host-source update on their way to the kernel
  void *base[kUpdMaxBuffers] = {};
  int n_buffers = 0;
  long n_dst = 0, nnz = 0;
  // the list was built after the backward state (the plan's, and with it its derived plans'), so the walk found those
  // states' copies; a list without is rebuilt once when the state appears
  bool has_bwd = false;
  std::vector<char> h_stage;    // host side of `stage`
  std::vector<int> h_wpos;      // host side of `wpos`: where a host-source update finds entry e in a dense blobs_[0]
  // The same list entry-major, for the solver step (solver_step.hip), which computes a value once per CSR entry: entry e
  // is stored at element e_off[k] of buffer e_buf[k] for k in [e_ptr[e], e_ptr[e + 1]).  Built with the first solver
  // step on an alignment (entry_view), kept by the rebuild that follows the backward state's appearance.
  DeviceBuffer e_ptr, e_off, e_buf;   // [nnz + 1] int32, [n_dst] uint32, [n_dst] uint8
  bool entry_view = false;
  bool vals_only = false;       // a plan without an in-place path: the value array is the only destination (solver step, then a rebuild)
};

// What a solver step needs of the update state (update_values.hip): where the plan's current values are and the
// entry-major destinations of the new ones.
struct SolverTargets {
  void *base[kUpdMaxBuffers];
  const int *e_ptr, *wpos;
  const unsigned *e_off;
  const unsigned char *e_buf;
  void *vals;        // gen.vals: nnz elements of the plan's Dtype, CSR order
  long nnz;
  bool in_place;     // false: the value array is the only destination and solver_end rebuilds the plan from it
};

// The generic kernel's device CSR (escoin_capi.hip upload; csr_tables.h generic_tables): rowptr [M + 1] absolute offsets
// into taps / vals; taps and vals [max(nnz, 1)], the packed (ic,kr,kc) and the values of the plan's Dtype
struct GenericArrays { DeviceBuffer rowptr, taps, vals; };

// What tiled_build / tiled_import put on the device for the tiled kernels
struct TiledArrays {
  DeviceBuffer stream;     // unit bodies of the weight stream (stream_builder.h)
  DeviceBuffer unit_hdr;   // 8 dwords per (conv group, oc group, ic block); generated code: 1 (code offset)
  DeviceBuffer chan;       // slot -> output channel (WeightStream::chan)
  JitModule jit;           // generated-code kernel: where the plan's code lives on the device (jit_module.h)
  // host: [conv group][index in colidx] -> the word of the stream / of the generated code that holds the value
  // (WeightStream::val_word, jit::Program::val_word); empty for a plan restored by the fast import
  std::vector<std::vector<uint32_t>> val_word;
  // host copies of what a generated-code plan loaded, kept for escoin_plan_export_aligned: the code
  // (position-independent words, jit_codegen.h), the unit table and the channel deal
  std::vector<uint32_t> jit_code, h_unit_off, h_chan;
};

// The dense fallback's device side (upload, dense_build_ktab)
struct DenseArrays {
  DeviceBuffer w;          // [M + dense_spare_rows()][dense_lda(Cg*KH*KW)], zero padded
  DeviceBuffer ktab;       // im2col decode per k: {image offset, dy | dx << 16} (dense_mfma.hip)
  // stream-K (dense_mfma.hip), allocated at WeightAlign for layers whose launches may split K: a launch never allocates
  DeviceBuffer sk_ws;      // flag words, then the partial accumulators
  int sk_flag_words = 0;
  MappedWord sk_fail;      // the word the kernel sets when a fix-up wait gave up (sticky until the next WeightAlign)
  mutable bool sk_used = false;   // the last dense launch of this plan split K (escoin_plan_stat "streamk")
  // the instantiation and store path of the last dense launch: WROWS + 4 * BMODE + 8 * vec_out + 16 * STREAMK, 0 before
  // the first one (escoin_plan_stat "dense_variant")
  mutable int variant_last = 0;
};

}  // namespace escoin

struct escoin_plan {
  escoin::Geometry g;
  int kernel_choice = ESCOIN_KERNEL_AUTO;
  int conv_mode = ESCOIN_CONV_MODE_SCONV_PAR;
  int dense_gate = 0;
  long max_launch_bytes = 0;   // option "max_launch_bytes": bottom-blob bytes one tiled launch may cover (0: the 4 GiB descriptor range)
  int tiling_batch = 0;   // option "tiling_batch": choose the tiled kernel's tiling as for this batch (0: desc.N)
  bool aligned = false;
  int device = -1;

  // host CSR, per group (unstretched column indices), exactly what
  // caffe_cpu_sparse_dense2csr produces (math_functions.cpp:92-105)
  std::vector<std::vector<int>> rowptr;   // [group][Mg+1]
  std::vector<std::vector<int>> colidx;   // [group][nnz_g]
  std::vector<std::vector<float>> values; // [group][nnz_g]   (Dtype = float plans)
  // Dtype = double (conv_layer.cpp:102 INSTANTIATE_CLASS): the align call fixes a plan's type; a double plan keeps its
  // values here, runs the order-preserving generic kernel on the device (no fast path) and the same host kernel
  std::vector<std::vector<double>> values64;
  bool is_f64 = false;
  // Caffe::CPU mode (sconv_cpu.cpp): true once a CSR is on the host, whether or not a device was there to upload to;
  // cpu_off = the nonzeros' offsets into the shared-halo padded image for THIS geometry (dilation folded in), built on
  // the first escoin_forward_cpu after an align
  bool host_aligned = false;
  std::vector<std::vector<int>> cpu_off;
  bool cpu_off_valid = false;
  // channel blocking of the CPU mode (sconv_cpu.h GroupJob::blk_ptr): per conv group, Mg x (cpu_blk_n + 1) nonzero indices
  // for blocks of cpu_blk_cb input channels (-1: not built; 0: this geometry runs unblocked)
  std::vector<std::vector<int>> cpu_blk;
  int cpu_blk_cb = -1, cpu_blk_n = 0, cpu_blk_isa = 0, cpu_blk_elem = 0;
  int cpu_img_force = 0;          // option "cpu_images_per_job": 0 = chosen from the geometry, n = at most n images per job
  int cpu_img_last = 0;           // what the last escoin_forward_cpu used
  int cpu_blk_force = 0;          // option "cpu_channel_block": 0 = chosen from the geometry, > 0 = this many channels per block
  std::vector<escoin::CpuWorkspace> cpu_ws;   // per team thread: padded image + store scratch
  unsigned long cpu_calls = 0;

  // Device memory has one owner each (gen, tiled_dev, dense, col, bwd): the device bytes are computed from them, and
  // weight_align / set_csr / import_aligned reset them all (free_device) before they build anew.
  escoin::GenericArrays gen;
  escoin::TiledConfig tiled;      // the tiled kernel's parameters (a plain value)
  escoin::TiledArrays tiled_dev;
  int code_loader = 0;            // option "code_loader": 0 executable device memory first, 1 the code object loader (jit_module.h)
  double align_ms = 0.0;          // wall time of the last weight_align / set_csr / import_aligned
  bool import_fast = false;       // the last import_aligned loaded a persisted code object as it was
  int small_rule = 0;              // KERNEL_AUTO's small-launch rule applied to this plan: 0 not considered, 1 kept generated code, 2 took the generic kernel

  // dense fallback (fp32 MFMA implicit GEMM), chosen per conv group: bit g of dense_mask = group g
  // goes to the MFMA kernel, bit g of sparse_mask = to the sparse kernels (layers with more than 64
  // groups take one decision for all of them: both masks are then all-ones / zero)
  escoin::DenseArrays dense;
  bool use_dense = false;         // every group dense
  unsigned long long dense_mask = 0, sparse_mask = ~0ull;
  int n_dense_groups = 0, n_sparse_groups = 0;
  int dense_threshold_pct = -1;   // option "dense_threshold_pct" (-1: the measured default)
  int body_variant = -1;          // option "body_variant": -1 the rule (align_rules.h body_variant), 0 always the generic body
  int code_touchers = 0;          // option "code_touchers": 0 the rule (align_rules.h touch_election), k >= 1 every k-th workgroup of an XCD and grid row
  int stream_stores = -1;         // option "stream_stores": pointwise layers write the top blob with non-temporal stores (1), never (0), by size (-1)

  // LOWERED_SPARSE comparator (sconv_lowered.hip): column buffer, grown on demand by the forward
  escoin::DeviceBuffer col;

  std::string kernel_name = "(not aligned)";

  // Backward (sconv_backward.hip): option "backward_kernel" and the state the first escoin_backward builds; reset with
  // the device side (free_device), so weight_align / set_csr / import_aligned drop it
  int bwd_kernel = ESCOIN_KERNEL_AUTO;
  int wgrad_kernel = ESCOIN_WGRAD_AUTO;   // option "wgrad_kernel"
  int wgrad_channel_block = 0;            // option "wgrad_channel_block" (0: from the geometry and the LDS budget)
  int wgrad_pointwise = 0;                // option "wgrad_pointwise": AUTO runs the pointwise kernel where it serves the plan
  int wgrad_pw_tile_entries = 0;          // option "wgrad_pointwise_tile_entries" (test option; 0: the rule)
  std::unique_ptr<escoin::BwdState> bwd;

  // In-place weight updates (update_values.hip): the state the first escoin_update_values builds; reset with the device
  // side.  From a device-source update until the next align (or host-source update) the DEVICE holds the plan's values
  // and the host mirrors are stale: whatever reads weights from the host calls sync_host_values first.
  std::unique_ptr<escoin::UpdState> upd;
  bool dev_authoritative = false;
  int (*sync_host_fn)(escoin_plan *) = nullptr;   // set with dev_authoritative: the read-back (update_values.hip)
  hipStream_t upd_stream = nullptr;   // the stream of the last device-source update
  int upd_last_fast = 0;              // stat "update_fast"
  long upd_count = 0;                 // stat "update_count": updates since the plan was created

  // Pruning (prune_select.hip): stats "prune_count" (prunes since the plan was created) and "prune_last_dropped"
  long prune_count = 0, prune_last_dropped = 0;
  // the last escoin_plan_prune's phases: the selection / scan / map launches (device events), the call's wall time until
  // the host holds the map, and from there to the end of the re-align
  double prune_kernels_ms = 0.0, prune_map_ms = 0.0, prune_realign_ms = 0.0;

  // Rewiring (rewire_select.hip): stats "rewire_count" (rewires since the plan was created), "rewire_last_dropped",
  // "rewire_last_grown", and the last escoin_plan_rewire's phases, as for a prune
  long rewire_count = 0, rewire_last_dropped = 0, rewire_last_grown = 0;
  double rewire_kernels_ms = 0.0, rewire_map_ms = 0.0, rewire_realign_ms = 0.0;

  // Space-to-depth (s2d.hip): option "s2d" and what upload() builds where it applies; reset with the device side
  int s2d = 0;
  std::unique_ptr<escoin::S2dState> s2d_state;
  // Space-to-batch (s2b.hip): option "s2b" and what upload() builds where it applies; reset with the device side
  int s2b = 0;
  std::unique_ptr<escoin::S2bState> s2b_state;
  // Batch-to-space (b2s.hip): options "b2s" and "b2s_block" and what upload() builds where they apply; reset with the device side
  int b2s = 0, b2s_block = 0;
  std::unique_ptr<escoin::B2sState> b2s_state;
  // Deconvolution (d2s.hip): option "deconv", the descriptor as the caller gave it (with the option set, g is the mirror
  // convolution's geometry -- M <-> C, H x W <-> OH x OW -- whose weight matrix, CSR and aligned form are this layer's) and
  // what upload() builds; reset with the device side.  cpu_inner: the CPU mode's inner plan (sconv_cpu.cpp), host only
  int deconv = 0;
  escoin_conv_desc user_desc = {};
  std::unique_ptr<escoin::D2sState> d2s_state;
  escoin::DerivedPlan cpu_inner;
  std::vector<float> cpu_t, cpu_wv, cpu_bv;
  // the inner plan of whichever of the four options serves this plan (null: none does)
  const escoin::DerivedPlan *inner_plan() const {
    return s2d_state ? &s2d_state->inner : s2b_state ? &s2b_state->inner : b2s_state ? &b2s_state->inner :
           d2s_state ? &d2s_state->inner : nullptr;
  }

  // Dense weight gradient (dense_wgrad.hip): option "dense_wgrad_splits" (0: the rule decides, n: at most n splits of the
  // pixel axis), the state the first escoin_dense_wgrad builds -- kept across aligns -- and stat "dwg_count" (device
  // calls since the plan was created)
  int dense_wgrad_splits = 0;
  std::unique_ptr<escoin::DenseWgradState> dwg;
  long dwg_count = 0;
};

namespace escoin {

// escoin_capi.hip: caffe_cpu_sparse_dense2csr over every conv group of a dense blobs_[0] (math_functions.cpp:92-105,
// base_conv_layer.cpp:55-66) into the plan's host CSR; fixes the plan's Dtype, releases what an earlier align left on
// the device and leaves the plan host_aligned (and not device-aligned).  T = float | double.
template <typename T> void csr_from_dense(escoin_plan *p, const T *w);

// sconv_generic.hip
int launch_generic(const escoin_plan *p, const float *bottom, const float *bias, float *top,
                   int n_images, hipStream_t stream);
int launch_generic_f64(const escoin_plan *p, const double *bottom, const double *bias, double *top,
                       int n_images, hipStream_t stream);
const char *generic_kernel_name(bool relu);
const char *generic_kernel_name_f64(bool relu);

// The values of a plan's Dtype: p->values (float) or p->values64 (double).
template <typename T> std::vector<std::vector<T>> &plan_vals(escoin_plan *p);
template <> inline std::vector<std::vector<float>> &plan_vals<float>(escoin_plan *p) { return p->values; }
template <> inline std::vector<std::vector<double>> &plan_vals<double>(escoin_plan *p) { return p->values64; }

// escoin_capi.hip: the device bytes a plan's owners hold -- the forward's (stat "device_bytes") and the backward
// state's, its transposed plan's included (stat "bwd_device_bytes"); escoin_plan_workspace_bytes is their sum.
struct DeviceBytes { size_t fwd, bwd, upd, dwg; };   // dwg: the dense weight gradient's state (stat "dwg_device_bytes")
DeviceBytes device_bytes(const escoin_plan *p);
// dense_wgrad.hip builds the dense weight gradient's state; escoin_capi.hip answers its "dwg_*" stats
long dwg_stat(const escoin_plan *p, const char *key);
// escoin_capi.hip: the shared tail of weight_align / set_csr -- rebuilds the device side from the host CSR
int realign_from_host_csr(escoin_plan *p, hipStream_t stream);
// escoin_capi.hip (in the core for the reason S2dHooks gives below): a derived plan of the float plan `owner` into *out --
// descriptor `desc`, the owner's options and these two kernel options, aligned on `csr` with the owner's values permuted
// through csr.src, which becomes out->src; tiling_batch >= 0 replaces the owner's "tiling_batch" (option "s2b": the inner
// plan's images are the owner's times P); wgrad_options hands the owner's "wgrad_kernel", "wgrad_channel_block", "wgrad_pointwise" and
// "wgrad_pointwise_tile_entries" down too
// (option "b2s": the inner plan computes the weight gradient).  A failure returns the failed call's code; the caller drops *out with its state.
int build_derived_plan(const escoin_plan *owner, const escoin_conv_desc &desc, int kernel, int backward_kernel,
                       DerivedCsr csr, hipStream_t stream, DerivedPlan *out, int tiling_batch = -1, bool wgrad_options = false);
// escoin_capi.hip: the first half of set_csr -- validates a CSR (flat, as escoin_plan_set_csr takes it) and copies it into
// the plan's host vectors; a refused CSR leaves the plan as it was.  T = float | double.
template <typename T>
int set_csr_host(escoin_plan *p, const int *rowptr, const int *colidx, const T *values, const int *nnz_per_group);
// escoin_capi.hip: brings the host mirrors (CSR values, the kept copy of the generated code, the transposed plan's) up
// to date after device-source updates -- through escoin_plan::sync_host_fn, which the update that made the device
// authoritative left (the host-only translation units do not depend on update_values.hip); a no-op otherwise.  Waits
// for the update's stream.
int sync_host_values(escoin_plan *p);
long upd_stat(const escoin_plan *p, const char *key);
// update_values.hip, for solver_step.hip.  solver_begin: the checks of a device-source update (`name` for the messages),
// update_count, and the update state with its entry-major view, built if need be; t->nnz == 0: nothing to launch.
// solver_end, after the kernel is in `stream`: the device becomes authoritative, or (no in-place path) the plan is
// rebuilt from its value array.  T = float | double.
template <typename T> int solver_begin(escoin_plan *p, const char *name, hipStream_t stream, SolverTargets *t);
template <typename T> int solver_end(escoin_plan *p, const SolverTargets &t, hipStream_t stream);
// the plan's host CSR as the table builders read it (csr_tables.h), and its total nonzeros
inline CsrView csr_view(const escoin_plan *p) { return CsrView{&p->g, &p->rowptr, &p->colidx}; }
inline long plan_nnz(const escoin_plan *p) { return csr_view(p).nnz(); }
// whether group `grp` of the plan runs on the dense kernel (its units in the stream / generated code are empty)
inline bool group_is_dense(const escoin_plan *p, int grp) {
  return p->n_dense_groups > 0 && (grp >= 64 || ((p->dense_mask >> grp) & 1ull));
}
// sconv_backward.hip builds the backward state; escoin_capi.hip answers its "bwd_*" stats
long bwd_stat(const escoin_plan *p, const char *key);

// sconv_tiled.hip
int tiled_device_cus();             // compute units of the current device
bool tiled_supported(const Geometry &g);   // align_rules.h's, for the current device
int tiled_build(escoin_plan *p, hipStream_t stream, bool jit);  // fills p->tiled, uploads streams / loads generated code
void tiled_release(escoin_plan *p);   // resets p->tiled_dev and p->tiled
// The fast half of escoin_plan_import_aligned: a generated-code plan restored from what
// escoin_plan_export_aligned wrote (tiling, channel deal, unit table, code object) -- no channel
// deal, no generator pass, no assembler.  `blob` is the code section of the persisted form, whose bytes
// aligned_form.h writes and parses; these two do the device side around it.
int tiled_export(const escoin_plan *p, std::vector<char> *out);
int tiled_import(escoin_plan *p, const char *blob, size_t bytes, hipStream_t stream);
int launch_tiled(const escoin_plan *p, const float *bottom, const float *bias, float *top,
                 int n_images, hipStream_t stream);
// what launch_tiled would refuse for the call's sizes, before anything is launched (a plan that also has dense groups)
int tiled_precheck(const escoin_plan *p, int n_images);
const char *tiled_kernel_name(const escoin_plan *p);

// sconv_lowered.hip (conv_mode LOWERED_SPARSE: im2col + CSR x dense, the lowering baseline)
int launch_lowered(escoin_plan *p, const float *bottom, const float *bias, float *top, int n_images,
                   hipStream_t stream);
int csrmm(int M, int N, int K, float alpha, const float *vals, const int *rowptr, const int *colidx,
          const float *B, float beta, float *C, hipStream_t stream);
int csrmm_f64(int M, int N, int K, double alpha, const double *vals, const int *rowptr, const int *colidx,
              const double *B, double beta, double *C, hipStream_t stream);
const char *lowered_kernel_name();

// dense_mfma.hip
int launch_dense(const escoin_plan *p, const float *bottom, const float *bias, float *top,
                 int n_images, hipStream_t stream);
const char *dense_kernel_name();
int dense_build_ktab(escoin_plan *p, hipStream_t stream);
int dense_lda(int K);          // floats per row of d_dense_w (K rounded up to whole k-steps)
int dense_spare_rows();       // zero rows after row M - 1

// wgrad_mfma.hip (option "wgrad_kernel" = MFMA): builds the kernel's tables for the tile plan bwd_choice made; stage 1 of
// the weight gradient of the plan's nnz entries over `chunks` chunks of n_images images into slab_w [chunks][nnz]
int wgm_build(const escoin_plan *p, const WgmPlan &wp, WgmState *w, hipStream_t stream);
int launch_wgrad_mfma(const escoin_plan *p, const WgmState &w, long nnz, const float *bottom, const float *top,
                      const float *top_diff, float *slab_w, int n_images, int chunks, hipStream_t stream);

// wgrad_pointwise.hip (option "wgrad_pointwise"): plans the tiles on the plan's CSR with the options bwd_choice read, and
// builds the kernel's tables; stage 1 of the weight and / or bias gradient (slab_w null: the bias alone, slab_b likewise)
// over `chunks` chunks of n_images images into slab_w [chunks][nnz] and slab_b [chunks][M]
int pw_build(const escoin_plan *p, const BwdOptions &o, PwWgrad *w, hipStream_t stream);
int launch_wgrad_pointwise(const escoin_plan *p, const PwWgrad &w, long nnz, const float *bottom, const float *top,
                           const float *top_diff, float *slab_w, float *slab_b, int n_images, int chunks, hipStream_t stream);

// dgrad_mfma.hip (option "backward_kernel" = ESCOIN_BWD_MFMA): builds the phase matrices and the kernel's tables for the
// tile plan bwd_choice made; the data gradient of n_images images
int dgm_build(const escoin_plan *p, const DgmPlan &dp, DgmState *m, hipStream_t stream);
int launch_dgrad_mfma(const escoin_plan *p, const DgmState &m, const float *top, const float *top_diff,
                      float *bottom_diff, int n_images, hipStream_t stream);

// s2d.hip (option "s2d"): X' of the first n_images images from the bottom blob (pack), bottom_diff of the first n_images
// images from dX' (unpack), and the pack kernel's name.  s2d.hip registers them when the library is loaded; the plan's core
// (escoin_capi.hip, sconv_backward.hip) calls through the table, like escoin_plan::sync_host_fn, so that a program linking
// the core's objects alone still links -- there the table is empty and option "s2d" is refused at the align.
struct S2dHooks {
  int (*pack)(const escoin_plan *p, const float *bottom, float *x, int n_images, hipStream_t stream);
  int (*unpack)(const escoin_plan *p, const float *dx, float *bottom_diff, int n_images, hipStream_t stream);
  const char *pack_kernel_name;
};
extern S2dHooks g_s2d_hooks;   // escoin_capi.hip

// s2b.hip (option "s2b"), registered like S2dHooks.  Each kernel serves both directions; `top_side` names the blob:
//   pack    false: X' from the bottom blob (offset = the pad); true: G' from top_diff (offset 0), times [mask > 0] where
//           mask (the top blob) is not null
//   unpack  false: bottom_diff from dX' (offset = the pad); true: the top blob from T' (offset 0), through ReLU if `relu`
// always of the first n_images images.
struct S2bHooks {
  int (*pack)(const escoin_plan *p, const float *src, const float *mask, float *dst, bool top_side, int n_images, hipStream_t stream);
  int (*unpack)(const escoin_plan *p, const float *src, float *dst, bool top_side, bool relu, int n_images, hipStream_t stream);
  const char *pack_kernel_name, *unpack_kernel_name;
};
extern S2bHooks g_s2b_hooks;   // escoin_capi.hip

// b2s.hip (option "b2s"), registered like S2dHooks.  Each kernel serves both sides; `top_side` names the blob (CH = M) or the
// bottom side (CH = C), and the buffers are the caller's:
//   pack    dst[n'][ch][j] = src[n' * B + j][ch] (mask > 0 ? that : 0 where mask, laid out as src, is not null), +0 past
//           n_images, for the ceil(n_images / B) inner images the first n_images images touch
//   unpack  dst[n][ch] = src[n / B][ch][n % B] for n < n_images, through ReLU if `relu`
struct B2sHooks {
  int (*pack)(const escoin_plan *p, const float *src, const float *mask, float *dst, bool top_side, int n_images, hipStream_t stream);
  int (*unpack)(const escoin_plan *p, const float *src, float *dst, bool top_side, bool relu, int n_images, hipStream_t stream);
  const char *pack_kernel_name, *unpack_kernel_name;
};
extern B2sHooks g_b2s_hooks;   // escoin_capi.hip

// d2s.hip (option "deconv"), registered like S2dHooks.  Of the first n_images images:
//   unpack      top from T' (+ bias[m] where bias is not null, through ReLU if `relu`): one store per top element
//   pack        G' from top_diff (times [mask > 0] where mask, the top blob, is not null), +0 outside OH x OW
//   carry       dst[idx[k]] += src[k] for k < n: the inner compact gradient into the outer entry order (idx = D2sState::src)
//               or into blobs_[0]'s layout (idx = D2sState::wpos); idx is injective
//   bias_sum    bias_diff[m] += the inner bias gradients of m's P phases, ascending
struct D2sHooks {
  int (*unpack)(const escoin_plan *p, const float *t, const float *bias, float *top, bool relu, int n_images, hipStream_t stream);
  int (*pack)(const escoin_plan *p, const float *top_diff, const float *mask, float *g, int n_images, hipStream_t stream);
  int (*carry)(const float *src, const int *idx, float *dst, long n, hipStream_t stream);
  int (*bias_sum)(const float *inner_bias_diff, float *bias_diff, int M, int P, hipStream_t stream);
  const char *unpack_kernel_name, *pack_kernel_name;
};
extern D2sHooks g_d2s_hooks;   // escoin_capi.hip
// The refusal of an entry point that option "deconv" does not carry yet (`who` names it); ESCOIN_OK on other plans.
inline int refuse_deconv(const escoin_plan *p, const char *who) {
  if (!p || !p->deconv) return ESCOIN_OK;
  return fail(ESCOIN_EINVAL, std::string(who) + ": not carried over to option \"deconv\" plans yet");
}

// escoin_capi.hip: what every align of an option "deconv" plan asks first -- whether d2s_plan serves the layer for this Dtype
// (the refusal is ESCOIN_EINVAL with the rule's message) and that no other derived-plan option is set; ESCOIN_OK on other plans
int deconv_precheck(const escoin_plan *p, bool is_f64);
// d2s_cpu.cpp: option "deconv" in CPU mode, behind escoin_forward_cpu / escoin_backward_cpu / escoin_backward_values_cpu;
// registered like S2dHooks, for the same reason (a program that links the core's objects alone refuses the option's CPU mode)
struct D2sCpuHooks {
  int (*forward)(escoin_plan *p, const float *bottom, const float *bias, float *top, int n_images, int n_threads);
  int (*backward)(escoin_plan *p, const float *bottom, const float *top, const float *top_diff, float *bottom_diff,
                  float *weight_diff, float *bias_diff, int n_images, int n_threads, bool compact);
};
extern D2sCpuHooks g_d2s_cpu_hooks;   // escoin_capi.hip

// Index of the k-th set bit of `mask` (k < popcount): blockIdx -> conv group when only some groups
// of a layer run in a launch.  Wave-uniform scalar code on the device.
__host__ __device__ inline int nth_set_bit(unsigned long long mask, int k) {
  for (; k > 0; --k) mask &= mask - 1;
  int i = 0;
  while (i < 63 && !((mask >> i) & 1ull)) ++i;
  return i;
}

}  // namespace escoin

#endif  // ESCOIN_PLAN_H_
