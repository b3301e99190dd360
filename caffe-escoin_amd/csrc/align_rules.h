// align_rules.h -- WeightAlign's decisions: which conv groups go to the dense kernel, which kernel and layout the sparse
// ones get, which data-gradient and weight-gradient kernels the backward runs or why it refuses (bwd_choice).  Pure C++
// (no HIP, no escoin_plan): every rule is a function of values -- geometry, nonzero counts, option values and the device's
// CU count -- so that it runs, and is tested, on a machine without a GPU (tests/test_align_rules.py,
// tests/test_bwd_choice.py).  The .hip files call these and do the device work: uploads, code loads, launches.
#ifndef ESCOIN_ALIGN_RULES_H_
#define ESCOIN_ALIGN_RULES_H_

#include <string>
#include <vector>

#include "geometry.h"
#include "jit_codegen.h"
#include "stream_builder.h"

namespace escoin {

constexpr int kTiledWaves = 8;
constexpr int kLdsBudget = 64 * 1024;   // per plane buffer; two buffers per workgroup

typedef std::vector<std::vector<int>> CsrIndex;     // [conv group][...]: rowptr / colidx of the host CSR
typedef std::vector<std::vector<float>> CsrValues;

// ---- dense / sparse split of the conv groups -----------------------------------------------------------------------
// The plan options the split reads (escoin_plan_set_option).
struct SplitOptions {
  int kernel, conv_mode, dense_gate, dense_threshold_pct, tiling_batch;
};
// One flag per conv group: 1 = the group runs on the dense (fp32 MFMA) kernel.
std::vector<char> dense_groups(const Geometry &g, const std::vector<long> &nnz_per_group, const SplitOptions &o, int n_cu);

// What the plan keeps of the flags: bit g of dense_mask = group g goes to the MFMA kernel, bit g of sparse_mask = to the
// sparse kernels (layers with more than 64 groups take one decision for all of them: both masks are then all-ones / zero).
struct GroupSplit {
  int n_dense = 0, n_sparse = 0;
  bool use_dense = false;         // every group dense
  unsigned long long dense_mask = 0, sparse_mask = ~0ull;
};
GroupSplit group_split(const std::vector<char> &dense);

// ---- the tiled kernels ---------------------------------------------------------------------------------------------
int default_lds_budget();
Tiling pick_tiling(const Geometry &g, int n_cu, int lds_budget = 0, float density = 0.f, int tiling_batch = 0,
                   bool one_tile_ok = false, int waves_per_wg = 0);
bool tiled_supported(const Geometry &g, int n_cu);

// escoin_plan_tiling_info's line
std::string tiling_info(const Tiling &t, bool jit, int nbuf, size_t lds_bytes, int tab_len, bool chained);

// KERNEL_AUTO's rule for pointwise launches of one round of workgroups under 64 MFLOP, evaluated from the tiling before
// any code is generated or loaded: 0 not considered, 1 generated code, 2 the generic kernel.
int small_launch_rule(const Geometry &g, int kernel_choice, int n_dense_groups, int tiling_batch, long nnz, const Tiling &t,
                      bool chained, int n_cu);

// 5x5 / pad 2 reaches two columns past a row: the asm epilogue needs whatever lies there in the lane order to be a
// zero-filled quad (or masked elements of the row's own partial quad).
bool epi5_reach_ok(const Tiling &t);

// Which compiled body a launch of generated code runs (sconv_tiled.hip): 1 = the chained instantiation, 0 = the
// generic body.  The chained one serves plans whose code stages its own planes and runs a tile as one call, on
// launches whose epilogue is the asm one that stores from the accumulators: static padding (1x1 / 0, 3x3 / 1,
// 5x5 / 2), rows no longer than a DPP row whose edge lanes pull in zeros (3x3, 5x5; for 5x5 also epi5_reach_ok), a
// top blob under 2 GiB.  option: plan option "body_variant" (-1 this rule, 0 always generic).
struct BodyLaunch {
  bool jit = false, chained = false, dma_in_code = false;   // the plan: generated code, jit_chain, jit_dma
  int stage_bytes = 0;                                      // LDS-staged weight stream per wave (0 for generated code)
  bool strided = false;                                     // strided pointwise view
  int n_dense_groups = 0;                                   // conv groups on the MFMA kernel
  bool epi_store = false;                                   // the launch's top blob is under 2 GiB
  long workgroups = 0;                                      // grid.x * grid.y
};
int body_variant(const Geometry &g, const Tiling &t, const BodyLaunch &l, int option);

// One launch of a tiled plan (sconv_tiled.hip launch_tiled_once) over n_images images: the pixel tiles, the grid of
// persistent workgroups that walk them and whether the workgroup columns are grouped by XCD.  groups: the conv groups
// the launch covers (the sparse ones when others run on the MFMA kernel); jit / code_bytes: generated code and its size.
struct TiledLaunchShape {
  int tiles = 0;                 // pixel tiles; a workgroup walks tiles blockIdx.x, + grid_x, ...
  int grid_x = 0, grid_y = 0;    // grid_y = groups x workgroup columns (n_ocblk)
  int xcd_q = -1, xcd_r = 0;     // columns grouped by XCD: workgroups / 8 and % 8; xcd_q < 0: the launch order
  bool epi_store = false;        // the launch's top blob is under 2 GiB (the asm epilogues' 32-bit store offsets)
};
TiledLaunchShape tiled_launch_shape(const Geometry &g, const Tiling &t, int n_images, int groups, bool jit, long code_bytes,
                                    int n_cu);

// ---- the size limits a launch checks (include/escoin.h "Size limits") -----------------------------------------------
// What the .hip files refuse at launch time, as functions of sizes alone: tests/cpp/launch_limits_check.cpp holds each
// to its edge without a device.  A verdict is the refusal's code and message, ESCOIN_OK and "" where the launch may go.
struct LaunchVerdict {
  int rc = ESCOIN_OK;
  const char *error = "";
  bool ok() const { return rc == ESCOIN_OK; }
};
// A buffer descriptor's 32-bit byte offsets (the plane DMA of the tiled kernels, both operands of the dense kernel): a
// launch addresses fewer bytes than this.  The last 16 stay out of range: kOOB of sconv_tiled.hip is the offset of a
// quad that must read as zeros.
constexpr unsigned long long kDescriptorRange = 0xFFFFFFF0ull;
// The asm epilogues' 32-bit byte offsets into the top blob (voff + g * ostr): a launch's top lies below this.
constexpr unsigned long long kEpiStoreRange = 1ull << 31;
constexpr unsigned kGridYZMax = 65535u;    // a grid's y and z

// the asm epilogues may store this launch's top blob (TiledLaunchShape::epi_store)
constexpr bool epi_store_fits(unsigned long long top_bytes) { return top_bytes < kEpiStoreRange; }
// the most bytes of bottom one tiled launch covers: plan option "max_launch_bytes" (> 0) lowers the descriptor's range
constexpr unsigned long long tiled_launch_range(long max_launch_bytes) {
  return max_launch_bytes > 0 && (unsigned long long)max_launch_bytes < kDescriptorRange ? (unsigned long long)max_launch_bytes
                                                                                          : kDescriptorRange;
}
// launch_tiled's sub-batch: images per launch of a bottom of n_images x in_image_bytes under `range`, at least one
int tiled_chunk(int n_images, unsigned long long in_image_bytes, unsigned long long range);
// ... and the launches that makes
constexpr long tiled_launches(int n_images, int chunk) { return ((long)n_images + chunk - 1) / chunk; }
// tiled: one image at or above the range
LaunchVerdict tiled_image_limit(unsigned long long in_image_bytes, unsigned long long range);
// tiled: a strided pointwise launch (always the asm epilogue) with a top of kEpiStoreRange bytes or more
LaunchVerdict tiled_strided_top_limit(bool strided, unsigned long long top_bytes);
// tiled: grid y
LaunchVerdict tiled_grid_limit(unsigned long grid_y);
// Everything launch_tiled refuses for sizes, for a call of n_images, in the order its launches would meet it: what a plan
// with dense and sparse conv groups asks BEFORE its dense half is launched (escoin_forward).  groups: the conv groups the
// tiled launches cover.
LaunchVerdict tiled_call_limits(const Geometry &g, const Tiling &t, int n_images, int groups, long max_launch_bytes);
// dense: N*OH*OW at or above 2^31
LaunchVerdict dense_pixels_limit(long pixels);
// dense: the bottom of the launch or the weight matrix at or above kDescriptorRange bytes
LaunchVerdict dense_bytes_limit(unsigned long long in_bytes, unsigned long long w_bytes);
// generic / lowered: grid y or z above kGridYZMax.  The message names the kernel.
enum GridKernel { kGridGeneric, kGridCsrmm, kGridCsrmmF64, kGridIm2col };
LaunchVerdict grid_yz_limit(GridKernel k, unsigned long grid_y, unsigned long grid_z);
// the generic kernel's grid: y = ceil(M / 4) (four waves per workgroup, one output channel each), z = the images
LaunchVerdict generic_call_limits(const Geometry &g, int n_images);

// ---- which workgroups touch generated code with whole lines (sconv_tiled.hip, plan option "code_touchers") ---------
// Every unit of generated code starts with n_pref loads that pull the NEXT unit's code towards the wave (jit_codegen.h):
// 64 lanes x 64 bytes each, so that the code is in the XCD's L2 when the instruction cache asks for it.  One workgroup
// per L2 achieves that; the others' touches return lines the L2 already holds, through the path the plane DMA uses.  The
// election leaves the instruction in place and changes the lane offset the compiled body hands it (v63): 64 x lane in a
// TOUCHER, 0 elsewhere -- all 64 lanes then read one dword, one line request, still counted by vmcnt.
//
// The workgroups that share code and L2 are those of one XCD and one grid row (grid y = conv group x workgroup column).
// Linear workgroup ids go round the eight XCDs, which is what the XCD grouping of tiled_launch_shape relies on too, so a
// workgroup's RANK in its set follows from its id alone (ids ascending = dispatch order):
//   grouped launches (xcd_q >= 0): XCD x runs the renumbered ids [start_x, start_x + count_x), k = id / 8 counts from
//     start_x and bx from the start of the row, so rank = min(k, bx);
//   launch order (xcd_q < 0): the row's ids of one residue modulo 8 are bx = bx0, bx0 + 8, ..., bx0 < 8: rank = bx / 8.
// A workgroup is a toucher when rank % T == 0: rank 0 of every set always is, T = 1 makes every workgroup one.
constexpr int kTouchXcds = 8;
constexpr int kTouchRuleStride = 8;         // what the rule answers wherever it elects (align_rules.cpp touch_election)
constexpr int kTouchMaxStride = 65535;      // ranks stay below a launch's grid x, which is below 2^16 workgroups
// rank % T == 0 without a division: q = floor(rank * mul / 2^32) with mul = floor(2^32 / T) + 1 is floor(rank / T) while
// rank * T < 2^32 (the multiplier is at most T / 2^32 too large per unit of rank).  T = 1 needs no test; its mul is 0.
constexpr unsigned touch_mul(int T) { return T >= 2 ? (unsigned)((1ull << 32) / (unsigned)T + 1) : 0u; }
constexpr int touch_rank(int xcd_q, int k, int bx) { return xcd_q >= 0 ? (k < bx ? k : bx) : bx >> 3; }
constexpr bool touch_elected(unsigned rank, unsigned T, unsigned mul) {
  return T <= 1u || rank == (unsigned)(((unsigned long long)rank * mul) >> 32) * T;
}
// (grid row, column in the row) of linear workgroup id `orig` -- the renumbering of tiled_body / chained_body -- and
// whether the workgroup is a toucher at stride T
struct TouchWorkgroup { int bx, by, xcd; bool toucher; };
TouchWorkgroup touch_workgroup(const TiledLaunchShape &s, int orig, int T);

// The stride T of a launch: 1 for stream plans, for plans without touches (n_pref = 0) and for grids of 2^16 columns or
// more, whatever the option says -- there is nothing to elect.  Otherwise option (plan option "code_touchers") k >= 1
// forces T = k (capped at kTouchMaxStride: then rank 0 alone) and 0 is the rule, a function of the device alone, never
// of a timing: kTouchRuleStride on eight XCDs, 1 on devices it does not take for that (CU counts below 64 or no multiple
// of 8).  What it ships and why it reads nothing of the launch: profiles/code_touch_election_mi355x.md.
int touch_election(const TiledLaunchShape &s, bool jit, int n_pref, int n_cu, int option);
// Line requests of a launch's code touches at stride T: every wave's first-unit touch plus the touches of each unit of
// each tile it walks, n_pref instructions each, 64 lines in a toucher and 1 elsewhere.  touchers: the touchers counted.
long touch_lines(const TiledLaunchShape &s, const Tiling &t, int n_pref, int T, long *touchers = nullptr);

// Generated code: the tiling, the plane buffers and the generator's options.  ok == false: the layer does not fit.
struct JitLayout {
  bool ok = false;
  Tiling t;
  int nbuf = 2;        // plane buffers
  int budget = 0;      // plane-buffer budget the tiling was chosen with
  int tab_len = 0;     // quad-table period of the code's own plane DMA (0: the kernel body stages the planes)
  jit::Options jopt;
};
JitLayout jit_layout(const Geometry &g, float density, int tiling_batch, int n_cu);
// Generates the layout's program, applies the code-touch rule (which may generate it again without touches:
// lay->jopt.prefetch says which one came out) and checks its size.  false: the code overflows or is too large.
bool jit_generate(const Geometry &g, float density, int tiling_batch, int n_cu, JitLayout *lay, const CsrIndex &rowptr,
                  const CsrIndex &colidx, const CsrValues &values, jit::Program *prog);

// The LDS-staged stream: the first (buffers, plane budget) whose stream fits the workgroup's LDS, with that stream.
struct StreamLayout {
  bool ok = false;
  Tiling t;
  int nbuf = 2, budget = 0, stage_bytes = 0;
  WeightStream ws;
};
StreamLayout stream_layout(const Geometry &g, float density, int tiling_batch, int n_cu, const CsrIndex &rowptr,
                           const CsrIndex &colidx, const CsrValues &values);

// ---- the staged weight-gradient kernel (sconv_backward.hip) --------------------------------------------------------
constexpr int kStgWaves = 8;                         // waves per workgroup
constexpr size_t kStgLdsBudget = 64 * 1024;          // two workgroups per CU
constexpr int kStgSmallInt = 1 << 21;                // div_small's range
constexpr int kStgBatch = 8;                         // entries per batched reduction; the walk reads its tap offsets one
                                                     // batch ahead, so their table is padded by two (csr_tables.h)

// The staged weight-gradient kernel's block plan (sconv_backward.hip header of that kernel): the LDS tile and the split
// of a conv group's input channels into staged blocks.  AUTO's rule and stg_build both read this one.
struct StgPlan {
  int rows_max = 0;   // padded rows of the tile: the longest chunk's span
  int cs = 0;         // floats per staged channel: rows_max * Wp
  int icb = 0;        // input channels per staged block
  int nblk = 0;       // blocks per conv group (grid z)
  int chunks = 0;     // chunks of the full batch
  int osplit = 1;     // workgroups a conv group's output channels are dealt over
  size_t lds_bytes = 0;   // the tile: sizeof(float) * icb * cs
};
// Whether the staged kernel serves this plan, and its block plan where it does.
bool stg_plan(const Geometry &g, bool is_f64, int wgrad_channel_block, int n_cu, StgPlan *sp);
bool stg_auto_prefers(const Geometry &g, long nnz, const StgPlan &sp, int n_cu);

// ---- the fp32-MFMA weight-gradient kernel (wgrad_mfma.hip) ---------------------------------------------------------
// One workgroup of four waves per (chunk, tile of kWgmTileM output channels of a conv group, tile of kWgmTileK columns
// of the group's weight matrix); the chunk's pixels go through LDS kWgmStepPixels at a time, double buffered.
constexpr int kWgmTileM = 64, kWgmTileK = 64;
constexpr int kWgmStepPixels = 32;                   // pixels per LDS step: 16 k-steps of v_mfma_f32_32x32x2_f32
constexpr int kWgmLdsRow = kWgmTileM + 1;            // floats per staged pixel row (odd: spreads stores and reads over the banks)
static_assert(kWgmTileM == kWgmTileK, "the G and the bottom tile share one row length");
constexpr size_t kWgmLdsBytes = sizeof(float) * 2 * 2 * kWgmStepPixels * kWgmLdsRow;   // 2 buffers x (G tile, bottom tile)
constexpr size_t kWgmLdsBudget = 64 * 1024;          // what the kernel is compiled for: two workgroups per CU at least
static_assert(kWgmLdsBytes <= kWgmLdsBudget, "the MFMA weight-gradient tiles exceed their LDS budget");

struct WgmPlan {
  int tile_m = kWgmTileM, tile_k = kWgmTileK;
  int mtiles = 0, ktiles = 0;     // tiles per conv group along the output channels / the columns
  int kpad = 0;                   // columns rounded up to whole tiles: the length of the kernel's ktab
  int chunks = 0;                 // chunks of the full batch
  size_t lds_bytes = 0;
};
// Whether the MFMA weight-gradient kernel serves this plan, and its tile plan where it does: float plans of any stride,
// pad, dilation, group count and kernel shape whose indices fit the kernel's 32-bit arithmetic (N*OH*OW, M*Cg*KH*KW and
// Cg*H*W below 2^31; H, W, the pads and the dilated kernel extent below 2^28; at most 65535 (group, M-tile) pairs and
// column tiles: the grid).
bool wgm_plan(const Geometry &g, bool is_f64, WgmPlan *wp);

// ---- the pointwise weight-gradient kernel (wgrad_pointwise.hip, plan option "wgrad_pointwise") ------------------------
// The sampled product dW[m][c] = sum over pixels of G[m][q] * X[c][q] for the CSR's (m, c) pairs of a 1x1, pad-0 layer.
// One workgroup of kPwThreads lanes per (tile, chunk).  A tile is rows [row0, row0 + rows) of one conv group crossed with
// its channels [c0, c0 + chans); the chunk's pixels go through LDS kPwStepPixels at a time, one row of kPwPitch floats per
// output channel and per input channel of the tile, and a lane owns up to E of the tile's entries, each one fma chain.
constexpr int kPwThreads = 256;
constexpr int kPwStepPixels = 32;                    // S: pixels per LDS step
constexpr int kPwPitch = kPwStepPixels + 4;          // floats per staged row: rows 16-byte aligned, 4 banks apart
constexpr int kPwMaxLaneEntries = 16;                // E is 1, 2, 4, 8 or 16
constexpr int kPwMaxTileEntries = kPwThreads * kPwMaxLaneEntries;
constexpr size_t kPwLdsBudget = 64 * 1024;           // two workgroups per CU
constexpr int kPwMaxLdsRows = (int)(kPwLdsBudget / (sizeof(float) * kPwPitch));   // G rows + bottom rows of a tile
constexpr int kPwMaxChannelBlock = 256;              // channels of a tile under the rule
constexpr int kPwMaxSliceRows = kPwThreads;          // one lane per G row sums the bias
constexpr int kPwMinSliceRows = 8;                   // the rule splits slices no further than this for more workgroups
constexpr long kPwSplitWork = 1L << 16;              // ... and not at all below this many (entry, chunk) pairs: such a launch
                                                     // is a few microseconds of latency, which more workgroups do not shorten

struct PwTile {
  int grp = 0, row0 = 0, rows = 0;   // conv group, first group-local output channel, output channels
  int c0 = 0, chans = 0;             // first group-local input channel, input channels
  int items = 0;                     // entries of the pattern inside (with no pattern: the most any pattern has)
};
struct PwPlan {
  int step = kPwStepPixels, pitch = kPwPitch;
  int cblk = 0;               // channels per c-block: c-block b of a group covers channels [b * cblk, min(Cg, (b + 1) * cblk))
  int lane_entries = 1;       // E: the kernel instantiation, 256 * E >= the fullest tile
  int tile_cap = 0;           // the most entries a tile may hold
  int chunks = 0;             // chunks of the full batch (grid y)
  int rows_max = 0, chans_max = 0;   // the tallest m-slice, the widest c-block
  size_t lds_bytes = 0;       // sizeof(float) * pitch * (rows_max + chans_max)
  int bias_tiles = 0;         // the tiles of c-block 0, which come first and cover every row of every group once: they sum
                              // the bias, and a bias-only call launches them alone
  std::vector<PwTile> tiles;  // c-block-0 tiles (empty ones included), then the other c-blocks' tiles that hold an entry
};
// Whether the pointwise kernel serves this plan, and its tiling where it does.  Served: float plans with KH = KW = 1 and
// pad 0, any stride and group count, with N*OH*OW, C*H*W and nnz below 2^31 and at most 65535 chunks (grid y; the tiles
// are grid x).  The predicate reads no pattern.  The tiling reads the pattern (rowptr / colidx: the host CSR per conv
// group; both null: every row is taken as full, which bounds every pattern):
//   cblk      min(Cg, kPwMaxChannelBlock, the cap), and min(that, wgrad_channel_block) where the option is > 0;
//   m-slices  per (group, c-block), greedy over the rows: a slice closes before the row that would bring it past the cap
//             (tile_entries > 0: min(tile_entries, kPwMaxTileEntries); else kPwMaxTileEntries) or past the slice height
//             min(Mg, kPwMaxSliceRows, kPwMaxLdsRows - cblk).  A row holds at most cblk <= cap entries of a c-block, so
//             every tile is within the cap.  Past c-block 0, rows without an entry at a slice's ends are left out;
//   height    halved, down to kPwMinSliceRows, while chunks * tiles stays below two workgroups per CU -- on plans of at
//             least kPwSplitWork (entry, chunk) pairs.
// Every entry is in exactly one tile; an empty pattern has its c-block-0 tiles only.  No result's bits depend on the
// tiling: an entry's sum is one lane's chain over the chunk's pixels.
bool pw_plan(const Geometry &g, bool is_f64, long nnz, const CsrIndex *rowptr, const CsrIndex *colidx, int wgrad_channel_block,
             int tile_entries, int n_cu, PwPlan *pp);

// ---- the dense weight gradient on the matrix cores (dense_wgrad.hip) ------------------------------------------------
// wgm_plan's predicate and tiles; the pixel axis is split over `splits` workgroups per tile, each walking `span` whole
// chunks with one accumulator set, so that a layer with few tiles still fills the device.  With tiles = group * mtiles *
// ktiles and resident = kDwgResidentPerCu * n_cu workgroups on the device at once (four per CU: what the kernel's 70
// VGPRs + 16 AGPRs and 33 KB of LDS allow), a split into S = ceil(chunks / span) spans costs
//     max(1, (r + ceil(r)) / 2) * span       r = tiles * S / resident rounds of resident workgroups (a partly filled last
//                                            round counts half of what it leaves empty: its workgroups start as slots
//                                            free up) x the chunks each workgroup walks
//   + S / kDwgSplitsPerChunkCost             the sum kernel's serial walk over the splits,
// in integer arithmetic (rounds in 1/1024, floor), and the plan takes the cheapest span (ties: the fewest splits) among
// those with S <= max_splits (when > 0) and at most kDwgMaxRounds rounds -- or S = 1 where nothing else qualifies.  A
// model of the launch's shape, never a timing; what was tried on the MI355X is in profiles/grow_score_mi355x.md.  Split s covers chunks [s * span, min((s + 1) * span, chunks)):
// every chunk once, none of them empty.  The partial slab is splits x M*Cg*KH*KW floats: at most about kDwgMaxRounds *
// resident tiles of 16 KB, whatever the batch size.
constexpr int kDwgResidentPerCu = 4;
constexpr long kDwgMaxRounds = 4;
constexpr long kDwgSplitsPerChunkCost = 512;
struct DwgPlan {
  WgmPlan tile;              // tile.chunks = chunks of the full batch
  int span = 0;              // chunks per split
  int splits = 0;            // workgroups per tile at the full batch (grid x)
  long positions = 0;        // D = M * Cg * KH * KW
  size_t slab_bytes = 0;     // sizeof(float) * splits * positions
};
bool dwg_plan(const Geometry &g, bool is_f64, int n_cu, int max_splits, DwgPlan *dp);

// ---- the fp32-MFMA data-gradient kernel (dgrad_mfma.hip) -----------------------------------------------------------
// The bottom pixels split into stride_h x stride_w phases ((h + pad_h) % stride_h, (w + pad_w) % stride_w); inside a phase
// every pixel has the same contributing taps, so a phase is a stride-1 implicit GEMM.  One workgroup of four waves per
// (phase, tile of kDgmTileP phase pixels, (conv group, tile of kDgmTileC input channels)); the phase's columns (output
// channel, tap) go through LDS kDgmStepK at a time, double buffered.  The geometry is the weight-gradient kernel's.
constexpr int kDgmTileC = kWgmTileM, kDgmTileP = kWgmTileK;
constexpr int kDgmStepK = kWgmStepPixels;            // columns per LDS step: 16 k-steps of v_mfma_f32_32x32x2_f32
constexpr int kDgmLdsRow = kWgmLdsRow;               // floats per staged column (odd, as in the weight-gradient kernel)
constexpr size_t kDgmLdsBytes = sizeof(float) * 2 * 2 * kDgmStepK * kDgmLdsRow;   // 2 buffers x (weight block, G block)
constexpr size_t kDgmLdsBudget = 64 * 1024;
static_assert(kDgmLdsBytes <= kDgmLdsBudget, "the MFMA data-gradient tiles exceed their LDS budget");

// One phase: the bottom pixels (h0 + stride_h * hh, w0 + stride_w * ww), hh < rows, ww < cols, and its taps.
struct DgmPhase {
  int h0 = 0, w0 = 0, rows = 0, cols = 0;
  int taps_h = 0, taps_w = 0;     // kernel rows / columns with kr * dil_h % stride_h == the phase's row residue (columns likewise)
  int kp = 0;                     // Mg * taps_h * taps_w: the phase's columns
  int ksteps = 0;                 // kp in whole steps
  long tiles = 0;                 // pixel tiles of the full batch: ceil(N * rows * cols / kDgmTileP)
};
struct DgmPlan {
  int tile_c = kDgmTileC, tile_p = kDgmTileP, step_k = kDgmStepK;
  int phases_h = 0, phases_w = 0;       // = stride_h, stride_w; phase index = residue_h * phases_w + residue_w
  int ctiles = 0;                       // channel tiles per conv group
  long tiles_max = 0;                   // the longest phase's pixel tiles (grid x of the full batch)
  long cols_total = 0;                  // sum of ksteps * step_k over the phases: the length of the column decode table
  long mat_floats = 0;                  // the phase matrices: group * ctiles * tile_c * cols_total
  size_t lds_bytes = 0;
  std::vector<DgmPhase> phase;          // [phases_h * phases_w]
};
// Whether the MFMA data-gradient kernel serves this plan, and its tile plan where it does: float plans of any stride,
// pad, dilation, group count and kernel shape whose indices fit the kernel's 32-bit arithmetic (N*H*W, Mg*OH*OW and the
// phase matrices' floats below 2^31; H, W, the pads and the dilated kernel extent below 2^28; at most 65535 phases and
// 65535 (group, channel tile) pairs: the grid's y and z; fewer than 2^31 (group, phase, channel tile) triples).
bool dgm_plan(const Geometry &g, bool is_f64, DgmPlan *dp);

// ---- the backward's kernels (sconv_backward.hip) -------------------------------------------------------------------
// Whether the data gradient can run as a stride-1 forward of top_diff with the transposed, flipped weights: float plans,
// stride 1, pad <= dilation * (kernel - 1), at most 32767 output channels per group (a plan's channel limit).
bool bwd_transposable(const Geometry &g, bool is_f64);
// The plan options the backward reads (escoin_plan_set_option), and s2d: the plan has an inner plan (option "s2d" or
// option "s2b" serves it: it has an S2dState or an S2bState).
// wgrad_pointwise: option "wgrad_pointwise"; pw_tile_entries: test option "wgrad_pointwise_tile_entries".
struct BwdOptions {
  int backward_kernel, wgrad_kernel, wgrad_channel_block;
  bool s2d;
  int wgrad_pointwise = 0, pw_tile_entries = 0;
};
// Who computes the data gradient: the inner plan of option "s2d" / "s2b" (AUTO, TILED, JIT and DENSE on such a plan; the inner
// plan refuses what it cannot serve), the transposed forward plan, the gather kernel, the MFMA kernel of dgrad_mfma.hip.
enum BwdDataPath { kBwdInner, kBwdTransposed, kBwdGather, kBwdMfma };
// What the first backward on an alignment builds, or why it builds nothing: rc != ESCOIN_OK is a refusal with its message
// (the first of the ladder's that applies).  stg / wgm / dgm are filled for the kernel that wgrad / data names.
struct BwdChoice {
  int rc = ESCOIN_OK;
  const char *error = "";
  BwdDataPath data = kBwdGather;
  int wgrad = ESCOIN_WGRAD_ENTRY;   // ESCOIN_WGRAD_ENTRY / STAGED / MFMA: what option "wgrad_kernel" resolves to, or
                                    // ESCOIN_WGRAD_POINTWISE: AUTO with option "wgrad_pointwise" on a plan pw_plan serves
  StgPlan stg;
  WgmPlan wgm;
  PwPlan pw;                        // (the tiling that bounds every pattern: the state's builder plans again on the CSR)
  DgmPlan dgm;
  int chunks_max = 0;               // chunks of the full batch: the slab's rows
};
BwdChoice bwd_choice(const Geometry &g, bool is_f64, long nnz, const BwdOptions &o, int n_cu);

// ---- strided layers on the stride-1 kernels via space-to-depth (s2d.hip, plan option "s2d") ------------------------
// A strided convolution is a stride-1 convolution of the padded bottom split into its stride_h x stride_w pixel phases,
// each phase a channel (include/escoin.h "Space-to-depth"): PH = min(stride_h, KH) x PW = min(stride_w, KW) phases own a
// tap; channel c' = (c * PH + ph) * PW + pw; tap (kr, kc) becomes tap (kr / stride_h, kc / stride_w) of phase
// (kr % stride_h, kc % stride_w); the inner image is H' x W' = (OH + KH' - 1) x (OW + KW' - 1), pad 0, stride 1.
// The pack / unpack kernels divide by constants of the launch (rows per plane, PH, the strides).  floor(n / d) for
// 0 <= n < 2^31 and d >= 1 as one multiplication (Granlund & Montgomery, "Division by invariant integers using
// multiplication", theorem 4.2 with N = 31): mul = floor(2^(31 + l) / d) + 1, l = ceil(log2 d), which fits 32 bits because
// d > 2^(l - 1); then floor(mul * n / 2^(31 + l)) = floor(n / d).
struct S2dDiv { unsigned mul, shift; };
constexpr S2dDiv s2d_div_make(unsigned d) {
  unsigned l = 0;
  while ((1ull << l) < d) ++l;
  return S2dDiv{(unsigned)((1ull << (31 + l)) / d + 1), 31 + l};
}
constexpr unsigned s2d_div(unsigned n, S2dDiv f) { return (unsigned)(((unsigned long long)f.mul * n) >> f.shift); }
// log2 of the lanes a row of `span` elements gets: the smallest power of two that covers it, a wave at most
constexpr unsigned s2d_lane_shift(unsigned span) {
  unsigned k = 0;
  while (k < 6 && (1u << k) < span) ++k;
  return k;
}
struct S2dPlan {
  int PH = 0, PW = 0;             // phases that own at least one tap
  escoin_conv_desc inner = {};    // the inner plan's descriptor
  long x_floats = 0;              // N * C' * H' * W': the rearranged bottom X' (and its gradient dX')
};
// Whether option "s2d" serves this plan, and the inner descriptor where it does: float plans with a stride above 1 in at
// least one axis and dilation 1, whose bottom, X' and inner weight matrix (N*C*H*W, N*C'*H'*W', M*Cg'*KH'*KW') stay below
// 2^31 elements (the pack / unpack kernels' 32-bit offsets; every workgroup count is below them), whose padded extents
// (H + 2 pad_h, W + 2 pad_w) stay below 2^28 and whose Cg' is a channel count a plan accepts (at most 32767).
bool s2d_plan(const Geometry &g, bool is_f64, S2dPlan *sp);

// ---- dilated layers on the stride-1 kernels via space-to-batch (s2b.hip, plan option "s2b") -------------------------
// A dilated stride-1 convolution is eh x ew independent undilated convolutions: output pixel (oh, ow) reads only padded
// input pixels of its own residue class modulo (eh, ew), eh = dil_h where KH > 1 (else 1), ew likewise (include/escoin.h
// "Space-to-batch").  Each class is an IMAGE of the inner plan: n' = (n * eh + qh) * ew + qw, an H' x W' =
// ceil((H + 2 pad_h) / eh) x ceil((W + 2 pad_w) / ew) image, pad 0, stride 1, dilation 1, no ReLU; the CSR is the outer one.
struct S2bPlan {
  int eh = 0, ew = 0;             // residue classes per axis; P = eh * ew inner images per outer image
  escoin_conv_desc inner = {};    // the inner plan's descriptor (N' = N * P)
  long x_floats = 0;              // N' * C * H' * W': the rearranged bottom X' (and its gradient dX')
  long t_floats = 0;              // N' * M * OH' * OW': the inner top T' (and the rearranged top_diff G')
};
// The most inner images option "s2b" builds a plan for: the generic kernel's grid z and the backward's (bwd_choice refuses
// N > 65535) are the image index.
constexpr long kS2bMaxInnerImages = 65535;
// Whether option "s2b" serves this plan, and the inner descriptor where it does: float plans with stride 1 in both axes
// and P = eh * ew > 1, whose bottom, top, X' and T' each stay below 2^31 elements (the pack / unpack kernels' 32-bit
// offsets; every row and workgroup count is below them), whose padded extents and dilations stay below 2^28 and whose
// N * P is at most kS2bMaxInnerImages.
bool s2b_plan(const Geometry &g, bool is_f64, S2bPlan *sp);

// ---- inner-product layers on the pointwise kernels via batch-to-space (b2s.hip, plan option "b2s") ------------------
// An inner product is a 1x1 convolution of N images of one pixel; with the batch as the pixel axis it is a pointwise layer
// of N' = ceil(N / B) images of 1 x B pixels (include/escoin.h "Batch-to-space"): X'[n'][c][j] = bottom[n' * B + j][c], +0
// past the batch; pad 0, stride 1, dilation 1, no ReLU; the CSR is the outer one.
struct B2sPlan {
  int B = 0;                      // batch positions per inner image: a multiple of 4 in 4..256
  escoin_conv_desc inner = {};    // the inner plan's descriptor (N' = ceil(N / B) images of 1 x B)
  long x_floats = 0;              // N' * C * B: the transposed bottom X' (and, in a scratch of its own, its gradient dX')
  long t_floats = 0;              // N' * M * B: the inner top T' (and the transposed top_diff G')
};
constexpr int kB2sMinBlock = 4, kB2sMaxBlock = 256;
// Whether option "b2s" serves this plan, and the block and the inner descriptor where it does: float plans with H = W = 1,
// KH = KW = 1 and pad 0 (with one pixel and one tap, stride and dilation are immaterial), whose bottom, top, X' and T' each
// stay below 2^31 elements (the pack / unpack kernels' 32-bit offsets) and whose N' is at most kS2bMaxInnerImages.
// `block` forces B (option "b2s_block": a multiple of 4 in 4..256, which the caller has checked); 0 is the rule: B = 64,
// the block that won or tied the sweep {64, 128, 256} on every benched layer at batch 256 and 32 (profiles/b2s_mi355x.md:
// of the three it pads the batch least and gives the most inner images, so the most workgroups; at batch 32 a row of 64
// half full beat a full row of 32) -- and where 64 gives more than kS2bMaxInnerImages, the smaller of 128 and 256 that
// does not.  n_cu is the device's compute units, which the shipped rule does not weigh.
bool b2s_plan(const Geometry &g, bool is_f64, int block, int n_cu, B2sPlan *bp);

// ---- Deconvolution layers on the stride-1 kernels via depth-to-space (d2s.hip, plan option "deconv") ----------------
// A stride-(sh, sw) deconvolution is a stride-1 convolution of the bottom itself with P = sh * sw times the output
// channels, one per output phase, followed by a depth-to-space interleave (include/escoin.h "Deconvolution"): inner
// channel m' = (m * sh + ph) * sw + pw, kernel KH' x KW' = ceil(KH / sh) x ceil(KW / sw), pad (KH' - 1, KW' - 1), so the
// inner top is H' x W' = (H + KH' - 1) x (W + KW' - 1); top[m][oh][ow] = T'[m'(m, hp % sh, wp % sw)][hp / sh][wp / sw]
// with hp = oh + pad_h, wp = ow + pad_w.  All P phases are inner channels, those without a tap (sh > KH) included.
inline int deconv_out_dim(int in, int k, int pad, int stride) { return stride * (in - 1) + k - 2 * pad; }
struct D2sPlan {
  const char *error = "";         // why the option does not serve the layer ("" where it does)
  int OH = 0, OW = 0;             // the top image
  int sh = 0, sw = 0, P = 0;      // the strides and the phases per output channel
  escoin_conv_desc inner = {};    // the inner plan's descriptor
  escoin_conv_desc mirror = {};   // the convolution whose backward this layer is (M <-> C, H x W <-> OH x OW): the
                                  // geometry of the layer's weight matrix, rows = the bottom's channels
  long t_floats = 0;              // N * M * P * H' * W': the inner top T' (and the rearranged top_diff G', in the same scratch)
  long top_floats = 0;            // N * M * OH * OW
  // the launches of the full batch: unpack walks the top's rows (N * M * OH of OW elements), pack the rows of G'
  // (N * M * P * H' of W' elements); each below 2^31 with the blobs they index
  long unpack_rows = 0, pack_rows = 0;
};
// The most inner output channels M * P: the generic kernel's grid takes four channels per block of an axis of 65535.
constexpr long kD2sMaxInnerChannels = 4L * 65535;
// Whether option "deconv" serves the layer `d` describes (read as Caffe's DeconvolutionLayer), and the plan where it does;
// where not, dp->error names the reason: a double plan, a dilation other than 1, an empty top, top / T' / the inner weight
// matrix (M * P * Cg * KH' * KW') at or above 2^31 elements, more than kD2sMaxInnerChannels inner channels, more than 32767
// output channels per group (the mirror convolution's input channels).
bool d2s_plan(const escoin_conv_desc &d, bool is_f64, D2sPlan *dp);

}  // namespace escoin
#endif  // ESCOIN_ALIGN_RULES_H_
