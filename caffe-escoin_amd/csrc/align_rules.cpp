// align_rules.cpp -- WeightAlign's decisions as functions of values (align_rules.h).  No HIP, no device, no plan.
#include "align_rules.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "knobs.h"

namespace escoin {

// Density above which KERNEL_AUTO sends a conv group to the dense fp32-MFMA kernel: the measured
// crossover between the tiled sparse kernel and the dense kernel (profiles/r02_crossover.md).
constexpr int kDefaultDenseThresholdPct = 50;
constexpr int kGenericDenseThresholdPct = 4;

// ---- which conv groups go to the dense (fp32 MFMA) kernel -------------------------------
//  * kernel DENSE or conv_mode LOWERED_GEMM (forward_gpu_gemm, base_conv_layer.cpp:713-746): all;
//  * dense_gate = 1: the reference's gate -- group 0's density decides for the whole layer
//    (nz_num_[0] / (M/g * kernel_dim) > 0.2, base_conv_layer.cpp:750, :805; quirk 5);
//  * otherwise (AUTO): each group by its own density against the measured crossover
//    (profiles/r02_crossover.md; option "dense_threshold_pct" overrides).
std::vector<char> dense_groups(const Geometry &g, const std::vector<long> &nnz_per_group, const SplitOptions &o, int n_cu) {
  const int G = g.d.group;
  std::vector<char> dense(G, 0);
  const double per_group = (double)g.Mg * g.kdim;
  long nnz = 0;
  for (long n_g : nnz_per_group) nnz += n_g;
  if (o.kernel == ESCOIN_KERNEL_DENSE || o.conv_mode == ESCOIN_CONV_MODE_LOWERED_GEMM) {
    dense.assign(G, 1);
  } else if (o.kernel == ESCOIN_KERNEL_AUTO) {
    if (o.dense_gate) {
      if ((double)nnz_per_group[0] / per_group > 0.2) dense.assign(G, 1);
    } else {
      // a geometry the tiled kernels do not cover (stride / dilation != 1) has only the generic kernel on
      // the sparse side -- one lane per output pixel, ~2 sparse TFLOP/s -- against 65-110 dense TFLOP/s:
      // the MFMA kernel wins from ~4 % density on (ResNet-50's stride-2 1x1 layers pruned @90 %:
      // 2.2-2.7 ms generic vs 0.17-0.58 ms dense, profiles/r04_chain_prune_1x1.md)
      const bool fast_sparse = tiled_supported(g, n_cu);
      const int auto_thr = fast_sparse ? kDefaultDenseThresholdPct : kGenericDenseThresholdPct;
      const double thr = (o.dense_threshold_pct >= 0 ? o.dense_threshold_pct : auto_thr) / 100.0;
      // Above the cut the dense kernel used to win by rule.  With generated code on every sparse layer it
      // does not: measured crossovers (profiles/r04_crossover.md) sit between 53 % density (AlexNet conv3, whose
      // 507 output tiles fill the 512 MFMA slots exactly) and > 90 % (res2, 64 output channels: half-empty
      // 64 x 128 tiles) -- no single density separates them, what WeightAlign knows about the two kernels does:
      //   dense  = rounds of 128 x 128 (64 x 128 when a group has <= 64 channels) output tiles on 512 slots at
      //            120 TFLOP/s (x 0.7 for the narrow tiles), no faster than the blobs at 4.0 TB/s;
      //   sparse = 50 us + 2 * pixels * nonzeros at 80 TFLOP/s (3x3 / 5x5), 20 us + ... at 68 (1x1), no faster than
      //            the blobs at 4.8 TB/s.
      // Re-fitted in round 5 (profiles/r05_crossover.md; round 4's constants -- 25 us + 68 / 58 TFLOP/s against 110 --
      // were fitted to generated code that still moved a literal per nonzero, and on round 5's code sent res2 @10 %
      // sparsity to the dense kernel at 782 us against 588, res4 / res5 @20 % at 688 / 682 against 583 / 574).
      // Worst regret over the 14 shapes x 12 sparsities of the table: 7.7 % (round 4's constants on this table: 33 %;
      // a fixed 50 % cut: 42 %).  The model only ever decides ABOVE the cut; below it the sparse kernel always won, and
      // above 92 % density the dense one (an unpruned layer is never turned into megabytes of code).  An explicit
      // dense_threshold_pct option is obeyed as given.
      auto model_says_dense = [&](long nnz_g) {
        if ((double)nnz_g > 0.92 * per_group) return true;
        const double n = (double)(o.tiling_batch > 0 ? o.tiling_batch : g.d.N);
        const double pix = n * g.OH * g.OW;
        const int tm = g.Mg <= 64 ? 64 : 128;
        const double tiles = std::ceil((double)g.Mg / tm) * std::ceil(pix / 128.0);
        const double rounds = std::ceil(tiles / 512.0);
        const double byt = 4.0 * n * ((double)g.Cg * g.d.H * g.d.W + (double)g.Mg * g.OH * g.OW);
        const double t_dense = std::max(rounds * 2.0 * tm * 128.0 * g.kdim / (120e6 * (tm == 64 ? 0.7 : 1.0) / 512.0), byt / 4.0e6);
        const double t_sparse = std::max((g.d.KH * g.d.KW > 1 ? 50.0 : 20.0) + 2.0 * pix * (double)nnz_g / (g.d.KH * g.d.KW > 1 ? 80e6 : 68e6), byt / 4.8e6 + 8.0);
        return t_dense < t_sparse;
      };
      const bool use_model = o.dense_threshold_pct < 0 && fast_sparse;
      if (G <= 64) {
        for (int grp = 0; grp < G; ++grp) {
          const long n_g = nnz_per_group[grp];
          dense[grp] = (double)n_g / per_group > thr && (!use_model || model_says_dense(n_g));
        }
      } else if ((double)nnz / (per_group * G) > thr && (!use_model || model_says_dense(nnz / G))) {
        dense.assign(G, 1);
      }
    }
  }
  return dense;
}

GroupSplit group_split(const std::vector<char> &dense) {
  const int G = (int)dense.size();
  GroupSplit s;
  for (int grp = 0; grp < G; ++grp)
    if (dense[grp]) {
      ++s.n_dense;
      if (grp < 64) s.dense_mask |= 1ull << grp;
    }
  s.n_sparse = G - s.n_dense;
  s.use_dense = s.n_dense == G;
  if (s.use_dense) s.dense_mask = ~0ull;
  s.sparse_mask = s.n_dense == 0 ? ~0ull : ~s.dense_mask & (G >= 64 ? ~0ull : ((1ull << G) - 1));
  return s;
}

// Workgroup shape: 8 waves sharing one staged input tile, 64 KB of planes per buffer (measured
// best over {1,2,4,8} waves x {16,32,64} KB on the ResNet / AlexNet / GoogLeNet layer sets).
// (The weight stream stores LDS row offsets / 32 in 11-bit fields: a plane buffer may not exceed
// 64 KiB, whatever ESCOIN_LDS_KB says.)
int default_lds_budget() {
  static const int lds_kb = (int)ESC_KNOB("LDS_KB", kLdsBudget / 1024);
  return std::max(4, std::min(lds_kb, 64)) * 1024;
}

Tiling pick_tiling(const Geometry &g, int n_cu, int lds_budget, float density, int tiling_batch, bool one_tile_ok,
                   int waves_per_wg) {
  // tuning overrides for experiments: ESCOIN_WAVES (1,2,4,8), ESCOIN_LDS_KB
  static const int knob_waves = (int)ESC_KNOB("WAVES", kTiledWaves);
  const int waves = waves_per_wg > 0 ? waves_per_wg : knob_waves;
  ConvGeom c = to_geom(g);
  c.density = density;
  if (tiling_batch > 0) c.N = tiling_batch;   // plan option "tiling_batch": tile as for this batch
  return choose_tiling(c, waves, lds_budget > 0 ? lds_budget : default_lds_budget(), n_cu, one_tile_ok);
}

bool tiled_supported(const Geometry &g, int n_cu) {
  if ((g.d.stride_h != 1 || g.d.stride_w != 1 || g.d.dil_h != 1 || g.d.dil_w != 1) && !strided_pointwise(g)) return false;
  Tiling t = pick_tiling(g, n_cu);
  if (!t.ok) return false;
  return true;
}

std::string tiling_info(const Tiling &t, bool jit, int nbuf, size_t lds_bytes, int tab_len, bool chained) {
  char b[320];
  snprintf(b, sizeof(b), "%s cut=%dx%d S4=%d tpl=%d G=%d n_ocg=%d columns=%d oc_waves=%d pix_waves=%d tr=%d nseg=%d band=%d bands=%d "
           "qpc=%d icb=%d n_icb=%d nbuf=%d lds=%zu dma_in_code=%d period=%d chained=%d", jit ? "generated-code" : "stream", t.H, t.W, t.S4, t.tpl,
           t.G, t.n_ocg, t.n_ocblk, t.oc_waves, t.pix_waves, t.tr, t.nseg, (int)t.band_mode, t.bands, t.plane_ch_floats / 4, t.icb,
           t.n_icb, nbuf, lds_bytes, (int)(tab_len > 0), tab_len, (int)chained);
  return b;
}

// Small launches.  The LDS-tiled kernels walk a tile block by block, every block a round trip to HBM, on as many
// workgroups as the batch has tiles x columns: 11-19 us for one image of a GoogLeNet 1x1 layer; the generic kernel
// puts a lane on every output pixel of the whole chip and needs 7-12 (profiles/r04_batch_sweep.md -- the reference's
// SCONV mode calls the layer image by image, conv_layer.cu:16-26).  Round 4 TIMED both kernels; a layer's bits then
// depended on the box's noise (two ranks could settle differently).  Now a RULE decides, from what WeightAlign knows --
// the same weights, options and batch give the same kernel in every process on the same device model:
//   pointwise layers only (the 3x3 / 5x5 layers keep generated code at every batch: the generic kernel needs
//   16-81 us where code needs 12-16), a launch of one round (tiles x columns <= workgroup slots of the chip: CUs, or
//   2 x CUs for the half-workgroup tilings) under 64 MFLOP;
//   generic  ~ max(7.0, 5.8 + 0.125 r, 6.2 + waves x (0.143 + 0.0473 r) / 1000)   us; r = nonzeros per output row (the
//              CSR row a wave walks with scalar loads: a latency chain), waves = N x M x ceil(OH OW / 64)
//   code     ~ 7.6 + (0.6 chained | 1.1 one call per block) x blocks per tile + 0.1 x MB of blobs    us
//   the kernel with the lower estimate.
// Fitted to 180 cells (profiles/r05_small_launch_fit.md; tools/small_launch_fit.py: both kernels forced, 1-32 images
// of every distinct GoogLeNet 1x1 shape): the models are within 6 % (code) / 12 % (generic) rms of the measurements
// and the rule's pick is at most 12.7 % behind the faster kernel, two cells of 180 more than 10 %.
// Evaluated from the TILING, before any code is generated or loaded (round 6): a layer the rule sends to
// the generic kernel no longer pays for code generation and a module load / unload at every WeightAlign.
// Returns 0 (not considered), 1 (generated code), 2 (generic kernel).
int small_launch_rule(const Geometry &g, int kernel_choice, int n_dense_groups, int tiling_batch, long nnz, const Tiling &t,
                      bool chained, int n_cu) {
  if (!(kernel_choice == ESCOIN_KERNEL_AUTO && n_dense_groups == 0 && (tiling_batch <= 0 || tiling_batch == g.d.N) &&
        g.d.KH == 1 && g.d.KW == 1))
    return 0;
  const double flops = 2.0 * g.d.N * g.OH * g.OW * (double)nnz;
  const long tiles = t.band_mode ? (long)g.d.N * t.bands : ((long)g.d.N + t.nseg - 1) / t.nseg;
  const long wgs = tiles * t.n_ocblk * g.d.group;
  const long slots = (long)n_cu * (t.waves == 4 ? 2 : 1);
  if (!(flops < 64e6 && wgs <= slots)) return 0;
  const double r = (double)nnz / (double)g.d.M;
  const double waves = (double)g.d.N * g.d.M * std::ceil((double)g.OH * g.OW / 64.0);
  const double mb = 4.0 * g.d.N * ((double)g.d.C * g.d.H * g.d.W + (double)g.d.M * g.OH * g.OW) * 1e-6;
  const double t_gen = std::max(std::max(7.0, 5.8 + 0.125 * r), 6.2 + waves * (0.143 + 0.0473 * r) * 1e-3);
  const double t_code = 7.6 + (chained ? 0.6 : 1.1) * t.n_icb + 0.1 * mb;
  const int pick = t_gen < t_code ? 2 : 1;
  if (getenv("ESCOIN_VERBOSE"))
    fprintf(stderr, "[escoin] small launch (%.1f MFLOP, %ld workgroups on %ld slots, %d blocks): code ~%.1f us, generic ~%.1f us -> %s\n",
            flops * 1e-6, wgs, slots, t.n_icb, t_code, t_gen, pick == 2 ? "generic" : "code");
  return pick;
}

bool epi5_reach_ok(const Tiling &t) {
  const int r = t.W & 3, full = (t.W + 3) / 4;          // quads holding the row
  return (r == 1 || r == 2) || t.RS >= 4 * (full + 1) || (r == 0 && t.S4 == 16);
}

int body_variant(const Geometry &g, const Tiling &t, const BodyLaunch &l, int option) {
  if (option == 0) return 0;
  // the plan: what ChainPlan needs (jit_layout; an imported blob is checked again here)
  if (!(l.jit && l.chained && l.dma_in_code && l.stage_bytes == 0 && t.pix_waves == 1 && t.oc_waves == t.waves &&
        t.n_ocg % t.oc_waves == 0))
    return 0;
  if (!static_pad(g) || l.strided || l.n_dense_groups > 0 || !l.epi_store) return 0;
  // the body divides workgroup ids by grid.x and by the columns with a float reciprocal (exact below these bounds)
  if (l.workgroups >= (1l << 20) || t.n_ocblk >= 4096) return 0;
  if (g.d.KW != 1) {
    // in-place asm epilogue: the element a row-edge lane pulls in through DPP is a zero anyway (padding column, after
    // masking) or the row ends at a DPP row boundary
    const bool wide = t.S4 > 16;
    const bool fast_epi = !wide && (t.RS > t.W || t.S4 == 16);
    if (!fast_epi) return 0;
    if (g.d.KW == 5 && !epi5_reach_ok(t)) return 0;
  }
  return 1;
}

TiledLaunchShape tiled_launch_shape(const Geometry &g, const Tiling &t, int n_images, int groups, bool jit, long code_bytes,
                                    int n_cu) {
  TiledLaunchShape s;
  s.tiles = t.band_mode ? n_images * t.bands : (n_images + t.nseg - 1) / t.nseg;
  s.epi_store = epi_store_fits((unsigned long long)n_images * g.d.M * t.OH * t.OW * 4);
  // persistent workgroups: one 8-wave workgroup per CU is resident (2 waves/SIMD); each walks
  // its share of the pixel tiles so that prologue, first fill and epilogue overlap across tiles
  s.grid_y = groups * t.n_ocblk;
  const int wg_per_cu = std::max(1, 8 / t.waves);
  const int gx = std::max(1, (n_cu * wg_per_cu) / s.grid_y);
  s.grid_x = std::min(s.tiles, gx);
  // Workgroup columns grouped by XCD (sconv_tiled.hip tiled_body): for generated code of more than one column whose bytes
  // do not sit comfortably in an XCD's 4 MiB L2 beside the streaming input -- from 2 MB of code (round 4: 4 MB for
  // layers without conv groups; with the round-5 code res4 @90 %, 2.9 MB, gains 4 %: profiles/r05_knob_retune.md).  Measured, same-call pairs
  // (profiles/r04_xcd_map.md): the gain grows with the code -- below 2 MB none, 2-4 MB 2-12 %, above 5 MB
  // 17-31 % (AlexNet @80 % all on generated code 0.632 -> 0.524 ms per step; res5 @70 % 369 -> 281 us).  The
  // price: every XCD reads the input tiles of its own columns instead of sharing them through one L2 -- extra
  // L2 misses (served mostly by the Infinity Cache), which is why layers whose code fits keep the launch order
  // (res2-res4 @90 %: time within 1 % either way, 1.2-1.5x instead of 1.6-2.7x algorithmic bytes fetched).
  // The stream kernel has no code to keep apart and always keeps the launch order.
  // ESCOIN_XCD_MAP: 0 never, 1 wherever there is more than one column, unset: the rule above.
  static const int xm = (int)ESC_KNOB("XCD_MAP", -1);
  static const long min_code_env = ESC_KNOB_SET("XCD_MIN_CODE_KB") ? ESC_KNOB("XCD_MIN_CODE_KB", 0) * 1024 : -1;
  const long min_code = min_code_env >= 0 ? min_code_env : 2l << 20;
  const int nwg = s.grid_x * s.grid_y;
  const bool on = s.grid_y > 1 && nwg >= 8 && (xm == 1 || (xm < 0 && jit && code_bytes >= min_code));
  s.xcd_q = on ? nwg / 8 : -1;
  s.xcd_r = on ? nwg % 8 : 0;
  return s;
}

// ---- the size limits a launch checks ----------------------------------------------------------------------------------
static LaunchVerdict refuse_launch(int rc, const char *msg) {
  LaunchVerdict v;
  v.rc = rc;
  v.error = msg;
  return v;
}

int tiled_chunk(int n_images, unsigned long long in_image_bytes, unsigned long long range) {
  const unsigned long long fit = range > 16 && in_image_bytes > 0 ? (range - 16) / in_image_bytes : 0;
  return (int)std::max<unsigned long long>(1, std::min<unsigned long long>((unsigned long long)std::max(n_images, 0), fit));
}

LaunchVerdict tiled_image_limit(unsigned long long in_image_bytes, unsigned long long range) {
  if (in_image_bytes >= range) return refuse_launch(ESCOIN_EINVAL, "tiled kernel: one image exceeds the 4 GiB descriptor range");
  return LaunchVerdict();
}

LaunchVerdict tiled_strided_top_limit(bool strided, unsigned long long top_bytes) {
  if (strided && !epi_store_fits(top_bytes))
    return refuse_launch(ESCOIN_EINVAL, "tiled kernel: strided pointwise layer with a top blob of 2 GiB or more");
  return LaunchVerdict();
}

LaunchVerdict tiled_grid_limit(unsigned long grid_y) {
  if (grid_y > kGridYZMax) return refuse_launch(ESCOIN_EINVAL, "tiled kernel: grid.y exceeds 65535");
  return LaunchVerdict();
}

LaunchVerdict tiled_call_limits(const Geometry &g, const Tiling &t, int n_images, int groups, long max_launch_bytes) {
  const unsigned long long in_image = (unsigned long long)g.d.C * g.d.H * g.d.W * 4;
  const unsigned long long range = tiled_launch_range(max_launch_bytes);
  LaunchVerdict v = tiled_image_limit(in_image, range);
  if (!v.ok()) return v;
  // the first launch is the largest
  const int first = std::min(n_images, tiled_chunk(n_images, in_image, range));
  v = tiled_strided_top_limit(strided_pointwise(g), (unsigned long long)first * g.d.M * g.OH * g.OW * 4);
  if (!v.ok()) return v;
  return tiled_grid_limit((unsigned long)groups * (unsigned long)t.n_ocblk);
}

LaunchVerdict dense_pixels_limit(long pixels) {
  if (pixels >= (1l << 31)) return refuse_launch(ESCOIN_EINVAL, "dense kernel: N*OH*OW does not fit 31 bits");
  return LaunchVerdict();
}

LaunchVerdict dense_bytes_limit(unsigned long long in_bytes, unsigned long long w_bytes) {
  if (in_bytes >= kDescriptorRange || w_bytes >= kDescriptorRange)
    return refuse_launch(ESCOIN_EINVAL, "dense kernel: bottom blob or weight matrix exceeds the 4 GiB descriptor range");
  return LaunchVerdict();
}

LaunchVerdict grid_yz_limit(GridKernel k, unsigned long grid_y, unsigned long grid_z) {
  if (grid_y <= kGridYZMax && (grid_z <= kGridYZMax || k == kGridCsrmmF64)) return LaunchVerdict();
  switch (k) {
    case kGridGeneric: return refuse_launch(ESCOIN_EINVAL, "generic kernel: grid dimension exceeds 65535");
    case kGridCsrmm: return refuse_launch(ESCOIN_EINVAL, "csrmm: grid dimension exceeds 65535");
    case kGridCsrmmF64: return refuse_launch(ESCOIN_EINVAL, "csrmm_f64: more than 65535 rows");
    default: return refuse_launch(ESCOIN_EINVAL, "im2col: grid dimension exceeds 65535");
  }
}

LaunchVerdict generic_call_limits(const Geometry &g, int n_images) {
  return grid_yz_limit(kGridGeneric, ((unsigned long)g.d.M + 3) / 4, (unsigned long)std::max(n_images, 0));
}

TouchWorkgroup touch_workgroup(const TiledLaunchShape &s, int orig, int T) {
  TouchWorkgroup w;
  w.xcd = orig & (kTouchXcds - 1);
  const int k = orig >> 3;
  const int wg = s.xcd_q >= 0 ? w.xcd * s.xcd_q + std::min(w.xcd, s.xcd_r) + k : orig;
  w.by = wg / s.grid_x;
  w.bx = wg - w.by * s.grid_x;
  w.toucher = touch_elected((unsigned)touch_rank(s.xcd_q, k, w.bx), (unsigned)T, touch_mul(T));
  return w;
}

int touch_election(const TiledLaunchShape &s, bool jit, int n_pref, int n_cu, int option) {
  // nothing to elect, forced or not: no code or no touches, or ranks the multiplication of touch_elected does not cover
  if (!jit || n_pref <= 0 || s.grid_x >= (1 << 16) || s.grid_x < 1 || s.grid_y < 1) return 1;
  if (option >= 1) return std::min(option, kTouchMaxStride);
  // what the rule cannot describe: a device that is not eight XCDs of whole CUs
  if (n_cu < 64 || n_cu % kTouchXcds != 0) return 1;
  // Measured inside the bench step on the four ResNet-50 3x3 shapes at 90 % (profiles/code_touch_election_mi355x.md):
  // strides 4, 8 and 16 are not separable and 3 % under stride 1 on the step; one toucher per set (its peers then meet
  // code that is still on its way) puts res2, whose sets are the largest, above stride 1.  8 is the middle of the flat
  // range.  The sweep separated neither the code's bytes per grid row (0.19-1.44 MB) nor the tiles a workgroup walks
  // (1-7), so the rule reads neither.  Sets of up to 8 workgroups have their first member alone.
  return kTouchRuleStride;
}

long touch_lines(const TiledLaunchShape &s, const Tiling &t, int n_pref, int T, long *touchers) {
  long lines = 0, nt = 0;
  if (n_pref > 0 && s.grid_x > 0)
    for (int orig = 0; orig < s.grid_x * s.grid_y; ++orig) {
      const TouchWorkgroup w = touch_workgroup(s, orig, T);
      const long walked = w.bx < s.tiles ? (s.tiles - w.bx + s.grid_x - 1) / s.grid_x : 0;
      lines += (long)t.waves * n_pref * (1 + walked * t.n_icb) * (w.toucher ? 64 : 1);
      nt += w.toucher;
    }
  if (touchers) *touchers = nt;
  return lines;
}

// Generated code: nothing but the planes (and two small tables) lives in LDS -- the first tiling
// the budget allows is the one.  WeightAlign = tiling, channel deal, code generation, code
// object (jit_module.h), unit table.
JitLayout jit_layout(const Geometry &g, float density, int tiling_batch, int n_cu) {
  JitLayout lay;
  ConvGeom cg = to_geom(g);
  cg.density = density;
  // Plane buffers: two, or three of 48 KiB with TWO fills in flight (the unit of block k stages block
  // k + 2) for layers that wait for their planes rather than walk: pointwise layers at <= 10 % density
  // spend 15-50 % of a launch in the walk, and with one fill in flight the LDS-DMA engine of a CU idles
  // from the landing of one block to the first instruction of the next (barrier, issue, HBM latency:
  // 1.6 of 4.5 us per block on GoogLeNet's 28 x 28 layers).  ESCOIN_JIT_NBUF forces 2 or 3.
  static const int env_jit_nbuf = (int)ESC_KNOB("JIT_NBUF", 0);
  // Measured on GoogLeNet's 39 pointwise layers at 95 %, same-box bench steps (profiles/r03_nbuf_sweep.md):
  // with up to 192 output channels per conv group the third buffer wins (set -5 %; the 48 KiB budget
  // also steers 160-channel layers to one pass of 20 channels per wave instead of two of 10: -30 % on
  // those); 256 and 384 output channels walked long enough to cover one fill and lost 5-10 % to the
  // smaller blocks -- until their code stopped computing a tile B without rows (jit_codegen.cpp): since
  // then the third buffer wins there too (5b/1x1: 48.7 -> 44.3 us).
  int jit_nbuf = env_jit_nbuf == 2 || env_jit_nbuf == 3 ? env_jit_nbuf
                 : (g.d.KH == 1 && g.d.KW == 1 && density <= 0.101f && g.Mg <= 384) ? 3 : 2;
  int jit_budget = jit_nbuf == 3 ? std::min(default_lds_budget(), 48 * 1024) : default_lds_budget();
  Tiling t = pick_tiling(g, n_cu, jit_budget, density, tiling_batch, true);
  if (!t.ok) return lay;
  // 3x3 / 5x5 layers with more than one workgroup column: 32 KiB plane buffers instead of 64.  Since the units
  // chain themselves a block costs ~14 instructions and a barrier, not 1300 cycles of compiled code, and smaller
  // blocks start the first walk sooner and keep the fills finer under it: same-call pairs, ResNet step 1.953 ->
  // 1.902 ms (res3 -3.7 %, res4 -4.7 %, res5 -5.0 %), AlexNet 0.555 -> 0.531 ms (every layer -3..-6 %).  Not for
  // layers with ONE column (res2: +4.8 % -- its planes come from HBM, non-temporal, and need the longer blocks'
  // lead) and not for pointwise layers (GoogLeNet set +3.5 %: they wait for their planes, not for the walk).
  // ESCOIN_LDS_KB set: as it says.
  if (!ESC_KNOB_SET("LDS_KB") && g.d.KH * g.d.KW > 1 && t.n_ocblk > 1 && jit_nbuf == 2 && jit_budget > 32 * 1024) {
    const Tiling t32 = pick_tiling(g, n_cu, 32 * 1024, density, tiling_batch, true);
    if (t32.ok) {
      t = t32;
      jit_budget = 32 * 1024;
    }
  }
  if (jit_nbuf == 3 && t.n_icb < 2) {      // (the fill sequence may run one tile ahead only)
    jit_nbuf = 2;
    t = pick_tiling(g, n_cu, default_lds_budget(), density, tiling_batch, true);
    if (!t.ok) return lay;
  }
  static const int max_period = (int)ESC_KNOB("JIT_DMA_PERIOD", 2048);
  // Two 4-wave workgroups per CU instead of one of eight, for HBM-bound pointwise layers with two to four tiles per
  // workgroup (GoogLeNet's 28 x 28 layers with up to 96 output channels at batch 256).  A workgroup's life is
  // start-up, then per tile [stream the planes at the DMA engine's rate | epilogue: the stores, during which its
  // DMA queue runs dry], and with one workgroup per CU nothing runs under the ends (profiles/r05_pointwise_ends.md:
  // without the stores a 28 x 28 layer is 29 % shorter).  Two independent workgroups on a CU overlap by themselves:
  // one streams while the other stores or starts.  Same-call A/B, HBM-cold (profiles/r05_half_workgroups.md):
  // 192@28x28 -> 64 / 96 / 16 / 32 channels -11 / -9 / -10 / -12 %, 256@28x28 -> 32 / 64 -9 / -10 % -- within 2 % of
  // what a copy of the layer's bytes takes at 6.3 TB/s plus 8 us; 56 x 56 (seven tiles per workgroup: already at that
  // bound) +1 %, 14 x 14 and smaller (one tile per workgroup) 0..+50 %: not taken there; nor for 128 channels at
  // 28 x 28 as one column of four waves with one quad per lane (G = 32, four bands of 25 rows): 69 -> 79 us.  Needs every output
  // channel in ONE column of four waves (G <= 24: up to 96 channels), 32 KiB plane buffers x 2 so that two
  // workgroups share a CU's LDS, and at least one tile per workgroup.  ESCOIN_HALF_WG = 0 / 1: never / wherever it fits.
  {
    static const int half_knob = (int)ESC_KNOB("HALF_WG", -1);
    const long nb = tiling_batch > 0 ? tiling_batch : g.d.N;
    auto tiles_of = [&](const Tiling &tt) { return tt.band_mode ? nb * tt.bands : (nb + tt.nseg - 1) / tt.nseg; };
    const bool pointwise = g.d.KH == 1 && g.d.KW == 1 && g.d.pad_h == 0 && g.d.pad_w == 0 && !strided_pointwise(g) &&
                           g.d.group == 1;
    const bool rule = pointwise && t.n_ocblk == 1 && g.Mg <= 96 && tiles_of(t) >= 2l * n_cu && tiles_of(t) <= 4l * n_cu &&
                      !ESC_KNOB_SET("WAVES") && !ESC_KNOB_SET("LDS_KB") && env_jit_nbuf == 0;
    if (half_knob != 0 && pointwise && (rule || half_knob == 1)) {
      const Tiling t4 = pick_tiling(g, n_cu, 32 * 1024, density, tiling_batch, true, 4);
      if (t4.ok && t4.waves == 4 && t4.pix_waves == 1 && t4.n_ocblk == 1 && t4.n_ocg % t4.oc_waves == 0 && tiles_of(t4) >= 2l * n_cu) {
        int padded = 0;
        const int period = jit::dma_period(t4.plane_ch_floats / 4, max_period, 0.07, &padded);
        if (period > 0) {
          const Tiling tp = padded * 4 == t4.plane_ch_floats ? t4 : repad_planes(cg, t4, padded, 32 * 1024);
          if (tp.ok && lds_bytes_for(tp, 0, 2, period) <= kLdsPerWorkgroup / 2) {
            t = t4;
            jit_nbuf = 2;
            jit_budget = 32 * 1024;
          }
        }
      }
    }
  }
  jit::Options jopt = jit::options_from_env();
  // Plane DMA from inside the generated code: one wave per oc-group (the unit then knows which wave
  // runs it), a quad table of at most 2048 entries per tile parity; a plane may grow by up to 7 %
  // to get there (res5: 162 -> 168 quads, period 1344 instead of 5184; 28 x 28 pointwise: 98 -> 104).
  int tab_len = 0;
  if (t.pix_waves == 1 && (t.waves == 8 || t.waves == 4)) {
    int padded = 0;
    const int period = jit::dma_period(t.plane_ch_floats / 4, max_period, 0.07, &padded);
    if (period > 0) {
      const Tiling tp = padded * 4 == t.plane_ch_floats ? t : repad_planes(cg, t, padded, jit_budget);
      if (tp.ok && lds_bytes_for(tp, 0, jit_nbuf, period) <= kLdsPerWorkgroup && (jit_nbuf == 2 || tp.n_icb >= 2)) {
        t = tp;
        tab_len = period;
        jopt.dma.on = true;
        jopt.dma.qpc = padded;
        jopt.dma.period = period;
        jopt.dma.chan_bytes = (uint32_t)((size_t)g.d.H * g.d.W * 4);
        jopt.dma.waves = t.waves;
        jopt.dma.nt = t.n_ocblk == 1;
        jopt.dma.ahead = jit_nbuf - 1;
        // the pieces of the next block go out over ALL rows of a unit (an LDS-DMA instruction among
        // FMAs costs its wave 5-20 cycles, in a burst ~100), except where a tile has few blocks (res2:
        // three; the last pieces then land too close to the block top that needs them: 70 %).  Same-call
        // pairs, 100 against 70 % everywhere: GoogLeNet set -0.8 %, res3 / res4 / res5 -1.5 %, res2 +2.5 %.
        // (round 5, with the weights through the scalar cache the 3x3 / 5x5 rows are shorter: res3 at 70 % -3 %, res4
        // -1 %, res5 +1 % -- 70 % up to 16 blocks there; profiles/r05_knob_retune.md)
        jopt.dma.spread_pct = t.n_icb <= (g.d.KW != 1 ? 16 : 3) ? 70 : 100;
        if (ESC_KNOB_SET("JIT_DMA_SPREAD")) jopt.dma.spread_pct = std::max(1, std::min(100, (int)ESC_KNOB("JIT_DMA_SPREAD", 100)));
      }
    }
  }
  if (tab_len == 0 && jit_nbuf == 3) {     // two fills in flight only where the code stages its planes itself
    jit_nbuf = 2;
    t = pick_tiling(g, n_cu, default_lds_budget(), density, tiling_batch, true);
    if (!t.ok) return lay;
  }
  if (lds_bytes_for(t, 0, jit_nbuf, tab_len) > kLdsPerWorkgroup) return lay;
  // block-to-block chaining (jit_codegen.h ChainPlan): wherever the code stages its planes itself and
  // every wave of every workgroup column has an oc-group
  jopt.chain.on = tab_len > 0 && t.pix_waves == 1 && t.n_ocg % t.oc_waves == 0;
  jopt.chain.nbuf = jit_nbuf;
  jopt.chain.buf_bytes = (uint32_t)((t.planes_bytes + 1023) / 1024 * 1024 + 1024);
  // weights through the scalar cache instead of a literal move per nonzero: the 3x3 / 5x5 layers (their kernel
  // instantiations carry the longer clobber list, sconv_tiled.hip chain_call)
  jopt.sweights = g.d.KW != 1 ? 1 : 0;
  // s_setprio 1 / 0 alternating every four rows in the units of the first half of a workgroup's waves: the two
  // waves of a SIMD then take turns at the FMA pipe in bursts instead of interleaving instruction by instruction,
  // and the halves drift apart so that one half's row tops (LDS reads, the scalar loads) fall under the other's
  // FMAs.  Same-call pairs (profiles/r05_knob_retune.md): ResNet-50 set -0.5..-1.4 %, AlexNet -1.7 %, GoogLeNet -0.5 %.
  if (!ESC_KNOB_SET("JIT_PRIO_ROWS")) jopt.prio_rows = 4;
  if (!ESC_KNOB_SET("JIT_PRIO_WAVES")) jopt.prio_waves = t.waves / 2;
  lay.ok = true;
  lay.t = t;
  lay.nbuf = jit_nbuf;
  lay.budget = jit_budget;
  lay.tab_len = tab_len;
  lay.jopt = jopt;
  return lay;
}

bool jit_generate(const Geometry &g, float density, int tiling_batch, int n_cu, JitLayout *lay, const CsrIndex &rowptr,
                  const CsrIndex &colidx, const CsrValues &values, jit::Program *prog) {
  ConvGeom cg = to_geom(g);
  cg.density = density;
  const Tiling &t = lay->t;
  jit::Options &jopt = lay->jopt;
  *prog = jit::build_program(cg, t, rowptr, colidx, values, jopt);
  // Code touches (a unit loads the first bytes of the code that runs next, so that it is in the L2 by then) cost
  // every wave a load per unit and a wait; where ALL of a layer's code is small enough to stay in every XCD's L2
  // beside the streaming input, the first workgroups' instruction fetches do the same job.  Same-call pairs
  // (profiles/r05_knob_retune.md): without them GoogLeNet's 56 x 56 layer -3.8 %, its 14 x 14 layers -2..-8 %; the half-workgroup layers and the 4 x 4 ones (fewer tiles than CUs: too few
  // workgroups share the fetches) +1..+10 % (kept there), res3..res5 / AlexNet (megabytes of code) +7..+40 %, and res2 (168 KB) -2 % alone but +3 % together with the
  // s_setprio rows above: pointwise layers only.
  // ESCOIN_JIT_PREFETCH = 0 / 1 overrides (experiments flavour).
  const long nb = tiling_batch > 0 ? tiling_batch : g.d.N;
  const long tiles_total = t.band_mode ? nb * t.bands : (nb + t.nseg - 1) / t.nseg;
  if (jopt.prefetch && !ESC_KNOB_SET("JIT_PREFETCH") && !prog->overflow && g.d.KH == 1 && g.d.KW == 1 && t.waves == 8 &&
      t.n_icb >= 2 && prog->code.size() * 4 <= 256u * 1024u && tiles_total >= n_cu) {
    jopt.prefetch = 0;
    *prog = jit::build_program(cg, t, rowptr, colidx, values, jopt);
  }
  return !(prog->overflow || prog->code.size() * 4 > kMaxJitBytes);
}

StreamLayout stream_layout(const Geometry &g, float density, int tiling_batch, int n_cu, const CsrIndex &rowptr,
                           const CsrIndex &colidx, const CsrValues &values) {
  StreamLayout lay;
  ConvGeom cg = to_geom(g);
  cg.density = density;
  // Buffers.  Two plane/staging buffers overlap one block's DMA with the previous block's walk.
  // Three (two blocks in flight, counted vmcnt waits inside a tile; ESCOIN_NBUF=3) were measured
  // on the HBM-bound pointwise layers and on the ResNet set: 7-8 % SLOWER -- the smaller planes
  // mean more blocks, and a block's fixed costs (barrier, DMA issue, loop prologue) outweigh the
  // DMA latency the third buffer hides.
  static const int env_nbuf = (int)ESC_KNOB("NBUF", 0);
  for (int nbuf = env_nbuf == 3 ? 3 : 2; nbuf >= 2; --nbuf) {
    // the staging areas share the workgroup's LDS with the plane buffers: shrink the planes until
    // everything fits (the body size depends on the channels per block, so this is a short search)
    const int start = nbuf == 2 ? default_lds_budget() : std::min(default_lds_budget(), 48 * 1024);
    for (int budget = start; budget >= 16 * 1024; budget -= 4 * 1024) {
      const Tiling t = pick_tiling(g, n_cu, budget, density, tiling_batch);
      if (!t.ok) break;
      if (nbuf == 3 && t.n_icb < 2) break;          // the fill sequence may run one tile ahead only
      WeightStream ws = build_stream(cg, t, rowptr, colidx, values);
      if (ws.overflow) continue;
      const int stage = stage_bytes_for(ws.max_body_bytes);
      if (lds_bytes_for(t, stage, nbuf) > kLdsPerWorkgroup) continue;
      lay.ok = true;
      lay.t = t;
      lay.nbuf = nbuf;
      lay.budget = budget;
      lay.stage_bytes = stage;
      lay.ws = std::move(ws);
      return lay;
    }
  }
  return lay;   // not ok: the caller falls back to the generic kernel
}

bool stg_plan(const Geometry &g, bool is_f64, int wgrad_channel_block, int n_cu, StgPlan *sp) {
  const escoin_conv_desc &d = g.d;
  if (is_f64 || d.stride_h != 1 || d.stride_w != 1) return false;
  const long opix = (long)g.OH * g.OW;
  const long Hp = (long)d.H + 2 * d.pad_h, Wp = (long)d.W + 2 * d.pad_w;
  if (opix > kStgSmallInt / 2 || Hp > kStgSmallInt / 2 || Wp > kStgSmallInt / 2) return false;   // div_small
  if ((double)d.N * d.M * (double)opix >= 2147483648.0 || (double)d.N * d.C * (double)d.H * d.W >= 2147483648.0) return false;
  if ((double)d.N * (double)Hp >= 1073741824.0) return false;
  // the longest span of padded rows a chunk touches
  const long total = (long)d.N * opix;
  const int span_h = d.dil_h * (d.KH - 1);
  long rows = 0;
  for (long q0 = 0; q0 < total; q0 += kBwdChunkPixels) {
    const long q1 = std::min(total, q0 + kBwdChunkPixels) - 1;
    const long n0 = q0 / opix, n1 = q1 / opix;
    const long P0 = n0 * Hp + (q0 - n0 * opix) / g.OW, P1 = n1 * Hp + (q1 - n1 * opix) / g.OW + span_h;
    rows = std::max(rows, P1 - P0 + 1);
  }
  if (rows < 1 || (size_t)rows * (size_t)Wp * sizeof(float) > kStgLdsBudget) return false;
  sp->rows_max = (int)rows;
  sp->cs = (int)(rows * Wp);
  sp->icb = (int)std::min<size_t>((size_t)g.Cg, kStgLdsBudget / (sizeof(float) * (size_t)sp->cs));
  if (wgrad_channel_block > 0) sp->icb = std::min(sp->icb, wgrad_channel_block);
  sp->lds_bytes = sizeof(float) * (size_t)sp->icb * (size_t)sp->cs;
  sp->nblk = (g.Cg + sp->icb - 1) / sp->icb;
  sp->chunks = (int)((total + kBwdChunkPixels - 1) / kBwdChunkPixels);
  // enough workgroups for two per CU where the chunks and blocks alone do not give them: deal the output channels
  const long wgs = (long)sp->chunks * d.group * sp->nblk;
  const long want = 2L * std::max(n_cu, 1);
  const int osplit = (int)std::min<long>((g.Mg + kStgWaves - 1) / kStgWaves, (want + wgs - 1) / std::max(wgs, 1L));
  sp->osplit = std::max(1, std::min(osplit, 65535 / std::max(d.group, 1)));
  return sp->nblk <= 65535;   // grid z
}

// AUTO's rule for the weight gradient: a function of the geometry, nnz and the device's CU count only -- the two
// kernels' times in microseconds from a cost model fitted to one MI355X run of tools/backward_bench.py
// (profiles/backward_mi355x.md, "AUTO's rule": the fit, its coefficients and its residuals on the 47 benched layers).
// Both kernels run in rounds of resident workgroups: the entry kernel's (chunk, output channel) workgroups of 4 waves
// sit 8 to a CU, the staged kernel's 64 KiB workgroups 2 to a CU.  A last, partly filled round still costs a
// workgroup's latency, hence the floor on its fraction.
//   entry   21.3 + 0.153 chunks (its stage 2 walks the chunks serially) + rounds x (3.0 + 1.138 x entries per row)
//   staged  13.4 + rounds x (19.3 (staging the tile) + steps x (1.02 (loading G) + 0.426 x entries per (row, block)))
//           with steps = output channels a wave takes in turn
static double stg_rounds(double workgroups, double resident, double tail_floor) {
  const double r = workgroups / resident, whole = std::floor(r), tail = r - whole;
  return whole + (tail > 0 ? std::max(tail, tail_floor) : 0.0);
}
bool stg_auto_prefers(const Geometry &g, long nnz, const StgPlan &sp, int n_cu) {
  const escoin_conv_desc &d = g.d;
  if (nnz <= 0) return false;
  const double cus = (double)std::max(n_cu, 1);
  const double entry = 21.3 + 0.153 * sp.chunks +
                       stg_rounds((double)sp.chunks * d.M, 8.0 * cus, 0.3) * (3.0 + 1.138 * (double)nnz / d.M);
  const int steps = ((g.Mg + sp.osplit - 1) / sp.osplit + kStgWaves - 1) / kStgWaves;
  const double per_pair = (double)nnz / ((double)d.M * sp.nblk);
  const double staged = 13.4 + stg_rounds((double)sp.chunks * d.group * sp.nblk * sp.osplit, 2.0 * cus, 0.4) *
                                   (19.3 + steps * (1.02 + 0.426 * per_pair));
  return staged < entry;
}

bool wgm_plan(const Geometry &g, bool is_f64, WgmPlan *wp) {
  const escoin_conv_desc &d = g.d;
  if (is_f64) return false;
  const double two31 = 2147483648.0;
  const long lim28 = 1L << 28;
  if ((double)d.N * g.OH * (double)g.OW >= two31 || (double)d.M * (double)g.kdim >= two31 ||
      (double)g.Cg * d.H * (double)d.W >= two31)
    return false;
  if (d.H >= lim28 || d.W >= lim28 || d.pad_h >= lim28 || d.pad_w >= lim28 || (long)d.dil_h * (d.KH - 1) >= lim28 ||
      (long)d.dil_w * (d.KW - 1) >= lim28)
    return false;
  WgmPlan p;
  p.mtiles = (g.Mg + p.tile_m - 1) / p.tile_m;
  p.ktiles = (g.kdim + p.tile_k - 1) / p.tile_k;
  if ((long)d.group * p.mtiles > 65535 || p.ktiles > 65535) return false;   // grid y, z
  p.kpad = p.ktiles * p.tile_k;
  p.chunks = (int)(((long)d.N * g.OH * g.OW + kBwdChunkPixels - 1) / kBwdChunkPixels);
  p.lds_bytes = kWgmLdsBytes;
  *wp = p;
  return true;
}

// The tiles of one slice height: per (group, c-block) the greedy m-slices.  A row's entries of a c-block are counted with a
// cursor per row (columns ascend within a row, and a pointwise column IS the group-local channel).
static void pw_tiles(const Geometry &g, const CsrIndex *rowptr, const CsrIndex *colidx, int cblk, int cap, int height,
                     std::vector<PwTile> *first, std::vector<PwTile> *rest) {
  const int nblk = (g.Cg + cblk - 1) / cblk;
  std::vector<int> cur((size_t)g.Mg);
  for (int grp = 0; grp < g.d.group; ++grp) {
    const int *rp = rowptr ? (*rowptr)[grp].data() : nullptr;
    const int *ci = rowptr && colidx ? (*colidx)[grp].data() : nullptr;
    for (int m = 0; m < g.Mg; ++m) cur[m] = rp ? rp[m] : 0;
    for (int b = 0; b < nblk; ++b) {
      const int c0 = b * cblk, chans = std::min(cblk, g.Cg - c0);
      std::vector<PwTile> *out = b == 0 ? first : rest;
      PwTile t;
      int last = -1;   // the slice's last row with an entry
      auto close = [&](int end) {
        if (b > 0) t.rows = last - t.row0 + 1;   // (rows without an entry at the end)
        else t.rows = end - t.row0;
        if (t.rows > 0 && (b == 0 || t.items > 0)) out->push_back(t);
      };
      bool open = false;
      for (int m = 0; m < g.Mg; ++m) {
        int cnt;
        if (ci) {
          const int end = rp[m + 1];
          int j = cur[m];
          while (j < end && ci[j] < c0 + chans) ++j;
          cnt = j - cur[m];
          cur[m] = j;
        } else {
          cnt = rp ? std::min(rp[m + 1] - rp[m], chans) : chans;
        }
        if (open && (t.items + cnt > cap || m - t.row0 >= height)) {
          close(m);
          open = false;
        }
        if (!open) {
          if (b > 0 && cnt == 0) continue;       // (rows without an entry at the start)
          t = PwTile();
          t.grp = grp; t.row0 = m; t.c0 = c0; t.chans = chans;
          open = true;
          last = m;
        }
        t.items += cnt;
        if (cnt > 0) last = m;
      }
      if (open) close(g.Mg);
    }
  }
}

bool pw_plan(const Geometry &g, bool is_f64, long nnz, const CsrIndex *rowptr, const CsrIndex *colidx, int wgrad_channel_block,
             int tile_entries, int n_cu, PwPlan *pp) {
  const escoin_conv_desc &d = g.d;
  if (is_f64 || d.KH != 1 || d.KW != 1 || d.pad_h != 0 || d.pad_w != 0) return false;
  const double two31 = 2147483648.0;
  const double pixels = (double)d.N * g.OH * (double)g.OW;
  if (pixels >= two31 || (double)d.C * d.H * (double)d.W >= two31 || nnz < 0 || (double)nnz >= two31) return false;
  const long chunks = ((long)pixels + kBwdChunkPixels - 1) / kBwdChunkPixels;
  if (chunks > (long)kGridYZMax) return false;   // grid y
  PwPlan p;
  p.chunks = (int)chunks;
  p.tile_cap = tile_entries > 0 ? std::min(tile_entries, kPwMaxTileEntries) : kPwMaxTileEntries;
  p.cblk = std::min(std::min(g.Cg, kPwMaxChannelBlock), p.tile_cap);
  if (wgrad_channel_block > 0) p.cblk = std::min(p.cblk, wgrad_channel_block);
  int height = std::min(std::min(g.Mg, kPwMaxSliceRows), kPwMaxLdsRows - p.cblk);
  const long want = 2L * std::max(n_cu, 1);
  std::vector<PwTile> first, rest;
  for (;;) {
    first.clear();
    rest.clear();
    pw_tiles(g, rowptr, colidx, p.cblk, p.tile_cap, height, &first, &rest);
    if (height <= kPwMinSliceRows || nnz * chunks < kPwSplitWork || chunks * (long)(first.size() + rest.size()) >= want) break;
    height = std::max(kPwMinSliceRows, height / 2);
  }
  p.bias_tiles = (int)first.size();
  p.tiles = std::move(first);
  p.tiles.insert(p.tiles.end(), rest.begin(), rest.end());
  int fullest = 0;
  for (const PwTile &t : p.tiles) {
    p.rows_max = std::max(p.rows_max, t.rows);
    p.chans_max = std::max(p.chans_max, t.chans);
    fullest = std::max(fullest, t.items);
  }
  while (kPwThreads * p.lane_entries < fullest) p.lane_entries *= 2;
  p.lds_bytes = sizeof(float) * (size_t)p.pitch * (size_t)(p.rows_max + p.chans_max);
  *pp = std::move(p);
  return true;
}

bool dwg_plan(const Geometry &g, bool is_f64, int n_cu, int max_splits, DwgPlan *dp) {
  DwgPlan p;
  if (!wgm_plan(g, is_f64, &p.tile)) return false;
  const long chunks = p.tile.chunks;      // >= 1: N, OH, OW >= 1
  const long tiles = (long)g.d.group * p.tile.mtiles * p.tile.ktiles;
  // every span length once, the longest (fewest splits) first: a later one must be strictly cheaper to win
  const long resident = (long)kDwgResidentPerCu * std::max(n_cu, 1);
  long best_span = chunks, best_cost = -1;
  for (long span = chunks; span >= 1; --span) {
    const long s = (chunks + span - 1) / span;
    if (s > 1 && ((max_splits > 0 && s > max_splits) || tiles * s > kDwgMaxRounds * resident)) break;   // (s only grows from here)
    // rounds in 1/1024: what the workgroups fill, and half of what the last round leaves empty; one round at least
    const long filled = tiles * s * 1024 / resident, whole = (tiles * s + resident - 1) / resident * 1024;
    const long rounds = std::max(1024L, (filled + whole) / 2);
    const long cost = rounds * span + (1024 / kDwgSplitsPerChunkCost) * s;
    if (best_cost < 0 || cost < best_cost) best_cost = cost, best_span = span;
  }
  p.span = (int)best_span;
  p.splits = (int)((chunks + best_span - 1) / best_span);
  p.positions = (long)g.d.M * g.kdim;
  p.slab_bytes = sizeof(float) * (size_t)p.splits * (size_t)p.positions;
  *dp = p;
  return true;
}

bool dgm_plan(const Geometry &g, bool is_f64, DgmPlan *dp) {
  const escoin_conv_desc &d = g.d;
  if (is_f64) return false;
  const double two31 = 2147483648.0;
  const long lim28 = 1L << 28;
  if ((double)d.N * d.H * (double)d.W >= two31 || (double)g.Mg * g.OH * (double)g.OW >= two31) return false;
  if (d.H >= lim28 || d.W >= lim28 || d.pad_h >= lim28 || d.pad_w >= lim28 || (long)d.dil_h * (d.KH - 1) >= lim28 ||
      (long)d.dil_w * (d.KW - 1) >= lim28)
    return false;
  DgmPlan p;
  p.phases_h = d.stride_h;
  p.phases_w = d.stride_w;
  p.ctiles = (g.Cg + p.tile_c - 1) / p.tile_c;
  if ((long)d.stride_h * d.stride_w > 65535 || (long)d.group * p.ctiles > 65535) return false;   // grid y, z
  if ((double)d.stride_h * d.stride_w * (double)d.group * p.ctiles >= two31) return false;        // the live lists' index
  // one axis of the split: the residue's first pixel, its pixel count and its taps
  auto axis = [](int r, int size, int pad, int stride, int dil, int K, int *first, int *count, int *taps) {
    *first = ((r - pad) % stride + stride) % stride;
    *count = *first < size ? (size - *first + stride - 1) / stride : 0;
    *taps = 0;
    for (int k = 0; k < K; ++k) *taps += (int)((long)k * dil % stride == r);
  };
  p.phase.resize((size_t)d.stride_h * d.stride_w);
  for (int rh = 0; rh < d.stride_h; ++rh)
    for (int rw = 0; rw < d.stride_w; ++rw) {
      DgmPhase &ph = p.phase[(size_t)rh * d.stride_w + rw];
      axis(rh, d.H, d.pad_h, d.stride_h, d.dil_h, d.KH, &ph.h0, &ph.rows, &ph.taps_h);
      axis(rw, d.W, d.pad_w, d.stride_w, d.dil_w, d.KW, &ph.w0, &ph.cols, &ph.taps_w);
      ph.kp = g.Mg * ph.taps_h * ph.taps_w;
      ph.ksteps = (ph.kp + p.step_k - 1) / p.step_k;
      ph.tiles = ((long)d.N * ph.rows * ph.cols + p.tile_p - 1) / p.tile_p;
      p.tiles_max = std::max(p.tiles_max, ph.tiles);
      p.cols_total += (long)ph.ksteps * p.step_k;
    }
  const double mat = (double)d.group * p.ctiles * p.tile_c * (double)p.cols_total;
  if (mat >= two31) return false;
  p.mat_floats = (long)mat;
  p.lds_bytes = kDgmLdsBytes;
  *dp = p;
  return true;
}

bool bwd_transposable(const Geometry &g, bool is_f64) {
  const escoin_conv_desc &d = g.d;
  return !is_f64 && d.stride_h == 1 && d.stride_w == 1 && d.pad_h <= d.dil_h * (d.KH - 1) &&
         d.pad_w <= d.dil_w * (d.KW - 1) && g.Mg <= 32767;
}

BwdChoice bwd_choice(const Geometry &g, bool is_f64, long nnz, const BwdOptions &o, int n_cu) {
  const escoin_conv_desc &d = g.d;
  BwdChoice c;
  auto refuse = [&c](const char *why) { c.rc = ESCOIN_EINVAL; c.error = why; return c; };
  if (g.Mg > 65535) return refuse("backward: more than 65535 output channels per group");
  if (d.C > 4 * 65535 || d.N > 65535) return refuse("backward: grid dimension exceeds 65535");
  const bool transposable = bwd_transposable(g, is_f64);
  const bool forced = o.backward_kernel == ESCOIN_KERNEL_TILED || o.backward_kernel == ESCOIN_KERNEL_JIT ||
                      o.backward_kernel == ESCOIN_KERNEL_DENSE;
  // an inner plan (option "s2d" / "s2b"): GENERIC and BWD_MFMA keep the plan's own gather / MFMA kernel, the others go to the inner plan
  const bool inner = o.s2d && o.backward_kernel != ESCOIN_KERNEL_GENERIC && o.backward_kernel != ESCOIN_BWD_MFMA;
  if (forced && !transposable && !inner)
    return refuse("backward_kernel: this plan has no transposed forward plan (needs a float plan, stride 1, "
                  "pad <= dilation * (kernel - 1)); only the gather kernel serves it");
  const bool staged_ok = stg_plan(g, is_f64, o.wgrad_channel_block, n_cu, &c.stg);
  if (o.wgrad_kernel == ESCOIN_WGRAD_STAGED && !staged_ok)
    return refuse("wgrad_kernel: the staged weight-gradient kernel needs a float plan with stride 1 whose "
                  "chunk tile of one input channel fits the LDS budget; only the entry kernel serves this plan");
  if (o.wgrad_kernel == ESCOIN_WGRAD_MFMA && !wgm_plan(g, is_f64, &c.wgm))
    return refuse("wgrad_kernel: the MFMA weight-gradient kernel needs a float plan whose pixel, weight and "
                  "image indices fit 31 bits; the entry kernel serves this plan");
  if (o.backward_kernel == ESCOIN_BWD_MFMA && !dgm_plan(g, is_f64, &c.dgm))
    return refuse("backward_kernel: the MFMA data-gradient kernel needs a float plan whose pixel, top and "
                  "matrix indices fit 31 bits; the gather kernel serves this plan");
  if (nnz > 0x7fffffffL) return refuse("backward: more than 2^31 nonzeros");
  c.data = inner ? kBwdInner
           : o.backward_kernel == ESCOIN_BWD_MFMA ? kBwdMfma
           : transposable && o.backward_kernel != ESCOIN_KERNEL_GENERIC ? kBwdTransposed : kBwdGather;
  if (o.wgrad_kernel == ESCOIN_WGRAD_MFMA) c.wgrad = ESCOIN_WGRAD_MFMA;
  else if (staged_ok && (o.wgrad_kernel == ESCOIN_WGRAD_STAGED ||
                         (o.wgrad_kernel == ESCOIN_WGRAD_AUTO && stg_auto_prefers(g, nnz, c.stg, n_cu))))
    c.wgrad = ESCOIN_WGRAD_STAGED;
  // option "wgrad_pointwise": AUTO's answer gives way on a plan the pointwise kernel serves; a forced kernel does not
  if (o.wgrad_pointwise && o.wgrad_kernel == ESCOIN_WGRAD_AUTO &&
      pw_plan(g, is_f64, nnz, nullptr, nullptr, o.wgrad_channel_block, o.pw_tile_entries, n_cu, &c.pw))
    c.wgrad = ESCOIN_WGRAD_POINTWISE;
  c.chunks_max = (int)(((long)d.N * g.OH * g.OW + kBwdChunkPixels - 1) / kBwdChunkPixels);
  return c;
}

bool s2d_plan(const Geometry &g, bool is_f64, S2dPlan *sp) {
  const escoin_conv_desc &d = g.d;
  if (is_f64) return false;
  if (d.stride_h == 1 && d.stride_w == 1) return false;
  if (d.dil_h != 1 || d.dil_w != 1) return false;
  const long lim28 = 1L << 28;
  if ((long)d.H + 2L * d.pad_h >= lim28 || (long)d.W + 2L * d.pad_w >= lim28 || d.stride_h >= lim28 || d.stride_w >= lim28) return false;
  S2dPlan p;
  p.PH = std::min(d.stride_h, d.KH);
  p.PW = std::min(d.stride_w, d.KW);
  escoin_conv_desc &in = p.inner;
  in = d;
  in.KH = (d.KH + d.stride_h - 1) / d.stride_h;
  in.KW = (d.KW + d.stride_w - 1) / d.stride_w;
  in.H = g.OH + in.KH - 1;
  in.W = g.OW + in.KW - 1;
  in.pad_h = in.pad_w = 0;
  in.stride_h = in.stride_w = 1;
  const double two31 = 2147483648.0;
  const double c_in = (double)d.C * p.PH * p.PW, cg_in = (double)g.Cg * p.PH * p.PW;
  if (cg_in > 32767.0) return false;
  const double x_floats = (double)d.N * c_in * in.H * (double)in.W;
  if (x_floats >= two31 || (double)d.N * d.C * d.H * (double)d.W >= two31) return false;
  if ((double)d.M * cg_in * in.KH * (double)in.KW >= two31) return false;
  in.C = d.C * p.PH * p.PW;
  p.x_floats = (long)x_floats;
  *sp = p;
  return true;
}

bool s2b_plan(const Geometry &g, bool is_f64, S2bPlan *sp) {
  const escoin_conv_desc &d = g.d;
  if (is_f64) return false;
  if (d.stride_h != 1 || d.stride_w != 1) return false;
  const long lim28 = 1L << 28;
  if ((long)d.H + 2L * d.pad_h >= lim28 || (long)d.W + 2L * d.pad_w >= lim28 || d.dil_h >= lim28 || d.dil_w >= lim28) return false;
  S2bPlan p;
  p.eh = d.KH > 1 ? d.dil_h : 1;     // (a dilation on an axis with one tap is no dilation)
  p.ew = d.KW > 1 ? d.dil_w : 1;
  const long P = (long)p.eh * p.ew;
  if (P <= 1 || (long)d.N * P > kS2bMaxInnerImages) return false;
  escoin_conv_desc &in = p.inner;
  in = d;
  in.N = (int)(d.N * P);
  in.H = (d.H + 2 * d.pad_h + p.eh - 1) / p.eh;
  in.W = (d.W + 2 * d.pad_w + p.ew - 1) / p.ew;
  in.pad_h = in.pad_w = 0;
  in.dil_h = in.dil_w = 1;
  in.fuse_relu = 0;                  // (the unpack kernel applies the outer plan's ReLU)
  const int ohi = in.H - d.KH + 1, owi = in.W - d.KW + 1;      // = ceil(OH / eh), ceil(OW / ew)
  const double two31 = 2147483648.0;
  const double x_floats = (double)in.N * d.C * in.H * (double)in.W, t_floats = (double)in.N * d.M * ohi * (double)owi;
  if (x_floats >= two31 || t_floats >= two31) return false;
  if ((double)d.N * d.C * d.H * (double)d.W >= two31 || (double)d.N * d.M * g.OH * (double)g.OW >= two31) return false;
  p.x_floats = (long)x_floats;
  p.t_floats = (long)t_floats;
  *sp = p;
  return true;
}

bool b2s_plan(const Geometry &g, bool is_f64, int block, int /*n_cu*/, B2sPlan *bp) {
  const escoin_conv_desc &d = g.d;
  if (is_f64) return false;
  if (d.H != 1 || d.W != 1 || d.KH != 1 || d.KW != 1 || d.pad_h != 0 || d.pad_w != 0) return false;
  auto inner_images = [&d](int B) { return ((long)d.N + B - 1) / B; };
  int B = block;
  if (B == 0) {
    B = 64;
    while (B < kB2sMaxBlock && inner_images(B) > kS2bMaxInnerImages) B *= 2;      // (a batch above 4 million)
  }
  if (B < kB2sMinBlock || B > kB2sMaxBlock || B % 4 != 0) return false;
  const long np = inner_images(B);
  if (np > kS2bMaxInnerImages) return false;
  const double two31 = 2147483648.0;
  const double x_floats = (double)np * d.C * B, t_floats = (double)np * d.M * B;
  if (x_floats >= two31 || t_floats >= two31) return false;      // (the bottom N * C and the top N * M are no larger)
  B2sPlan p;
  p.B = B;
  escoin_conv_desc &in = p.inner;
  in = d;
  in.N = (int)np;
  in.H = 1;
  in.W = B;
  in.stride_h = in.stride_w = 1;
  in.dil_h = in.dil_w = 1;
  in.fuse_relu = 0;                  // (the unpack kernel applies the outer plan's ReLU)
  p.x_floats = (long)x_floats;
  p.t_floats = (long)t_floats;
  *bp = p;
  return true;
}

bool d2s_plan(const escoin_conv_desc &d, bool is_f64, D2sPlan *dp) {
  D2sPlan p;
  auto refuse = [&](const char *why) { p.error = why; *dp = p; return false; };
  if (is_f64) return refuse("option \"deconv\": a double plan has no deconvolution (the inner kernels are fp32)");
  if (d.dil_h != 1 || d.dil_w != 1) return refuse("option \"deconv\": a dilation other than 1 is not served");
  const long oh = (long)d.stride_h * (d.H - 1) + d.KH - 2L * d.pad_h, ow = (long)d.stride_w * (d.W - 1) + d.KW - 2L * d.pad_w;
  if (oh < 1 || ow < 1) return refuse("option \"deconv\": empty top (OH or OW < 1: the pad crops the whole image)");
  if (d.M / d.group > 32767) return refuse("option \"deconv\": more than 32767 output channels per group");
  const double two31 = 2147483648.0;
  const double Pd = (double)d.stride_h * d.stride_w;
  if ((double)d.M * Pd > (double)kD2sMaxInnerChannels)
    return refuse("option \"deconv\": M * stride_h * stride_w exceeds the inner plan's channel limit (a grid axis)");
  const int kh = (d.KH + d.stride_h - 1) / d.stride_h, kw = (d.KW + d.stride_w - 1) / d.stride_w;
  const long hi = (long)d.H + kh - 1, wi = (long)d.W + kw - 1;
  const double top_floats = (double)d.N * d.M * (double)oh * (double)ow;
  if (top_floats >= two31) return refuse("option \"deconv\": the top blob reaches 2^31 elements");
  const double t_floats = (double)d.N * d.M * Pd * (double)hi * (double)wi;
  if (t_floats >= two31) return refuse("option \"deconv\": the inner top T' reaches 2^31 elements");
  if ((double)d.M * Pd * (d.C / d.group) * kh * (double)kw >= two31)
    return refuse("option \"deconv\": the inner weight matrix reaches 2^31 elements");
  p.OH = (int)oh; p.OW = (int)ow;
  p.sh = d.stride_h; p.sw = d.stride_w; p.P = d.stride_h * d.stride_w;
  escoin_conv_desc &in = p.inner;
  in = d;
  in.M = d.M * p.P;
  in.KH = kh; in.KW = kw;
  in.pad_h = kh - 1; in.pad_w = kw - 1;
  in.stride_h = in.stride_w = 1;
  in.dil_h = in.dil_w = 1;
  in.fuse_relu = 0;                  // (the unpack kernel adds the bias and applies the ReLU; has_bias stays the outer plan's)
  escoin_conv_desc &mi = p.mirror;
  mi = d;
  mi.C = d.M; mi.M = d.C;
  mi.H = p.OH; mi.W = p.OW;
  p.t_floats = (long)t_floats;
  p.top_floats = (long)top_floats;
  p.unpack_rows = (long)d.N * d.M * oh;
  p.pack_rows = (long)d.N * d.M * p.P * hi;
  *dp = p;
  return true;
}

}  // namespace escoin
