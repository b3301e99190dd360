// tests/cpp/launch_limits_check.cpp -- the size limits of the library, on the host alone (test code).
//
// Compiled with plain g++ against align_rules.cpp, stream_builder.cpp and jit_codegen.cpp: no HIP header, no device.
//
//   launch_limits_check edges             every launch-time limit of align_rules.h ("the size limits a launch checks") and
//                                         every plan rule's 2^31 / 65535 limit, one unit on either side of its edge;
//                                         prints one line per check and exits 1 at the first that fails
//   launch_limits_check cases <manifest>  one line per case: N C H W M KH KW pad_h pad_w stride_h stride_w dil_h dil_w group
//                                         kernel n_images n_cu weights-file (float32, M x Cg x KH x KW); takes the case
//                                         to its layout the way sconv_tiled.hip's tiled_build does and prints, as JSON,
//                                         what a forward of n_images would do: the launches of launch_tiled, each one's
//                                         epilogue path and compiled body, and what the dense and generic kernels say
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "align_rules.h"

using namespace escoin;

static Geometry geom(long N, long C, long H, long W, long M, int KH, int KW, int pad_h, int pad_w, int stride, int dil, int group) {
  Geometry g;
  escoin_conv_desc &d = g.d;
  memset(&d, 0, sizeof d);
  d.N = (int)N; d.C = (int)C; d.H = (int)H; d.W = (int)W; d.M = (int)M; d.KH = KH; d.KW = KW; d.pad_h = pad_h; d.pad_w = pad_w;
  d.stride_h = d.stride_w = stride; d.dil_h = d.dil_w = dil; d.group = group;
  g.OH = (d.H + 2 * d.pad_h - (d.dil_h * (d.KH - 1) + 1)) / d.stride_h + 1;
  g.OW = (d.W + 2 * d.pad_w - (d.dil_w * (d.KW - 1) + 1)) / d.stride_w + 1;
  g.Cg = d.C / d.group;
  g.Mg = d.M / d.group;
  g.kdim = g.Cg * d.KH * d.KW;
  return g;
}

static int n_checks = 0, n_failed = 0;
static void expect(bool ok, const char *what) {
  ++n_checks;
  printf("%s  %s\n", ok ? "ok  " : "FAIL", what);
  if (!ok) ++n_failed;
}
static bool refuses(const LaunchVerdict &v, const char *msg) { return v.rc == ESCOIN_EINVAL && !strcmp(v.error, msg); }
static bool passes(const LaunchVerdict &v) { return v.rc == ESCOIN_OK && !strcmp(v.error, ""); }

static int edges() {
  const unsigned long long two31 = 1ull << 31, range = 0xFFFFFFF0ull;
  // ---- the launch-time limits, at their documented values --------------------------------------------------------
  expect(kDescriptorRange == range && kEpiStoreRange == two31 && kGridYZMax == 65535u, "the three constants are the documented ones");
  expect(epi_store_fits(two31 - 4) && !epi_store_fits(two31), "epi_store: true at 2^31 - 4 bytes, false at 2^31");
  {
    // ... and through tiled_launch_shape, which is what a launch reads: 16 -> 512 1x1 on 16 x 16, one image = 2^19 bytes
    const Geometry g = geom(4096, 16, 16, 16, 512, 1, 1, 0, 0, 1, 1, 1);
    Tiling t;
    t.OH = 16; t.OW = 16; t.nseg = 1; t.n_ocblk = 1; t.waves = 8;
    expect(tiled_launch_shape(g, t, 4095, 1, false, 0, 256).epi_store && !tiled_launch_shape(g, t, 4096, 1, false, 0, 256).epi_store,
           "tiled_launch_shape: epi_store at 4095 images of 2^19 bytes, not at 4096");
  }
  expect(passes(dense_bytes_limit(range - 4, 16)) && passes(dense_bytes_limit(16, range - 4)),
         "dense: 0xFFFFFFF0 - 4 bytes of bottom or of weights pass");
  const char *dense_msg = "dense kernel: bottom blob or weight matrix exceeds the 4 GiB descriptor range";
  expect(refuses(dense_bytes_limit(range, 16), dense_msg) && refuses(dense_bytes_limit(16, range), dense_msg),
         "dense: 0xFFFFFFF0 bytes of bottom or of weights are refused");
  expect(passes(dense_pixels_limit((1l << 31) - 1)) && refuses(dense_pixels_limit(1l << 31), "dense kernel: N*OH*OW does not fit 31 bits"),
         "dense: N*OH*OW passes at 2^31 - 1 and is refused at 2^31");
  const char *strided_msg = "tiled kernel: strided pointwise layer with a top blob of 2 GiB or more";
  expect(passes(tiled_strided_top_limit(true, two31 - 4)) && refuses(tiled_strided_top_limit(true, two31), strided_msg) &&
             passes(tiled_strided_top_limit(false, two31)) && passes(tiled_strided_top_limit(false, 4 * two31)),
         "tiled: a strided pointwise top passes at 2^31 - 4 bytes and is refused at 2^31; other layers are not asked");
  const char *image_msg = "tiled kernel: one image exceeds the 4 GiB descriptor range";
  expect(passes(tiled_image_limit(range - 4, range)) && refuses(tiled_image_limit(range, range), image_msg) &&
             passes(tiled_image_limit(4092, 4096)) && refuses(tiled_image_limit(4096, 4096), image_msg),
         "tiled: an image passes 4 bytes below the range and is refused at it (the real range and option max_launch_bytes)");
  expect(passes(tiled_grid_limit(65535)) && refuses(tiled_grid_limit(65536), "tiled kernel: grid.y exceeds 65535"),
         "tiled: grid y passes at 65535 and is refused at 65536");
  const char *grid_msg[4] = {"generic kernel: grid dimension exceeds 65535", "csrmm: grid dimension exceeds 65535",
                             "csrmm_f64: more than 65535 rows", "im2col: grid dimension exceeds 65535"};
  for (int k = 0; k < 4; ++k) {
    const GridKernel gk = (GridKernel)k;
    bool ok = passes(grid_yz_limit(gk, 65535, 65535)) && refuses(grid_yz_limit(gk, 65536, 1), grid_msg[k]);
    if (gk == kGridCsrmmF64) ok = ok && passes(grid_yz_limit(gk, 1, 65536));     // (its grid has no z)
    else ok = ok && refuses(grid_yz_limit(gk, 1, 65536), grid_msg[k]);
    expect(ok, grid_msg[k]);
  }
  expect(passes(generic_call_limits(geom(65535, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1), 65535)) &&
             refuses(generic_call_limits(geom(65536, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1), 65536), grid_msg[0]) &&
             passes(generic_call_limits(geom(1, 1, 1, 1, 4 * 65535, 1, 1, 0, 0, 1, 1, 1), 1)) &&
             refuses(generic_call_limits(geom(1, 1, 1, 1, 4 * 65535 + 1, 1, 1, 0, 0, 1, 1, 1), 1), grid_msg[0]),
         "generic: 65535 images and 4 x 65535 output channels pass, one more of either is refused");
  // ---- launch_tiled's sub-batch ----------------------------------------------------------------------------------
  expect(tiled_launch_range(0) == range && tiled_launch_range(4096) == 4096 && tiled_launch_range(0x7fffffffffffL) == range,
         "tiled: the launch range is the descriptor's unless option max_launch_bytes lowers it");
  {
    const unsigned long long in_image = 256ull * 16 * 16 * 4;      // 256 channels of 16 x 16: 2^18 bytes
    const int want = (int)((range - 16) / in_image);
    expect(want == 16383 && tiled_chunk(16385, in_image, range) == want && tiled_launches(16385, want) == 2 &&
               tiled_chunk(16383, in_image, range) == 16383 && tiled_launches(16383, 16383) == 1 &&
               tiled_chunk(16384, in_image, range) == 16383 && tiled_launches(16384, 16383) == 2,
           "tiled: with the real limit a launch takes (0xFFFFFFF0 - 16) / in_image = 16383 images of 2^18 bytes");
    expect((unsigned long long)want * in_image < range && (unsigned long long)(want + 1) * in_image >= range,
           "tiled: that sub-batch is the largest the descriptor covers");
    expect(tiled_chunk(5, range - 4, range) == 1 && tiled_chunk(5, 2 * range, range) == 1 && tiled_chunk(0, in_image, range) == 1,
           "tiled: a sub-batch is one image at least");
    expect(tiled_chunk(7, 1000, 4096) == 4 && tiled_launches(7, 4) == 2, "tiled: option max_launch_bytes = 4096 puts 4 images of 1000 bytes in a launch");
  }
  {
    // tiled_call_limits: the order a call's launches meet the refusals in
    Tiling t;
    t.n_ocblk = 1;
    const Geometry sp = geom(2048, 8, 32, 32, 256, 1, 1, 0, 0, 2, 1, 1);      // strided pointwise: top image 256 x 16 x 16 x 4 = 2^18 bytes
    expect(strided_pointwise(sp) && passes(tiled_call_limits(sp, t, 8191, 1, 0)) && refuses(tiled_call_limits(sp, t, 8192, 1, 0), strided_msg),
           "tiled_call_limits: the strided pointwise layer 8 x 32 x 32 -> 256 passes at 8191 images and is refused at 8192");
    t.n_ocblk = 65536;
    expect(refuses(tiled_call_limits(sp, t, 1, 1, 0), "tiled kernel: grid.y exceeds 65535"), "tiled_call_limits: grid y");
    expect(refuses(tiled_call_limits(sp, t, 1, 1, 1024), image_msg), "tiled_call_limits: the image limit comes first");
  }
  // ---- the plan rules: refused at the first size past their stated limit, accepted just below -----------------------
  WgmPlan wp;
  expect(wgm_plan(geom(32767, 1, 256, 256, 1, 1, 1, 0, 0, 1, 1, 1), false, &wp) && !wgm_plan(geom(32768, 1, 256, 256, 1, 1, 1, 0, 0, 1, 1, 1), false, &wp),
         "wgm_plan: N*OH*OW = 2^31 - 2^16 accepted, 2^31 refused");
  expect(wgm_plan(geom(1, 32767, 256, 256, 1, 1, 1, 0, 0, 1, 1, 1), false, &wp) && !wgm_plan(geom(1, 32768, 256, 256, 1, 1, 1, 0, 0, 1, 1, 1), false, &wp),
         "wgm_plan: Cg*H*W = 2^31 - 2^16 accepted, 2^31 refused");
  expect(wgm_plan(geom(1, 32767, 1, 1, 65536, 1, 1, 0, 0, 1, 1, 1), false, &wp) && !wgm_plan(geom(1, 32768, 1, 1, 65536, 1, 1, 0, 0, 1, 1, 1), false, &wp),
         "wgm_plan: M*Cg*KH*KW = 2^31 - 2^16 accepted, 2^31 refused");
  expect(wgm_plan(geom(1, 65535, 1, 1, 65535 * 64, 1, 1, 0, 0, 1, 1, 65535), false, &wp) &&
             !wgm_plan(geom(1, 65536, 1, 1, 65536 * 64, 1, 1, 0, 0, 1, 1, 65536), false, &wp),
         "wgm_plan: 65535 (group, M-tile) pairs accepted, 65536 refused");
  expect(wgm_plan(geom(1, 65535 * 64, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1), false, &wp) && !wgm_plan(geom(1, 65535 * 64 + 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1), false, &wp),
         "wgm_plan: 65535 column tiles accepted, 65536 refused");
  DgmPlan dp;
  expect(dgm_plan(geom(32767, 1, 256, 256, 1, 1, 1, 0, 0, 1, 1, 1), false, &dp) && !dgm_plan(geom(32768, 1, 256, 256, 1, 1, 1, 0, 0, 1, 1, 1), false, &dp),
         "dgm_plan: N*H*W = 2^31 - 2^16 accepted, 2^31 refused");
  expect(dgm_plan(geom(1, 1, 256, 256, 32767, 1, 1, 0, 0, 1, 1, 1), false, &dp) && !dgm_plan(geom(1, 1, 256, 256, 32768, 1, 1, 0, 0, 1, 1, 1), false, &dp),
         "dgm_plan: Mg*OH*OW = 2^31 - 2^16 accepted, 2^31 refused");
  expect(dgm_plan(geom(1, 65535 * 64, 1, 1, 65535, 1, 1, 0, 0, 1, 1, 65535), false, &dp) &&
             !dgm_plan(geom(1, 65536 * 64, 1, 1, 65536, 1, 1, 0, 0, 1, 1, 65536), false, &dp),
         "dgm_plan: 65535 (group, channel tile) pairs accepted, 65536 refused");
  expect(dgm_plan(geom(1, 1, 600, 600, 1, 1, 1, 0, 0, 255, 1, 1), false, &dp) && !dgm_plan(geom(1, 1, 600, 600, 1, 1, 1, 0, 0, 256, 1, 1), false, &dp),
         "dgm_plan: 255 x 255 = 65025 phases accepted, 256 x 256 = 65536 refused");
  // the large-blob test's strided shape: dgm_plan's largest batch is 32767 images; wgm_plan (dense_wgrad) takes it up to 131071
  expect(dgm_plan(geom(32767, 1, 256, 256, 1, 3, 3, 1, 1, 2, 1, 1), false, &dp) && !dgm_plan(geom(32768, 1, 256, 256, 1, 3, 3, 1, 1, 2, 1, 1), false, &dp) &&
             wgm_plan(geom(131071, 1, 256, 256, 1, 3, 3, 1, 1, 2, 1, 1), false, &wp) && !wgm_plan(geom(131072, 1, 256, 256, 1, 3, 3, 1, 1, 2, 1, 1), false, &wp),
         "1 x 256 x 256 under 3x3 stride 2: dgm_plan accepts 32767 images and refuses 32768, wgm_plan accepts 131071 and refuses 131072");
  S2dPlan sd;
  // stride 2, 1x1: X' has C' = C channels of OH x OW pixels, so the bottom is the larger blob
  expect(s2d_plan(geom(32767, 1, 256, 256, 1, 1, 1, 0, 0, 2, 1, 1), false, &sd) && !s2d_plan(geom(32768, 1, 256, 256, 1, 1, 1, 0, 0, 2, 1, 1), false, &sd),
         "s2d_plan: a bottom of 2^31 - 2^16 elements accepted, of 2^31 refused");
  // stride 2, 2x2 on 2 x 2: X' = N x 4 C x 1 x 1 is as large as the bottom; the inner weight matrix M x 4 Cg
  expect(s2d_plan(geom(1, 8191, 2, 2, 65536, 2, 2, 0, 0, 2, 1, 1), false, &sd) && !s2d_plan(geom(1, 8192, 2, 2, 65536, 2, 2, 0, 0, 2, 1, 1), false, &sd),
         "s2d_plan: an inner weight matrix of 2^31 - 2^18 elements accepted, of 2^31 refused (Cg' = 32768 is refused too)");
  // the large-blob test's shape: the bottom passes 4 GiB at 2^30 + 2^17 elements, X' (512 x 17 x 17 per image) is larger
  expect(s2d_plan(geom(8193, 128, 32, 32, 16, 3, 3, 1, 1, 2, 1, 1), false, &sd) && sd.x_floats == 8193l * 512 * 17 * 17 && sd.x_floats > (1l << 30),
         "s2d_plan: 128 x 32 x 32 under stride 2 at 8193 images accepted");
  S2bPlan sb;
  expect(s2b_plan(geom(16383, 1, 4, 4, 1, 3, 3, 2, 2, 1, 2, 1), false, &sb) && sb.inner.N == 65532 &&
             !s2b_plan(geom(16384, 1, 4, 4, 1, 3, 3, 2, 2, 1, 2, 1), false, &sb),
         "s2b_plan: N * P = 65532 inner images accepted, 65536 refused");
  expect(s2b_plan(geom(65535, 1, 3, 4, 1, 1, 3, 0, 1, 1, 1, 1), false, &sb) == false, "s2b_plan: no dilation, no plan");
  {
    // dilation 2 on the width only (KH = 1): P = 2, so N * P = 65534 accepted and 65536 refused
    Geometry a = geom(32767, 1, 4, 4, 1, 1, 3, 0, 2, 1, 2, 1), b = geom(32768, 1, 4, 4, 1, 1, 3, 0, 2, 1, 2, 1);
    expect(s2b_plan(a, false, &sb) && sb.inner.N == 65534 && !s2b_plan(b, false, &sb), "s2b_plan: N * P = 65534 accepted, 65536 refused (P = 2)");
  }
  // 4 x 4 with pad 2 and dilation 2: four classes of 4 x 4 pixels, X' = 64 C elements per image (the bottom and the tops are smaller)
  expect(s2b_plan(geom(1, (1 << 25) - 1, 4, 4, 1, 3, 3, 2, 2, 1, 2, 1), false, &sb) && sb.x_floats == (1l << 31) - 64 &&
             !s2b_plan(geom(1, 1 << 25, 4, 4, 1, 3, 3, 2, 2, 1, 2, 1), false, &sb),
         "s2b_plan: X' of 2^31 - 64 elements accepted, of 2^31 refused");
  // the large-blob test's shapes: 256 channels at 16385 images is one image too many for N * P, 512 channels at 8193 is served
  expect(!s2b_plan(geom(16385, 256, 16, 16, 16, 3, 3, 2, 2, 1, 2, 1), false, &sb) && s2b_plan(geom(8193, 512, 16, 16, 16, 3, 3, 2, 2, 1, 2, 1), false, &sb) &&
             sb.inner.N == 32772,
         "s2b_plan: 256 x 16 x 16 at 16385 images refused (65540 inner images), 512 x 16 x 16 at 8193 accepted");
  B2sPlan bp;
  expect(b2s_plan(geom(65535 * 256, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1), false, 0, 256, &bp) && bp.B == 256 && bp.inner.N == 65535 &&
             !b2s_plan(geom(65535 * 256 + 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1), false, 0, 256, &bp),
         "b2s_plan: 65535 inner images of 256 accepted, 65536 refused");
  expect(b2s_plan(geom(65537 * 4, 4096, 1, 1, 16, 1, 1, 0, 0, 1, 1, 1), false, 0, 256, &bp) && bp.B == 64 && bp.inner.N == 4097 &&
             bp.x_floats == 4097l * 4096 * 64,
         "b2s_plan: 65537 x 4 images of 4096 features: blocks of 64, 4097 inner images, X' of 2^30 + 2^18 elements");
  expect(b2s_plan(geom(8191 * 64, 4096, 1, 1, 16, 1, 1, 0, 0, 1, 1, 1), false, 0, 256, &bp) &&
             !b2s_plan(geom(8192 * 64, 4096, 1, 1, 16, 1, 1, 0, 0, 1, 1, 1), false, 0, 256, &bp),
         "b2s_plan: X' of 2^31 - 2^18 elements accepted, of 2^31 refused");
  BwdOptions bo;
  bo.backward_kernel = ESCOIN_KERNEL_AUTO; bo.wgrad_kernel = ESCOIN_WGRAD_ENTRY; bo.wgrad_channel_block = 0; bo.s2d = false;
  const char *bwd_grid = "backward: grid dimension exceeds 65535";
  expect(bwd_choice(geom(65535, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1), false, 1, bo, 256).rc == ESCOIN_OK &&
             !strcmp(bwd_choice(geom(65536, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1), false, 1, bo, 256).error, bwd_grid),
         "bwd_choice: 65535 images accepted, 65536 refused");
  expect(bwd_choice(geom(1, 4 * 65535, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1), false, 1, bo, 256).rc == ESCOIN_OK &&
             !strcmp(bwd_choice(geom(1, 4 * 65535 + 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1), false, 1, bo, 256).error, bwd_grid),
         "bwd_choice: 4 x 65535 input channels accepted, one more refused");
  expect(bwd_choice(geom(1, 1, 1, 1, 65535, 1, 1, 0, 0, 1, 1, 1), false, 1, bo, 256).rc == ESCOIN_OK &&
             !strcmp(bwd_choice(geom(1, 1, 1, 1, 65536, 1, 1, 0, 0, 1, 1, 1), false, 1, bo, 256).error,
                     "backward: more than 65535 output channels per group"),
         "bwd_choice: 65535 output channels per group accepted, 65536 refused");
  expect(bwd_choice(geom(1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1), false, 0x7fffffffL, bo, 256).rc == ESCOIN_OK &&
             !strcmp(bwd_choice(geom(1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1), false, 0x80000000L, bo, 256).error, "backward: more than 2^31 nonzeros"),
         "bwd_choice: 2^31 - 1 nonzeros accepted, 2^31 refused");
  bo.wgrad_kernel = ESCOIN_WGRAD_MFMA;
  expect(bwd_choice(geom(32767, 1, 256, 256, 1, 1, 1, 0, 0, 1, 1, 1), false, 1, bo, 256).rc == ESCOIN_OK &&
             bwd_choice(geom(32768, 1, 256, 256, 1, 1, 1, 0, 0, 1, 1, 1), false, 1, bo, 256).rc == ESCOIN_EINVAL,
         "bwd_choice: wgrad_kernel MFMA is refused where wgm_plan refuses");
  // the weight-gradient shape of the large-blob tests: top_diff passes 2^31 ELEMENTS at 32769 images, which is no limit of
  // wgm_plan's (its kernel indexes top_diff with 64-bit expressions): N*OH*OW is 2^23 + 2^8
  expect(wgm_plan(geom(32769, 16, 16, 16, 256, 3, 3, 1, 1, 1, 1, 1), false, &wp), "wgm_plan: 16 -> 256 3x3 on 16 x 16 accepted at 32769 images");
  // ... but a limit of stg_plan's (N*M*OH*OW and N*C*H*W below 2^31): the staged kernel takes that layer up to 32767 images
  StgPlan stg;
  expect(stg_plan(geom(32767, 16, 16, 16, 256, 3, 3, 1, 1, 1, 1, 1), false, 0, 256, &stg) &&
             !stg_plan(geom(32768, 16, 16, 16, 256, 3, 3, 1, 1, 1, 1, 1), false, 0, 256, &stg) &&
             !stg_plan(geom(32768, 256, 16, 16, 16, 3, 3, 1, 1, 1, 1, 1), false, 0, 256, &stg),
         "stg_plan: top_diff or bottom of 2^31 - 2^16 elements accepted, of 2^31 refused");
  bo.wgrad_kernel = ESCOIN_WGRAD_STAGED;
  expect(bwd_choice(geom(32767, 16, 16, 16, 256, 3, 3, 1, 1, 1, 1, 1), false, 1, bo, 256).wgrad == ESCOIN_WGRAD_STAGED &&
             bwd_choice(geom(32769, 16, 16, 16, 256, 3, 3, 1, 1, 1, 1, 1), false, 1, bo, 256).rc == ESCOIN_EINVAL,
         "bwd_choice: wgrad_kernel STAGED is refused where stg_plan refuses");
  printf("%d checks, %d failed\n", n_checks, n_failed);
  return n_failed ? 1 : 0;
}

static int cases(const char *manifest) {
  std::ifstream in(manifest);
  int kernel, n_images, n_cu, n_cases = 0, stride, dil;
  std::string path;
  long N, C, H, W, M;
  int KH, KW, pad_h, pad_w, stride_w, dil_w, group;
  while (in >> N >> C >> H >> W >> M >> KH >> KW >> pad_h >> pad_w >> stride >> stride_w >> dil >> dil_w >> group >> kernel >> n_images >> n_cu >> path) {
    Geometry g = geom(N, C, H, W, M, KH, KW, pad_h, pad_w, stride, dil, group);
    if (stride_w != stride || dil_w != dil) { fprintf(stderr, "square strides and dilations only\n"); return 2; }
    const escoin_conv_desc &d = g.d;
    std::vector<float> w((size_t)d.M * g.kdim);
    FILE *f = fopen(path.c_str(), "rb");
    if (!f || fread(w.data(), 4, w.size(), f) != w.size()) { fprintf(stderr, "%s: short or missing weights\n", path.c_str()); return 2; }
    fclose(f);
    CsrIndex rowptr(d.group), colidx(d.group);
    CsrValues values(d.group);
    long nnz = 0;
    for (int grp = 0; grp < d.group; ++grp) {
      rowptr[grp].assign(g.Mg + 1, 0);
      const float *A = w.data() + (size_t)grp * g.Mg * g.kdim;
      for (int i = 0; i < g.Mg; ++i) {
        for (int j = 0; j < g.kdim; ++j)
          if (A[(size_t)i * g.kdim + j] != 0) {
            values[grp].push_back(A[(size_t)i * g.kdim + j]);
            colidx[grp].push_back(j);
          }
        rowptr[grp][i + 1] = (int)colidx[grp].size();
      }
      nnz += (long)colidx[grp].size();
    }
    const float density = (float)((double)nnz / std::max<double>(1.0, (double)d.M * g.kdim));
    BodyLaunch bl;
    Tiling t;
    std::string info = "(no tiled layout)";
    jit::Program prog;
    JitLayout lay;
    if (kernel != ESCOIN_KERNEL_TILED) lay = jit_layout(g, density, 0, n_cu);
    if (lay.ok && jit_generate(g, density, 0, n_cu, &lay, rowptr, colidx, values, &prog)) {
      t = lay.t;
      bl.jit = true; bl.chained = prog.chained; bl.dma_in_code = lay.tab_len > 0;
      info = tiling_info(t, true, lay.nbuf, lds_bytes_for(t, 0, lay.nbuf, lay.tab_len), lay.tab_len, prog.chained);
    } else {
      const StreamLayout sl = stream_layout(g, density, 0, n_cu, rowptr, colidx, values);
      if (sl.ok) {
        t = sl.t;
        bl.stage_bytes = sl.stage_bytes;
        info = tiling_info(t, false, sl.nbuf, lds_bytes_for(t, sl.stage_bytes, sl.nbuf), 0, false);
      }
    }
    const unsigned long long in_image = (unsigned long long)d.C * d.H * d.W * 4;
    const int chunk = tiled_chunk(n_images, in_image, tiled_launch_range(0));
    const long launches = tiled_launches(n_images, chunk);
    int epi[2] = {0, 0}, variant[2] = {0, 0};
    const int n_launch[2] = {std::min(chunk, n_images), n_images - (int)(launches - 1) * chunk};      // the first and the last launch
    if (t.ok)
      for (int i = 0; i < 2; ++i) {
        const TiledLaunchShape ls = tiled_launch_shape(g, t, n_launch[i], d.group, bl.jit, 0, n_cu);
        bl.strided = strided_pointwise(g);
        bl.epi_store = ls.epi_store;
        bl.workgroups = (long)ls.grid_x * ls.grid_y;
        epi[i] = ls.epi_store ? 1 : 0;
        variant[i] = body_variant(g, t, bl, -1);
      }
    const LaunchVerdict tv = t.ok ? tiled_call_limits(g, t, n_images, d.group, 0) : LaunchVerdict();
    LaunchVerdict dv = dense_pixels_limit((long)n_images * g.OH * g.OW);
    if (dv.ok()) dv = dense_bytes_limit((unsigned long long)n_images * in_image, 16);
    const LaunchVerdict gv = generic_call_limits(g, n_images);
    printf("{\"case\": %d, \"tiling_info\": \"%s\", \"jit\": %d, \"chained\": %d, \"chunk\": %d, \"launches\": %ld, "
           "\"first_images\": %d, \"last_images\": %d, \"epi_store_first\": %d, \"epi_store_last\": %d, "
           "\"body_variant_first\": %d, \"body_variant_last\": %d, \"tiled_error\": \"%s\", \"dense_error\": \"%s\", \"generic_error\": \"%s\"}\n",
           n_cases++, info.c_str(), bl.jit ? 1 : 0, bl.chained ? 1 : 0, chunk, launches, n_launch[0], n_launch[1], epi[0], epi[1],
           variant[0], variant[1], tv.error, dv.error, gv.error);
    fflush(stdout);
  }
  return n_cases > 0 ? 0 : 2;
}

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "edges")) return edges();
  if (argc == 3 && !strcmp(argv[1], "cases")) return cases(argv[2]);
  fprintf(stderr, "usage: launch_limits_check edges | cases <manifest>\n");
  return 2;
}
