// tests/cpp/value_map_check.cpp -- the value maps of the generated code and of the weight stream (test code).
//
// escoin_update_values patches a plan's weights in place: into the literals and weight lines of the machine code
// jit_codegen.cpp generated, or into the quads of stream_builder.cpp's weight stream.  That is only right if the
// PATTERN alone shapes the code.  For every geometry below (the list of emulate_tiled.cpp, plus one whose units
// outgrow the weight lines) and for both builders:
//   1. the map has one entry per CSR entry, all distinct and in range;
//   2. code[val_word[e]] is the bit pattern of value e;
//   3. the code generated from other values B at the same pattern differs from A's ONLY at mapped words;
//   4. A's code patched through the map equals B's code word for word.
// B holds explicit zeros, a -0.0 and values of every magnitude: nothing may select an instruction by value.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "align_rules.h"
#include "jit_codegen.h"
#include "stream_builder.h"

using namespace escoin;

static unsigned rng_state = 4711;
static float frand() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return ((rng_state >> 8) & 0xFFFF) / 32768.0f - 1.0f;
}
static uint32_t bits_of(float v) {
  uint32_t u;
  std::memcpy(&u, &v, 4);
  return u;
}

struct Case { int N, C, H, W, M, KH, KW, ph, pw, group; float sparsity; int waves; int lds; int ncu = 1; int product = 0; };

// Cases with `product` set take the tiling and the generator's options of their generated-code run from the product's
// own layout rule (csrc/align_rules.h jit_layout) for a batch of 256 on 256 CUs instead of assembling them by hand;
// the value names the branch of the rule the case is there for, and missing it fails the case:
//   1 = 3x3 with more than one workgroup column (32 KiB planes), 2 = one column (64 KiB planes),
//   3 = three plane buffers (pointwise), 4 = two 4-wave workgroups per CU (pointwise)
static bool product_layout(const Case &cs, float density, Tiling *t, jit::Options *jo) {
  Geometry G{};
  G.d = escoin_conv_desc{cs.N, cs.C, cs.H, cs.W, cs.M, cs.KH, cs.KW, cs.ph, cs.pw, 1, 1, 1, 1, cs.group, 1, 0};
  G.OH = cs.H + 2 * cs.ph - cs.KH + 1;
  G.OW = cs.W + 2 * cs.pw - cs.KW + 1;
  G.Cg = cs.C / cs.group;
  G.Mg = cs.M / cs.group;
  G.kdim = G.Cg * cs.KH * cs.KW;
  const JitLayout lay = jit_layout(G, density, 256, 256);
  if (!lay.ok) { printf("product layout: the layer does not fit\n"); return false; }
  const bool hit = cs.product == 1 ? lay.t.n_ocblk > 1 && lay.budget == 32 * 1024 && lay.t.waves == 8
                 : cs.product == 2 ? lay.t.n_ocblk == 1 && lay.budget == 64 * 1024 && lay.nbuf == 2
                 : cs.product == 3 ? lay.nbuf == 3 && lay.jopt.dma.ahead == 2
                                   : lay.t.waves == 4 && lay.nbuf == 2;
  if (!hit) { printf("product layout: branch %d not taken (columns=%d budget=%d nbuf=%d waves=%d)\n", cs.product, lay.t.n_ocblk, lay.budget, lay.nbuf, lay.t.waves); return false; }
  *t = lay.t;
  *jo = lay.jopt;
  return true;
}


typedef std::vector<std::vector<int>> Idx;
typedef std::vector<std::vector<float>> Val;

// the four statements for one builder's output
static int check_map(const char *what, const std::vector<uint32_t> &a, const std::vector<uint32_t> &b,
                     const std::vector<std::vector<uint32_t>> &map, const Idx &ci, const Val &va, const Val &vb) {
  if (a.size() != b.size()) { printf("%s: %zu words from A, %zu from B\n", what, a.size(), b.size()); return 1; }
  if (map.size() != ci.size()) { printf("%s: map has %zu groups\n", what, map.size()); return 1; }
  std::vector<char> mapped(a.size(), 0);
  std::vector<uint32_t> patched = a;
  for (size_t cg = 0; cg < ci.size(); ++cg) {
    if (map[cg].size() != ci[cg].size()) { printf("%s: group %zu: %zu map entries for %zu nonzeros\n", what, cg, map[cg].size(), ci[cg].size()); return 1; }
    for (size_t e = 0; e < map[cg].size(); ++e) {
      const uint32_t w = map[cg][e];
      if (w >= a.size()) { printf("%s: entry %zu maps to word %u of %zu\n", what, e, w, a.size()); return 1; }
      if (mapped[w]) { printf("%s: word %u mapped twice\n", what, w); return 1; }
      mapped[w] = 1;
      if (a[w] != bits_of(va[cg][e])) { printf("%s: word %u holds %08x, value %zu is %08x\n", what, w, a[w], e, bits_of(va[cg][e])); return 1; }
      patched[w] = bits_of(vb[cg][e]);
    }
  }
  for (size_t w = 0; w < a.size(); ++w) {
    if (!mapped[w] && a[w] != b[w]) { printf("%s: unmapped word %zu differs between A and B (%08x / %08x)\n", what, w, a[w], b[w]); return 1; }
    if (patched[w] != b[w]) { printf("%s: patched word %zu is %08x, B has %08x\n", what, w, patched[w], b[w]); return 1; }
  }
  return 0;
}

static int run(const Case &cs, bool use_jit) {
  ConvGeom g{cs.N, cs.C, cs.H, cs.W, cs.M, cs.KH, cs.KW, cs.ph, cs.pw, cs.group, 0, 0, 0, 0};
  g.OH = cs.H + 2 * cs.ph - cs.KH + 1;
  g.OW = cs.W + 2 * cs.pw - cs.KW + 1;
  g.Cg = cs.C / cs.group;
  g.Mg = cs.M / cs.group;
  g.density = 1.0f - cs.sparsity;
  Tiling t = choose_tiling(g, cs.waves, cs.lds, cs.ncu, use_jit);
  if (!t.ok) { printf("tiling rejected\n"); return 2; }
  const int kdim = g.Cg * g.KH * g.KW;
  Idx rp(g.group), ci(g.group);
  Val va(g.group), vb(g.group);
  long nnz = 0;
  for (int cg = 0; cg < g.group; ++cg) {
    rp[cg].assign(g.Mg + 1, 0);
    for (int m = 0; m < g.Mg; ++m) {
      for (int j = 0; j < kdim; ++j) {
        const float r = frand();
        if (std::fabs(frand()) < cs.sparsity) continue;
        va[cg].push_back(r == 0 ? 0.5f : r);
        // B: another value at the same place -- every 11th an explicit zero, one -0.0, some huge, some tiny
        float b = frand() * (nnz % 5 == 0 ? 1e30f : nnz % 7 == 0 ? 1e-30f : 1.f);
        if (nnz % 11 == 3) b = 0.f;
        if (nnz == 1) b = -0.f;
        vb[cg].push_back(b);
        ci[cg].push_back(j);
        ++nnz;
      }
      rp[cg][m + 1] = (int)ci[cg].size();
    }
  }
  if (!use_jit) {
    const WeightStream a = build_stream(g, t, rp, ci, va), b = build_stream(g, t, rp, ci, vb);
    if (a.unit_hdr != b.unit_hdr || a.chan != b.chan || a.val_word != b.val_word) { printf("stream: headers, deal or map depend on the values\n"); return 1; }
    const int rc = check_map("stream", a.words, b.words, a.val_word, ci, va, vb);
    printf("stream %dx%d C=%d M=%d K=%dx%d g=%d: %ld nonzeros, %zu words %s\n", cs.H, cs.W, cs.C, cs.M, cs.KH, cs.KW, cs.group, nnz,
           a.words.size(), rc ? "FAILED" : "ok");
    return rc;
  }
  // (options as tests/cpp/emulate_tiled.cpp derives them from the case: both read-ahead depths, both weight placements,
  //  plane DMA with one and two fills in flight, chained and unchained units)
  jit::Options jo;
  if (cs.product && !product_layout(cs, g.density, &t, &jo)) return 2;
  if (!cs.product) {
    jo.depth = 1 + (cs.N & 1);
    jo.prio_rows = (cs.M & 1) ? 2 : 0;
    jo.hi_sets = (cs.N & 1) ? 24 : 0;
    jo.depth_one_tile = (cs.N & 1) ? 5 + cs.N % 9 : 5;
    jo.sweights = cs.KW != 1 && (cs.C & 3) != 1;
  }
  if (!cs.product && t.pix_waves == 1 && (t.waves == 8 || t.waves == 4)) {
    int padded = 0;
    jo.dma.period = jit::dma_period(t.plane_ch_floats / 4, 1 << 24, 0.0, &padded);
    jo.dma.on = jo.dma.period > 0 && padded == t.plane_ch_floats / 4;
    jo.dma.qpc = t.plane_ch_floats / 4;
    jo.dma.waves = t.waves;
    jo.dma.chan_bytes = (uint32_t)(cs.H * cs.W * 4);
    jo.dma.nt = (cs.N & 2) != 0;
    jo.dma.spread_pct = 40 + 10 * (cs.M % 5);
    jo.dma.ahead = (t.n_icb >= 2 && (cs.C & 1)) ? 2 : 1;
    jo.chain.on = jo.dma.on && (cs.H % 3 != 0);
    jo.chain.nbuf = jo.dma.ahead + 1;
    jo.chain.buf_bytes = (uint32_t)((t.planes_bytes + 1023) / 1024 * 1024 + 1024);
  }
  const jit::Program a = jit::build_program(g, t, rp, ci, va, jo), b = jit::build_program(g, t, rp, ci, vb, jo);
  if (a.overflow || b.overflow) { printf("jit: LDS offset overflow\n"); return 3; }
  if (a.unit_off != b.unit_off || a.chan != b.chan || a.val_word != b.val_word || a.n_pref != b.n_pref) { printf("jit: unit table, deal, map or touches depend on the values\n"); return 1; }
  const int rc = check_map("jit", a.code, b.code, a.val_word, ci, va, vb);
  // which form holds each value: the literal behind an s_mov_b32 (the word in front of it is the move), or a weight line
  long lit = 0, line = 0;
  for (const auto &m : a.val_word)
    for (uint32_t w : m) ((w > 0 && (a.code[w - 1] & 0xFF80FFFFu) == 0xBE8000FFu) ? lit : line)++;
  if (!jo.sweights && line) { printf("jit: %ld values outside a literal in code without weight lines\n", line); return 1; }
  printf("jit %dx%d C=%d M=%d K=%dx%d g=%d waves=%d%s: %ld nonzeros, %zu words, literals=%ld lines=%ld %s\n", cs.H, cs.W, cs.C, cs.M, cs.KH,
         cs.KW, cs.group, t.waves, a.chained ? " chained" : "", nnz, a.code.size(), lit, line, rc ? "FAILED" : "ok");
  return rc;
}

int main() {
  const Case cases[] = {
      {3, 8, 7, 7, 40, 3, 3, 1, 1, 1, 0.9f, 8, 65536},
      {2, 16, 14, 14, 24, 3, 3, 1, 1, 1, 0.9f, 8, 65536},
      {2, 6, 28, 28, 20, 3, 3, 1, 1, 1, 0.8f, 8, 8192},
      {2, 5, 56, 56, 16, 3, 3, 1, 1, 1, 0.9f, 8, 65536},
      {2, 5, 56, 56, 70, 3, 3, 1, 1, 1, 0.9f, 8, 65536},
      {2, 8, 27, 27, 16, 5, 5, 2, 2, 2, 0.8f, 8, 65536},
      {3, 12, 13, 13, 20, 3, 3, 1, 1, 2, 0.8f, 8, 65536},
      {2, 20, 12, 12, 50, 5, 5, 0, 0, 1, 0.5f, 8, 65536},
      {2, 24, 28, 28, 33, 1, 1, 0, 0, 1, 0.95f, 8, 65536},
      {1, 3, 20, 20, 8, 3, 3, 2, 2, 1, 0.5f, 8, 65536},
      {2, 4, 9, 70, 8, 3, 3, 1, 1, 1, 0.6f, 8, 65536},
      {1, 4, 5, 200, 4, 3, 1, 1, 0, 1, 0.5f, 8, 65536},
      {2, 4, 6, 6, 4, 2, 2, 1, 1, 1, 0.3f, 8, 65536},
      {1, 2, 4, 4, 3, 3, 3, 1, 1, 1, 0.0f, 8, 65536},
      {1, 2, 4, 4, 3, 3, 3, 1, 1, 1, 1.0f, 8, 65536},
      {5, 64, 7, 7, 48, 3, 3, 1, 1, 1, 0.5f, 8, 65536},
      {7, 40, 14, 14, 16, 1, 1, 0, 0, 1, 0.9f, 8, 65536},
      {5, 30, 7, 7, 48, 1, 1, 0, 0, 1, 0.9f, 8, 65536},
      {300, 6, 7, 7, 12, 1, 1, 0, 0, 1, 0.8f, 8, 65536},
      {3, 6, 13, 13, 10, 1, 1, 0, 0, 2, 0.7f, 8, 65536},
      {3, 8, 21, 6, 7, 5, 5, 4, 4, 1, 0.9f, 8, 65536},
      {2, 4, 5, 7, 6, 3, 3, 2, 2, 1, 0.5f, 8, 65536},
      {2, 5, 56, 56, 70, 3, 3, 1, 1, 1, 0.9f, 8, 65536, 256},
      {5, 30, 7, 7, 48, 1, 1, 0, 0, 1, 0.9f, 8, 65536, 256},
      {40, 16, 7, 7, 64, 1, 1, 0, 0, 1, 0.9f, 8, 65536, 8},
      {1, 48, 56, 56, 64, 1, 1, 0, 0, 1, 0.97f, 8, 65536, 256},
      {32, 300, 14, 14, 256, 1, 1, 0, 0, 1, 0.95f, 8, 65536, 32},
      {16, 400, 7, 7, 384, 1, 1, 0, 0, 1, 0.97f, 8, 65536, 16},
      {16, 10, 4, 4, 300, 1, 1, 0, 0, 1, 0.8f, 8, 65536, 16},
      {2, 21, 14, 14, 16, 3, 3, 1, 1, 1, 0.8f, 8, 16384},
      {3, 24, 28, 28, 64, 3, 3, 1, 1, 1, 0.9f, 8, 16384},
      {5, 33, 14, 14, 32, 1, 1, 0, 0, 1, 0.9f, 8, 8192},
      {4, 45, 7, 7, 24, 3, 3, 1, 1, 1, 0.85f, 8, 8192},
      {3, 20, 56, 56, 8, 3, 3, 1, 1, 1, 0.9f, 8, 32768},
      {9, 37, 7, 7, 64, 1, 1, 0, 0, 1, 0.9f, 8, 4096, 256},
      {4, 48, 28, 28, 64, 1, 1, 0, 0, 1, 0.95f, 4, 32768, 4},
      {3, 40, 28, 28, 96, 1, 1, 0, 0, 1, 0.9f, 4, 8192, 2},
      {2, 21, 14, 14, 16, 3, 3, 1, 1, 1, 0.8f, 4, 16384},
      {3, 30, 28, 28, 128, 1, 1, 0, 0, 1, 0.9f, 4, 32768, 1},
      {2, 26, 28, 28, 176, 1, 1, 0, 0, 1, 0.93f, 4, 8192, 1},
      // multi-threaded chains (>= 20000 nonzeros: the chains are generated on threads and put together, offsets rebased)
      {2, 128, 14, 14, 128, 3, 3, 1, 1, 1, 0.8f, 8, 65536},
      // tiny images, the whole layer in one block: units of more than 30 000 nonzeros keep their literal moves while the
      // other units of the same program use weight lines
      {1, 900, 2, 2, 380, 3, 3, 1, 1, 1, 0.05f, 8, 65536},
      // tiling and options from the product's layout rule (product_layout above)
      {2, 40, 14, 14, 80, 3, 3, 1, 1, 1, 0.9f, 8, 65536, 256, 1},
      {2, 5, 56, 56, 16, 3, 3, 1, 1, 1, 0.9f, 8, 65536, 256, 2},
      {3, 120, 14, 14, 24, 1, 1, 0, 0, 1, 0.95f, 8, 65536, 256, 3},
      {3, 24, 28, 28, 16, 1, 1, 0, 0, 1, 0.95f, 8, 65536, 256, 4},
  };
  int bad = 0;
  for (const Case &c : cases) {
    bad += run(c, false) != 0;
    bad += run(c, true) != 0;
  }
  printf(bad ? "FAILED %d case(s)\n" : "all cases OK\n", bad);
  return bad ? 1 : 0;
}
