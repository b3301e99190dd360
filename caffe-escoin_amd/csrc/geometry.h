// geometry.h -- a layer's geometry as the library's host side sees it, and what follows from it alone.
// Pure C++ (no HIP), like stream_builder.h: escoin_plan.h includes it, align_rules.h builds on it.
#ifndef ESCOIN_GEOMETRY_H_
#define ESCOIN_GEOMETRY_H_

#include <cstddef>

#include "escoin.h"
#include "stream_builder.h"

namespace escoin {

// A kernel tap: column col = (ic * KH + kr) * KW + kc of a conv group's weight matrix (ic group-local).
struct Tap { int ic, kr, kc; };
inline Tap decode_tap(int col, int KH, int KW) { return Tap{col / (KW * KH), (col / KW) % KH, col % KW}; }
// A tap packed for the device tables (the generic kernel's taps; the gather kernel's ttap, with the group-local output
// channel in ic's place): ic << 16 | kr << 8 | kc
inline int pack_tap(const Tap &t) { return (int)(((unsigned)t.ic << 16) | ((unsigned)t.kr << 8) | (unsigned)t.kc); }

struct Geometry {
  escoin_conv_desc d;
  int OH, OW;
  int Cg, Mg;   // channels per group
  int kdim;     // kernel_dim_ = Cg*KH*KW
};

constexpr int kBwdChunkPixels = 1024;   // flattened (n, oh, ow) pixels per chunk of the weight-gradient reduction

constexpr size_t kLdsPerWorkgroup = 160 * 1024;

// Generated code may not exceed this many bytes per layer (a res5 layer at 60 % sparsity is ~45 MB).
constexpr size_t kMaxJitBytes = (size_t)512 << 20;

// 1x1 convolutions with stride 2 and no padding (ResNet-50's res{3,4,5}a_branch1 / branch2a) run on the pointwise
// path over a strided view of the bottom blob: even input rows only are staged, whole (a 16-byte DMA slot carries two
// outputs' inputs and two columns nobody uses: the HBM lines are the same either way), the walk accumulates all four
// columns of a lane's quad and the epilogue stores elements 0 and 2.  Needs an even input width (view rows then start
// on 16-byte boundaries; a row's last quad may hold a single output) and the asm epilogue (top blob < 2 GiB, checked
// at launch).
inline bool strided_pointwise(const Geometry &g) {
  return g.d.KH == 1 && g.d.KW == 1 && g.d.pad_h == 0 && g.d.pad_w == 0 && g.d.stride_h == 2 && g.d.stride_w == 2 &&
         g.d.dil_h == 1 && g.d.dil_w == 1 && g.d.W % 2 == 0 && g.OW * 2 == g.d.W;
}

inline ConvGeom to_geom(const Geometry &g) {
  ConvGeom c;
  c.N = g.d.N; c.C = g.d.C; c.H = g.d.H; c.W = g.d.W; c.M = g.d.M; c.KH = g.d.KH; c.KW = g.d.KW;
  c.pad_h = g.d.pad_h; c.pad_w = g.d.pad_w; c.group = g.d.group;
  c.OH = g.OH; c.OW = g.OW; c.Cg = g.Cg; c.Mg = g.Mg;
  if (strided_pointwise(g)) {
    // the view the kernel walks: OH rows (input rows 0, 2, ...) of the full input width, lanes over input quads
    c.sub = 2;
    c.H = g.OH; c.OH = g.OH;
    c.OW = g.d.W;
  }
  return c;
}

inline bool static_pad(const Geometry &g) {
  return (g.d.KW == 1 && g.d.pad_w == 0) || (g.d.KW == 3 && g.d.pad_w == 1) || (g.d.KW == 5 && g.d.pad_w == 2);
}

// LDS bytes of a tiled workgroup.  tab_len: entries of the quad table per tile parity (0: one channel plane)
inline size_t lds_bytes_for(const Tiling &t, int stage_bytes, int nbuf, int tab_len = 0) {
  const size_t buf = ((size_t)t.planes_bytes + 1023) / 1024 * 1024 + 1024;
  const size_t qpc = tab_len > 0 ? (size_t)tab_len : (size_t)t.plane_ch_floats / 4;     // (may include padding quads)
  return nbuf * (buf + (size_t)t.waves * stage_bytes) + 2 * qpc * 4 + (size_t)t.waves * t.n_icb * 4;
}

}  // namespace escoin

#endif  // ESCOIN_GEOMETRY_H_
