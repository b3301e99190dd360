// aligned_form.cpp -- the persisted aligned form's byte layout: sizes, writers, parsers (aligned_form.h).  Host only.
#include "aligned_form.h"

#include <algorithm>
#include <cstring>

namespace escoin {

// ---- the outer container ---------------------------------------------------------------------------------------------
static inline uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
uint64_t content_tag(const void *data, size_t n, uint64_t seed) {
  const uint64_t P1 = 0x9E3779B185EBCA87ull, P2 = 0xC2B2AE3D27D4EB4Full, P3 = 0x165667B19E3779F9ull;
  const unsigned char *p = static_cast<const unsigned char *>(data);
  uint64_t v[4] = {seed + P1 + P2, seed + P2, seed, seed - P1};
  size_t i = 0;
  for (; i + 32 <= n; i += 32)
    for (int k = 0; k < 4; ++k) {
      uint64_t w;
      memcpy(&w, p + i + 8 * k, 8);
      v[k] = rotl64(v[k] + w * P2, 31) * P1;
    }
  uint64_t h = rotl64(v[0], 1) + rotl64(v[1], 7) + rotl64(v[2], 12) + rotl64(v[3], 18) + (uint64_t)n;
  for (; i < n; ++i) h = rotl64(h ^ (p[i] * P3), 11) * P1;
  h ^= h >> 33; h *= P2; h ^= h >> 29; h *= P3; h ^= h >> 32;
  return h;
}
uint64_t pair_tag_of(uint64_t csr_tag, uint64_t jit_tag) {
  const uint64_t both[2] = {csr_tag, jit_tag};
  return content_tag(both, sizeof(both), 0x6573636F696E3236ull);
}

// [nnz_per_group][rowptr][colidx][values]
static size_t csr_arrays_bytes(const Geometry &g, uint64_t nnz) {
  return 4 * (size_t)g.d.group + 4 * (size_t)g.d.group * (g.Mg + 1) + 8 * (size_t)nnz;
}

size_t aligned_bytes(const Geometry &g, uint64_t nnz, size_t code_section_bytes) {
  return sizeof(AlignedHdr) + sizeof(escoin_conv_desc) + csr_arrays_bytes(g, nnz) + code_section_bytes;
}

void aligned_write(const Geometry &g, const CsrIndex &rowptr, const CsrIndex &colidx, const CsrValues &values,
                   const std::vector<char> &code_section, void *buf) {
  uint64_t nnz = 0;
  for (int grp = 0; grp < g.d.group; ++grp) nnz += colidx[grp].size();
  AlignedHdr h{kAlignedMagic, kAlignedVersion, (uint64_t)aligned_bytes(g, nnz, code_section.size()), nnz, (uint64_t)code_section.size(), 0, 0, 0};
  char *const hdr_at = static_cast<char *>(buf);
  char *q = hdr_at + sizeof(h);
  const char *const csr_at = q;
  auto put = [&](const void *src, size_t n) {
    if (n) memcpy(q, src, n);
    q += n;
  };
  put(&g.d, sizeof(g.d));
  for (int grp = 0; grp < g.d.group; ++grp) { const int n = (int)colidx[grp].size(); put(&n, 4); }
  for (int grp = 0; grp < g.d.group; ++grp) put(rowptr[grp].data(), 4 * (size_t)(g.Mg + 1));
  for (int grp = 0; grp < g.d.group; ++grp) put(colidx[grp].data(), 4 * colidx[grp].size());
  for (int grp = 0; grp < g.d.group; ++grp) put(values[grp].data(), 4 * values[grp].size());
  h.csr_tag = content_tag(csr_at, (size_t)(q - csr_at), 1);
  const char *const jit_at = q;
  put(code_section.data(), code_section.size());
  h.jit_tag = content_tag(jit_at, code_section.size(), 2);
  h.pair_tag = pair_tag_of(h.csr_tag, h.jit_tag);
  memcpy(hdr_at, &h, sizeof(h));
}

AlignedForm aligned_parse(const void *buf, size_t bytes, const Geometry &g) {
  AlignedForm f;
  auto refuse = [&](const char *msg) {
    f.rc = ESCOIN_EINVAL;
    f.error = msg;
    return f;
  };
  AlignedHdr h;
  if (bytes < sizeof(h) + sizeof(escoin_conv_desc)) return refuse("import_aligned: truncated blob");
  const char *q = static_cast<const char *>(buf);
  memcpy(&h, q, sizeof(h)); q += sizeof(h);
  if (h.magic != kAlignedMagic || h.version != kAlignedVersion || h.total_bytes != bytes)
    return refuse("import_aligned: not an aligned-form blob of this library build");
  escoin_conv_desc &d = f.d;
  memcpy(&d, q, sizeof(d)); q += sizeof(d);
  if (d.C != g.d.C || d.M != g.d.M || d.KH != g.d.KH || d.KW != g.d.KW || d.group != g.d.group)
    return refuse("import_aligned: the blob was exported for other weights (C / M / kernel / group differ)");
  // (bounded before it sizes anything: a layer has at most group * Mg * kdim weights)
  if (h.nnz > (uint64_t)g.d.group * (uint64_t)g.Mg * (uint64_t)g.kdim || h.jit_bytes > bytes)
    return refuse("import_aligned: nnz or code section larger than the layer / the blob");
  const size_t csr_bytes = csr_arrays_bytes(g, h.nnz);
  if (sizeof(h) + sizeof(d) + csr_bytes + h.jit_bytes != bytes) return refuse("import_aligned: section sizes do not add up");
  {
    // the content tags, before a single byte of either section is trusted
    const char *csr_at = static_cast<const char *>(buf) + sizeof(h);
    const size_t csr_sec = sizeof(d) + csr_bytes;
    const uint64_t ct = content_tag(csr_at, csr_sec, 1), jt = content_tag(csr_at + csr_sec, (size_t)h.jit_bytes, 2);
    if (ct != h.csr_tag || jt != h.jit_tag || pair_tag_of(ct, jt) != h.pair_tag)
      return refuse("import_aligned: content tag mismatch -- the blob is torn, or its code section does not belong to its CSR section");
  }
  auto take = [&](auto &v, size_t n) {
    v.resize(n);
    if (n) memcpy(v.data(), q, 4 * n);
    q += 4 * n;
  };
  take(f.nnz_per_group, (size_t)g.d.group);
  take(f.rowptr, (size_t)g.d.group * (g.Mg + 1));
  take(f.colidx, (size_t)h.nnz);
  take(f.values, (size_t)h.nnz);
  uint64_t sum = 0;
  for (int n : f.nnz_per_group) sum += (uint64_t)std::max(0, n);
  if (sum != h.nnz) return refuse("import_aligned: nnz_per_group does not match the blob's nnz");
  f.same_geom = d.H == g.d.H && d.W == g.d.W && d.pad_h == g.d.pad_h && d.pad_w == g.d.pad_w &&
                d.stride_h == g.d.stride_h && d.stride_w == g.d.stride_w && d.dil_h == g.d.dil_h &&
                d.dil_w == g.d.dil_w && d.N == g.d.N;
  f.code_section = q;
  f.code_section_bytes = (size_t)h.jit_bytes;
  return f;
}

// ---- the code section --------------------------------------------------------------------------------------------------
// The Tiling as int32s: ok, band_mode, then these in this order.
#define ESC_TILING_INTS(X) X(KW) X(KH) X(H) X(W) X(OH) X(OW) X(S4) X(RS) X(rows_per_slab) X(pix_waves) X(oc_waves) \
  X(waves) X(G) X(n_ocg) X(n_ocblk) X(tpl) X(rows_per_wg) X(tr) X(nseg) X(bands) X(plane_rows) X(plane_seg_floats)  \
  X(plane_ch_floats) X(icb) X(n_icb) X(planes_bytes)
#define X(f) +1
// (a field added to Tiling and forgotten above would silently not be persisted: it breaks the build here instead)
static_assert(2 ESC_TILING_INTS(X) == kTilingInts && sizeof(Tiling) == 4 * kTilingInts,
              "ESC_TILING_INTS must list every field of Tiling: a new field changes the persisted form (bump kAlignedJitVersion)");
#undef X

static void tiling_to_ints(const Tiling &t, int32_t *v) {
  int i = 0;
  v[i++] = t.ok ? 1 : 0;
  v[i++] = t.band_mode ? 1 : 0;
#define X(f) v[i++] = (int32_t)t.f;
  ESC_TILING_INTS(X)
#undef X
}
static Tiling tiling_from_ints(const int32_t *v) {
  Tiling t;
  int i = 0;
  t.ok = v[i++] != 0;
  t.band_mode = v[i++] != 0;
#define X(f) t.f = v[i++];
  ESC_TILING_INTS(X)
#undef X
  return t;
}

std::vector<char> code_section_write(const CodeSection &s, int n_cu, const std::string &isa) {
  int32_t ti[kTilingInts];
  tiling_to_ints(s.tiling, ti);
  AlignedJitHdr h;
  memset(&h, 0, sizeof(h));
  h.magic = kAlignedJitMagic; h.version = kAlignedJitVersion; h.n_cu = (uint32_t)n_cu;
  h.n_tiling_ints = (uint32_t)kTilingInts;
  h.nbuf = s.nbuf; h.jit_pref = s.jit_pref; h.dma_period = s.dma_period; h.lds_budget = s.lds_budget;
  h.tiling_batch = s.tiling_batch; h.density = s.density; h.jit_chain = s.chained ? 1 : 0;
  h.jit_self_zero = 1; h.reserved0 = 0;
  h.n_dense_groups = s.n_dense_groups; h.dense_mask = s.dense_mask;
  strncpy(h.isa, isa.c_str(), sizeof(h.isa) - 1);
  h.jit_rows = s.jit_rows; h.jit_records = s.jit_records;
  h.code_bytes = s.code.size() * 4; h.reserved1 = 0;
  h.n_unit_off = s.unit_off.size(); h.n_chan = s.chan.size();
  std::vector<char> out(sizeof(h) + sizeof(ti) + 4 * (s.unit_off.size() + s.chan.size() + s.code.size()));
  char *q = out.data();
  auto put = [&](const void *src, size_t n) {
    if (n) memcpy(q, src, n);
    q += n;
  };
  put(&h, sizeof(h));
  put(ti, sizeof(ti));
  put(s.unit_off.data(), s.unit_off.size() * 4);
  put(s.chan.data(), s.chan.size() * 4);
  put(s.code.data(), s.code.size() * 4);
  return out;
}

bool code_section_parse(const char *blob, size_t bytes, const Geometry &g, const CodeFit &fit, CodeSection *s) {
  AlignedJitHdr h;
  if (bytes < sizeof(h)) return false;
  memcpy(&h, blob, sizeof(h));
  if (h.magic != kAlignedJitMagic || h.version != kAlignedJitVersion || h.n_cu != (uint32_t)fit.n_cu ||
      h.tiling_batch != fit.tiling_batch)
    return false;
  // the dense / sparse split of the conv groups is part of the code (dense groups have empty units): it must be the
  // split the importing plan's options (dense_threshold_pct, dense_gate, conv_mode ...) give
  if (h.n_dense_groups != fit.n_dense_groups || h.dense_mask != fit.dense_mask) return false;
  h.isa[sizeof(h.isa) - 1] = 0;
  if (fit.isa.compare(0, sizeof(h.isa) - 1, h.isa) != 0) return false;
  // every count below is bounded before anything is allocated or indexed with it
  const uint64_t max_units = (uint64_t)g.d.group * g.Mg * g.Cg, max_chan = (uint64_t)g.d.group * g.Mg * 64;
  if (h.n_unit_off > max_units || h.n_chan > max_chan || h.code_bytes > bytes || (h.code_bytes & 3) || h.code_bytes == 0 || h.code_bytes > kMaxJitBytes) return false;
  const size_t need = sizeof(h) + (size_t)h.n_tiling_ints * 4 + (size_t)(h.n_unit_off + h.n_chan) * 4 + (size_t)h.code_bytes;
  if (h.n_tiling_ints != (uint32_t)kTilingInts || need != bytes) return false;
  const char *q = blob + sizeof(h);
  int32_t ti[kTilingInts];
  memcpy(ti, q, sizeof(ti)); q += sizeof(ti);
  const Tiling t = tiling_from_ints(ti);
  // the tiling must be one of THIS geometry (a re-cut pointwise image keeps H * W) and fit the device
  const long view_pixels = strided_pointwise(g) ? (long)g.OH * g.d.W : (long)g.d.H * g.d.W;
  // (ranges first: the checks after them divide by these fields.  The fields come from the blob: sums and products of
  //  fields that have only a lower bound yet are taken in 64 bits; the waves are bounded before their product -- a
  //  workgroup has at most kTiledWaves)
  if (t.S4 < 2 || t.S4 > 64 || (t.S4 & (t.S4 - 1)) || t.RS != 4 * t.S4 || t.rows_per_slab != 64 / t.S4 || t.oc_waves < 1 ||
      t.oc_waves > kTiledWaves || t.pix_waves < 1 || t.pix_waves > kTiledWaves || t.oc_waves * t.pix_waves != t.waves ||
      (t.tpl != 1 && t.tpl != 2) || t.G < 1 || t.G > 48 || t.icb < 1 ||
      t.n_icb < 1 || t.tr < 1 || t.nseg < 1 || t.bands < 1 || t.H < 1 || t.W < 1 || t.W > 256 || t.OH < 1 || t.OW < 1 ||
      (long)t.plane_rows != (long)t.tr + t.KH - 1 || (long)t.plane_seg_floats != (long)t.plane_rows * t.RS || t.plane_ch_floats < 8 ||
      t.plane_ch_floats > 16384 || (t.plane_ch_floats & 3) || (long)t.planes_bytes != (long)t.icb * t.plane_ch_floats * 4 ||
      t.planes_bytes > 64 * 1024 || t.rows_per_wg != t.pix_waves * t.tpl * t.rows_per_slab ||
      (long)t.n_ocblk != ((long)t.n_ocg + t.oc_waves - 1) / t.oc_waves || h.jit_pref < 0 || h.jit_pref > 4096 || h.dma_period > 65536)
    return false;
  if (!t.ok || t.KW != g.d.KW || t.KH != g.d.KH || (long)t.H * t.W != view_pixels || (t.waves != kTiledWaves && t.waves != 4) ||
      t.G < 1 || t.n_ocg != (g.Mg + t.G - 1) / t.G || t.icb < 1 || (long)t.n_icb != ((long)g.Cg + t.icb - 1) / t.icb ||
      (h.nbuf != 2 && h.nbuf != 3) || h.jit_self_zero != 1 || (h.jit_chain && (h.dma_period <= 0 || t.n_ocg % t.oc_waves != 0)) || h.n_unit_off != (uint64_t)g.d.group * t.n_ocg * t.n_icb ||
      h.n_chan != (uint64_t)g.d.group * t.n_ocg * t.G || h.dma_period < 0 ||
      lds_bytes_for(t, 0, h.nbuf, h.dma_period) > kLdsPerWorkgroup)
    return false;
  s->unit_off.resize((size_t)h.n_unit_off);
  s->chan.resize((size_t)h.n_chan);
  if (h.n_unit_off) memcpy(s->unit_off.data(), q, s->unit_off.size() * 4);
  q += s->unit_off.size() * 4;
  if (h.n_chan) memcpy(s->chan.data(), q, s->chan.size() * 4);
  q += s->chan.size() * 4;
  for (uint32_t o : s->unit_off) if ((uint64_t)o >= h.code_bytes) return false;
  for (uint32_t ch : s->chan) if ((int)ch >= g.Mg) return false;
  s->code.resize((size_t)(h.code_bytes / 4));
  memcpy(s->code.data(), q, (size_t)h.code_bytes);
  s->tiling = t;
  s->nbuf = h.nbuf; s->jit_pref = h.jit_pref; s->dma_period = h.dma_period; s->lds_budget = h.lds_budget;
  s->tiling_batch = h.tiling_batch; s->chained = h.jit_chain != 0; s->density = h.density;
  s->n_dense_groups = h.n_dense_groups; s->dense_mask = h.dense_mask;
  s->jit_rows = (long)h.jit_rows; s->jit_records = (long)h.jit_records;
  return true;
}

}  // namespace escoin
