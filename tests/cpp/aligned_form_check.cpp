// tests/cpp/aligned_form_check.cpp -- the persisted aligned form (csrc/aligned_form.h) on the host alone (test code).
//
// Compiled with plain g++ against aligned_form.cpp, align_rules.cpp, stream_builder.cpp and jit_codegen.cpp, no ROCm
// include path, with -fsanitize=address,undefined: the parsers take bytes another process wrote, so besides what they
// answer the run proves that no input of the enumerated set makes them read out of bounds, overflow a signed int or
// allocate from a count they did not bound.  Arguments: the golden blobs (tests/golden/aligned_form_*.bin).  Prints
// one "OK <case>" line per case; anything else is a failure (exit status 1 at the first one).
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <iterator>
#include <string>
#include <vector>

#include "aligned_form.h"

using namespace escoin;

#define REQUIRE(cond, ...)                                  \
  do {                                                      \
    if (!(cond)) {                                          \
      printf("FAIL %s:%d %s -- ", __FILE__, __LINE__, #cond); \
      printf(__VA_ARGS__);                                  \
      printf("\n");                                         \
      exit(1);                                              \
    }                                                       \
  } while (0)

typedef std::vector<char> Bytes;

static Geometry geometry_of(const escoin_conv_desc &d) {
  Geometry g;
  g.d = d;
  g.OH = (d.H + 2 * d.pad_h - (d.dil_h * (d.KH - 1) + 1)) / d.stride_h + 1;
  g.OW = (d.W + 2 * d.pad_w - (d.dil_w * (d.KW - 1) + 1)) / d.stride_w + 1;
  g.Cg = d.C / d.group;
  g.Mg = d.M / d.group;
  g.kdim = g.Cg * d.KH * d.KW;
  return g;
}
static Geometry geometry(int N, int C, int HW, int M, int K, int pad, int group) {
  escoin_conv_desc d;
  memset(&d, 0, sizeof(d));
  d.N = N; d.C = C; d.H = d.W = HW; d.M = M; d.KH = d.KW = K; d.pad_h = d.pad_w = pad;
  d.stride_h = d.stride_w = d.dil_h = d.dil_w = 1; d.group = group;
  return geometry_of(d);
}

template <typename T>
static T read_at(const Bytes &b, size_t off) {
  T v;
  REQUIRE(off + sizeof(T) <= b.size(), "read at %zu", off);
  memcpy(&v, b.data() + off, sizeof(T));
  return v;
}
template <typename T>
static void write_at(Bytes &b, size_t off, const T &v) {
  REQUIRE(off + sizeof(T) <= b.size(), "write at %zu", off);
  memcpy(b.data() + off, &v, sizeof(T));
}

// what the exporter recorded about its device and plan: the fit under which its own section is accepted
static CodeFit fit_of(const AlignedJitHdr &h) {
  CodeFit fit;
  char isa[sizeof(h.isa) + 1] = {0};
  memcpy(isa, h.isa, sizeof(h.isa));
  fit.n_cu = (int)h.n_cu; fit.isa = isa; fit.tiling_batch = h.tiling_batch;
  fit.n_dense_groups = h.n_dense_groups; fit.dense_mask = h.dense_mask;
  return fit;
}

// the parser on an exact-size heap copy of the first n bytes: a read past them is the sanitizer's to report
static bool parse_copy(const Bytes &sec, size_t n, const Geometry &g, const CodeFit &fit, CodeSection *s) {
  Bytes exact(sec.begin(), sec.begin() + (ptrdiff_t)n);
  return code_section_parse(exact.data(), exact.size(), g, fit, s);
}

static bool same_tiling(const Tiling &a, const Tiling &b) {
  int32_t x[kTilingInts], y[kTilingInts];
  static_assert(sizeof(x) == sizeof(Tiling), "28 ints");
  // (field by field through the serialisation: Tiling has padding bytes behind its bools)
  CodeSection sa, sb;
  sa.tiling = a; sb.tiling = b;
  const Bytes wa = code_section_write(sa, 1, ""), wb = code_section_write(sb, 1, "");
  memcpy(x, wa.data() + sizeof(AlignedJitHdr), sizeof(x));
  memcpy(y, wb.data() + sizeof(AlignedJitHdr), sizeof(y));
  return memcmp(x, y, sizeof(x)) == 0;
}
static bool same_section(const CodeSection &a, const CodeSection &b) {
  return same_tiling(a.tiling, b.tiling) && a.nbuf == b.nbuf && a.jit_pref == b.jit_pref && a.dma_period == b.dma_period &&
         a.lds_budget == b.lds_budget && a.tiling_batch == b.tiling_batch && a.chained == b.chained &&
         memcmp(&a.density, &b.density, 4) == 0 && a.n_dense_groups == b.n_dense_groups && a.dense_mask == b.dense_mask &&
         a.jit_rows == b.jit_rows && a.jit_records == b.jit_records && a.unit_off == b.unit_off && a.chan == b.chan &&
         a.code == b.code;
}

// the CSR pieces of a parsed blob, per conv group as aligned_write takes them
static void split_groups(const AlignedForm &f, const Geometry &g, CsrIndex *rp, CsrIndex *ci, CsrValues *va) {
  size_t at = 0;
  for (int grp = 0; grp < g.d.group; ++grp) {
    const size_t n = (size_t)f.nnz_per_group[grp];
    rp->emplace_back(f.rowptr.begin() + (ptrdiff_t)grp * (g.Mg + 1), f.rowptr.begin() + (ptrdiff_t)(grp + 1) * (g.Mg + 1));
    ci->emplace_back(f.colidx.begin() + (ptrdiff_t)at, f.colidx.begin() + (ptrdiff_t)(at + n));
    va->emplace_back(f.values.begin() + (ptrdiff_t)at, f.values.begin() + (ptrdiff_t)(at + n));
    at += n;
  }
}

// ---- golden round trip -------------------------------------------------------------------------------------------------
static void golden(const char *path) {
  std::ifstream in(path, std::ios::binary);
  const Bytes blob((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  REQUIRE(blob.size() > sizeof(AlignedHdr) + sizeof(escoin_conv_desc), "%s: missing or short", path);
  const std::string name = std::string(path).substr(std::string(path).find_last_of('/') + 1);
  const Geometry g = geometry_of(read_at<escoin_conv_desc>(blob, sizeof(AlignedHdr)));
  const AlignedForm f = aligned_parse(blob.data(), blob.size(), g);
  REQUIRE(f.rc == ESCOIN_OK && f.same_geom && f.code_section_bytes > sizeof(AlignedJitHdr), "%s: %s", path, f.error.c_str());
  const Bytes sec(f.code_section, f.code_section + f.code_section_bytes);
  const AlignedJitHdr jh = read_at<AlignedJitHdr>(sec, 0);
  CodeSection s;
  REQUIRE(parse_copy(sec, sec.size(), g, fit_of(jh), &s), "%s: its own fit is refused", path);
  printf("OK golden %s parse\n", name.c_str());
  const Bytes sec2 = code_section_write(s, (int)jh.n_cu, fit_of(jh).isa);
  REQUIRE(sec2 == sec, "%s: code section rewritten differs", path);
  CsrIndex rp, ci;
  CsrValues va;
  split_groups(f, g, &rp, &ci, &va);
  REQUIRE(aligned_bytes(g, f.colidx.size(), sec2.size()) == blob.size(), "%s: size", path);
  Bytes again(blob.size());
  aligned_write(g, rp, ci, va, sec2, again.data());
  REQUIRE(again == blob, "%s: blob rewritten differs", path);
  printf("OK golden %s rewrite\n", name.c_str());
}

// ---- programs generated on the host ------------------------------------------------------------------------------------
struct Export {
  std::string name;
  Geometry g;
  CsrIndex rowptr, colidx;
  CsrValues values;
  CodeSection s;
  CodeFit fit;
  Bytes sec, blob;
};
constexpr int kCus = 256;
static const char *const kIsa = "gfx950:sramecc+:xnack-";

// One weight in ten, by a fixed rule of (row, column); scale distinguishes two exports of one pattern.
static Export make_export(const char *name, const Geometry &g, float scale) {
  Export e;
  e.name = name;
  e.g = g;
  const int G = g.d.group;
  e.rowptr.resize(G); e.colidx.resize(G); e.values.resize(G);
  long nnz = 0;
  for (int grp = 0; grp < G; ++grp) {
    e.rowptr[grp].assign(g.Mg + 1, 0);
    for (int i = 0; i < g.Mg; ++i) {
      for (int j = 0; j < g.kdim; ++j)
        if ((i * 7 + j * 13 + grp * 3) % 10 == 0) {
          e.colidx[grp].push_back(j);
          e.values[grp].push_back(scale * 0.25f * (float)(1 + (i + 2 * j) % 5) * ((i + j) % 2 ? -1.f : 1.f));
        }
      e.rowptr[grp][i + 1] = (int)e.colidx[grp].size();
    }
    nnz += (long)e.colidx[grp].size();
  }
  const int tiling_batch = g.d.N;
  const float density = (float)((double)nnz / ((double)g.Mg * G * g.kdim));
  JitLayout lay = jit_layout(g, density, tiling_batch, kCus);
  REQUIRE(lay.ok, "%s: jit_layout", name);
  jit::Program prog;
  REQUIRE(jit_generate(g, density, tiling_batch, kCus, &lay, e.rowptr, e.colidx, e.values, &prog), "%s: jit_generate", name);
  // as sconv_tiled.hip's tiled_build / tiled_export fill it
  CodeSection &s = e.s;
  s.tiling = lay.t;
  s.nbuf = lay.nbuf; s.jit_pref = lay.jopt.prefetch ? prog.n_pref : 0; s.dma_period = lay.tab_len; s.lds_budget = lay.budget;
  s.tiling_batch = tiling_batch; s.chained = prog.chained; s.density = density;
  s.jit_rows = prog.n_rows; s.jit_records = prog.n_records;
  s.unit_off = prog.unit_off; s.chan = prog.chan; s.code = prog.code;
  e.fit.n_cu = kCus; e.fit.isa = kIsa; e.fit.tiling_batch = tiling_batch;
  e.sec = code_section_write(s, kCus, kIsa);
  e.blob.resize(aligned_bytes(g, (uint64_t)nnz, e.sec.size()));
  aligned_write(g, e.rowptr, e.colidx, e.values, e.sec, e.blob.data());
  return e;
}

static void host_round_trip(const Export &e) {
  const AlignedForm f = aligned_parse(e.blob.data(), e.blob.size(), e.g);
  REQUIRE(f.rc == ESCOIN_OK && f.same_geom, "%s: %s", e.name.c_str(), f.error.c_str());
  REQUIRE(memcmp(&f.d, &e.g.d, sizeof(f.d)) == 0, "%s: descriptor", e.name.c_str());
  CsrIndex rp, ci;
  CsrValues va;
  split_groups(f, e.g, &rp, &ci, &va);
  REQUIRE(rp == e.rowptr && ci == e.colidx && va == e.values, "%s: CSR", e.name.c_str());
  REQUIRE(f.code_section_bytes == e.sec.size() && memcmp(f.code_section, e.sec.data(), e.sec.size()) == 0, "%s: section", e.name.c_str());
  CodeSection s;
  REQUIRE(parse_copy(e.sec, e.sec.size(), e.g, e.fit, &s), "%s: refused", e.name.c_str());
  REQUIRE(same_section(s, e.s), "%s: a field or vector differs", e.name.c_str());
  printf("OK host %s fields\n", e.name.c_str());
  const Bytes sec2 = code_section_write(s, kCus, kIsa);
  Bytes again(e.blob.size());
  aligned_write(e.g, rp, ci, va, sec2, again.data());
  REQUIRE(sec2 == e.sec && again == e.blob, "%s: rewritten differs", e.name.c_str());
  printf("OK host %s rewrite\n", e.name.c_str());
}

// each mismatch between the exporter's record and the importer's device / plan, alone: "does not fit"
static void mismatches(const Export &e) {
  CodeSection s;
  const struct { const char *name; std::function<void(CodeFit &)> change; } cases[] = {
      {"n_cu", [](CodeFit &f) { f.n_cu = 304; }},
      {"isa", [](CodeFit &f) { f.isa = "gfx942:sramecc+:xnack-"; }},
      {"tiling_batch", [](CodeFit &f) { f.tiling_batch += 1; }},
      {"n_dense_groups", [](CodeFit &f) { f.n_dense_groups = 1; }},
      {"dense_mask", [](CodeFit &f) { f.dense_mask = 1; }},
  };
  for (const auto &c : cases) {
    CodeFit fit = e.fit;
    c.change(fit);
    REQUIRE(!parse_copy(e.sec, e.sec.size(), e.g, fit, &s), "%s accepted", c.name);
    REQUIRE(parse_copy(e.sec, e.sec.size(), e.g, e.fit, &s), "%s: the unchanged fit refused", c.name);
    printf("OK nofit %s\n", c.name);
  }
}

// ---- the outer container -------------------------------------------------------------------------------------------------
static void refused(const char *name, const Bytes &blob, const Geometry &g, const char *message) {
  const AlignedForm f = aligned_parse(blob.data(), blob.size(), g);
  REQUIRE(f.rc == ESCOIN_EINVAL, "%s: rc %d", name, f.rc);
  REQUIRE(f.error.find(message) != std::string::npos, "%s: message '%s'", name, f.error.c_str());
  printf("OK outer %s\n", name);
}

static void outer(const Export &a, const Export &b) {
  const AlignedHdr h = read_at<AlignedHdr>(a.blob, 0);
  const size_t jit_at = a.blob.size() - (size_t)h.jit_bytes;
  Bytes bad = a.blob;
  bad[jit_at - 4 * (size_t)h.nnz + 2] ^= 0x40;
  refused("flip_values", bad, a.g, "content tag");
  bad = a.blob;
  bad[jit_at + (size_t)h.jit_bytes / 2] ^= 0x01;
  refused("flip_code", bad, a.g, "content tag");
  // A's CSR, B's code with B's (valid) code tag; the pair tag is still A's
  REQUIRE(b.blob.size() == a.blob.size() && b.sec.size() == a.sec.size() && b.sec != a.sec, "splice: the exports must differ in values only");
  bad = a.blob;
  memcpy(bad.data() + jit_at, b.blob.data() + jit_at, (size_t)h.jit_bytes);
  write_at(bad, offsetof(AlignedHdr, jit_tag), read_at<AlignedHdr>(b.blob, 0).jit_tag);
  REQUIRE(content_tag(bad.data() + jit_at, (size_t)h.jit_bytes, 2) == read_at<AlignedHdr>(bad, 0).jit_tag, "splice: code tag");
  refused("splice", bad, a.g, "content tag");
  bad = a.blob;
  bad[0] ^= (char)0xFF;
  refused("magic", bad, a.g, "not an aligned-form blob of this library build");
  bad = a.blob;
  write_at(bad, offsetof(AlignedHdr, total_bytes), h.total_bytes + 1);
  refused("total_bytes", bad, a.g, "not an aligned-form blob of this library build");
  bad = a.blob;
  write_at(bad, sizeof(AlignedHdr) + offsetof(escoin_conv_desc, M), a.g.d.M * 2);
  refused("other_M", bad, a.g, "exported for other weights");
  bad = a.blob;
  write_at(bad, offsetof(AlignedHdr, nnz), (uint64_t)a.g.d.group * a.g.Mg * a.g.kdim + 1);
  refused("nnz", bad, a.g, "nnz or code section larger than the layer / the blob");
  bad = a.blob;
  write_at(bad, offsetof(AlignedHdr, nnz), h.nnz + 1);
  refused("sizes", bad, a.g, "section sizes do not add up");
}

// ---- the code section, parsed directly: the tags do not shield it ------------------------------------------------------
// One field of the section set to one value.  may_fit(v): whether the checks (which are sconv_tiled.hip's of before this
// unit, unchanged) accept the field at v when v is not what the exporter wrote; every other combination must be refused.
struct Field {
  const char *name;
  size_t off, size;
  std::function<bool(long long)> may_fit;
};
static const auto kNever = [](long long) { return false; };
static const auto kAlways = [](long long) { return true; };      // informational: no check reads it

static void mutate(const Export &e, const char *what, const std::vector<Field> &fields) {
  const long long values[] = {0, 1, -1, 0x7FFFFFFFll};      // (-1: all ones, UINT64_MAX in a 64-bit count)
  for (const Field &fd : fields)
    for (long long v : values) {
      Bytes sec = e.sec;
      Bytes before(sec.begin() + (ptrdiff_t)fd.off, sec.begin() + (ptrdiff_t)(fd.off + fd.size));
      if (fd.size == 8) write_at<int64_t>(sec, fd.off, (int64_t)v);
      else write_at<int32_t>(sec, fd.off, (int32_t)v);
      const bool unchanged = memcmp(before.data(), sec.data() + fd.off, fd.size) == 0;
      CodeSection s;
      const bool fits = parse_copy(sec, sec.size(), e.g, e.fit, &s);
      REQUIRE(fits == (unchanged || fd.may_fit(v)), "%s %s = %lld: %s", e.name.c_str(), fd.name, v, fits ? "accepted" : "refused");
    }
  printf("OK code %s %s\n", e.name.c_str(), what);
}

static void code_section(const Export &e) {
  const AlignedJitHdr h = read_at<AlignedJitHdr>(e.sec, 0);
  CodeSection s;
  // truncation at every section boundary and one byte either side of each (one byte past the end: a longer buffer)
  const size_t ints_at = sizeof(AlignedJitHdr), unit_at = ints_at + 4 * kTilingInts, chan_at = unit_at + 4 * (size_t)h.n_unit_off,
               code_at = chan_at + 4 * (size_t)h.n_chan, end = code_at + (size_t)h.code_bytes;
  REQUIRE(end == e.sec.size(), "%s: layout", e.name.c_str());
  Bytes longer = e.sec;
  longer.push_back(0);
  for (size_t b : {(size_t)0, ints_at, unit_at, chan_at, code_at, end})
    for (int delta : {-1, 0, 1}) {
      if (b == 0 && delta < 0) continue;
      const size_t n = b + (size_t)delta;
      if (n == end) continue;      // (the whole section)
      REQUIRE(!parse_copy(longer, n, e.g, e.fit, &s), "%s: accepted at %zu of %zu bytes", e.name.c_str(), n, end);
    }
  printf("OK code %s truncation\n", e.name.c_str());

  // every header field.  Accepted beyond the exporter's own value: the prefetch count and the quad-table period within
  // their ranges (a chained program needs a period), any jit_chain (0: the generic body runs the same code; nonzero
  // reads as 1) and what no check reads (the plane budget, the density, the statistics, the reserved words).
  REQUIRE(h.jit_chain == 1 && h.dma_period > 1, "%s: the host programs are chained", e.name.c_str());
#define HF(f, rule) Field{#f, offsetof(AlignedJitHdr, f), sizeof(h.f) > 8 ? 4 : sizeof(h.f), rule}
  mutate(e, "header_fields",
         {HF(magic, kNever), HF(version, kNever), HF(n_cu, kNever), HF(n_tiling_ints, kNever), HF(nbuf, kNever),
          HF(jit_pref, [](long long v) { return v >= 0 && v <= 4096; }),
          HF(dma_period, [](long long v) { return v >= 1 && v <= 65536; }), HF(lds_budget, kAlways),
          HF(tiling_batch, kNever), HF(jit_chain, kAlways), HF(jit_self_zero, kNever), HF(reserved0, kAlways),
          HF(density, kAlways), HF(n_dense_groups, kNever), HF(dense_mask, kNever), HF(jit_rows, kAlways),
          HF(jit_records, kAlways), HF(code_bytes, kNever), HF(reserved1, kAlways), HF(n_unit_off, kNever),
          HF(n_chan, kNever), HF(isa, kNever)});
#undef HF
  // every one of the 28 tiling ints.  Accepted beyond the exporter's own value: ok reads as "!= 0", band_mode is read
  // by no check, and the image cut's OH / OW, the segments and the bands have a lower bound only; every other field is
  // tied to the geometry or to another field by an equality.
  static const char *const names[kTilingInts] = {"ok", "band_mode", "KW", "KH", "H", "W", "OH", "OW", "S4", "RS", "rows_per_slab",
      "pix_waves", "oc_waves", "waves", "G", "n_ocg", "n_ocblk", "tpl", "rows_per_wg", "tr", "nseg", "bands", "plane_rows",
      "plane_seg_floats", "plane_ch_floats", "icb", "n_icb", "planes_bytes"};
  std::vector<Field> ints;
  for (int i = 0; i < kTilingInts; ++i) {
    const std::string n = names[i];
    std::function<bool(long long)> rule = kNever;
    if (n == "ok") rule = [](long long v) { return v != 0; };
    else if (n == "band_mode") rule = kAlways;
    else if (n == "OH" || n == "OW" || n == "nseg" || n == "bands") rule = [](long long v) { return v >= 1; };
    ints.push_back(Field{names[i], ints_at + 4 * (size_t)i, 4, rule});
  }
  mutate(e, "tiling_ints", ints);

  // the first and the last unit offset at code_bytes, the first channel at Mg
  for (size_t at : {unit_at, chan_at - 4}) {
    Bytes sec = e.sec;
    write_at<uint32_t>(sec, at, (uint32_t)h.code_bytes);
    REQUIRE(!parse_copy(sec, sec.size(), e.g, e.fit, &s), "%s: unit offset == code_bytes accepted", e.name.c_str());
  }
  printf("OK code %s unit_off\n", e.name.c_str());
  Bytes sec = e.sec;
  write_at<uint32_t>(sec, chan_at, (uint32_t)e.g.Mg);
  REQUIRE(!parse_copy(sec, sec.size(), e.g, e.fit, &s), "%s: channel == Mg accepted", e.name.c_str());
  printf("OK code %s chan\n", e.name.c_str());
}

int main(int argc, char **argv) {
  for (int i = 1; i < argc; ++i) golden(argv[i]);
  const Export programs[] = {make_export("k3p1", geometry(4, 32, 14, 32, 3, 1, 1), 1.f),
                             make_export("k1", geometry(4, 64, 28, 32, 1, 0, 1), 1.f),
                             make_export("k5p2g2", geometry(4, 16, 12, 16, 5, 2, 2), 1.f)};
  for (const Export &e : programs) host_round_trip(e);
  mismatches(programs[0]);
  outer(programs[0], make_export("k3p1", geometry(4, 32, 14, 32, 3, 1, 1), 1.5f));
  for (const Export &e : programs) code_section(e);
  return 0;
}
