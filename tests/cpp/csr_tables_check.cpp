// csr_tables_check.cpp -- every builder of csrc/csr_tables.{h,cpp} against a brute-force restatement, on the host.
// Compiled with plain g++ against csr_tables.cpp alone: no HIP header, no device (tests/test_csr_tables.py).
//
// A case's pattern is drawn as (ic, kr, kc) triples, so the restatements never decode a column: they know every entry's
// tap, row and flat index from how the pattern was made, and restate each table by scattering tags into a dense matrix
// and scanning it, by sorting, or by the table's defining formula.  Prints "OK <case> <builder>" per check that held
// and "FAIL ..." lines otherwise; exit status 1 if anything failed.
#include <algorithm>
#include <cstdio>
#include <string>
#include <tuple>
#include <vector>

#include "align_rules.h"   // kStgBatch
#include "csr_tables.h"

using namespace escoin;

namespace {

int g_failed = 0;

struct Checker {
  std::string name;
  bool ok = true;
  void expect(bool cond, const char *what, long a = 0, long b = 0) {
    if (cond) return;
    if (ok) std::printf("FAIL %s: %s (%ld, %ld)\n", name.c_str(), what, a, b);
    ok = false;
  }
  template <typename T>
  void same(const std::vector<T> &got, const std::vector<T> &want, const char *what) {
    expect(got.size() == want.size(), what, (long)got.size(), (long)want.size());
    if (got.size() != want.size()) return;
    for (size_t i = 0; i < got.size(); ++i)
      if (got[i] != want[i]) return expect(false, what, (long)i, (long)got[i]);
  }
  ~Checker() {
    if (ok) std::printf("OK %s\n", name.c_str());
    else ++g_failed;
  }
};

// One nonzero as the pattern generator made it.
struct Ent { int grp, m, ic, kr, kc, col; long e; };

struct Case {
  std::string name;
  Geometry g;
  std::vector<std::vector<int>> rowptr, colidx;
  std::vector<Ent> ents;                 // in CSR order: ents[e].e == e
  int icb = 1, nblk = 1;                 // staged_tables' blocks
  long nnz() const { return (long)ents.size(); }
  CsrView view() const { return CsrView{&g, &rowptr, &colidx}; }
};

Geometry geometry(int group, int C, int M, int KH, int KW, int H, int W, int pad_h, int pad_w, int stride, int dil) {
  Geometry g{};
  g.d.N = 1; g.d.C = C; g.d.H = H; g.d.W = W; g.d.M = M; g.d.KH = KH; g.d.KW = KW;
  g.d.pad_h = pad_h; g.d.pad_w = pad_w; g.d.stride_h = g.d.stride_w = stride; g.d.dil_h = g.d.dil_w = dil;
  g.d.group = group;
  g.OH = (H + 2 * pad_h - (dil * (KH - 1) + 1)) / stride + 1;
  g.OW = (W + 2 * pad_w - (dil * (KW - 1) + 1)) / stride + 1;
  g.Cg = C / group; g.Mg = M / group;
  g.kdim = g.Cg * KH * KW;
  return g;
}

unsigned next_random(unsigned *state) { return *state = *state * 1664525u + 1013904223u; }

// keep(grp, m, ic, kr, kc, is_last_column) decides the pattern; the CSR is written in (group, row, ic, kr, kc) order,
// which is ascending columns.
template <typename Keep>
Case make_case(const std::string &name, const Geometry &g, int icb, Keep keep) {
  Case c;
  c.name = name; c.g = g; c.icb = icb; c.nblk = (g.Cg + icb - 1) / icb;
  c.rowptr.assign(g.d.group, std::vector<int>(g.Mg + 1, 0));
  c.colidx.assign(g.d.group, std::vector<int>());
  for (int grp = 0; grp < g.d.group; ++grp)
    for (int m = 0; m < g.Mg; ++m) {
      int col = 0;
      for (int ic = 0; ic < g.Cg; ++ic)
        for (int kr = 0; kr < g.d.KH; ++kr)
          for (int kc = 0; kc < g.d.KW; ++kc, ++col)
            if (keep(grp, m, ic, kr, kc, col == g.kdim - 1)) {
              c.ents.push_back(Ent{grp, m, ic, kr, kc, col, (long)c.ents.size()});
              c.colidx[grp].push_back(col);
            }
      c.rowptr[grp][m + 1] = (int)c.colidx[grp].size();
    }
  return c;
}

Case random_case(const std::string &name, const Geometry &g, int icb, unsigned seed) {
  unsigned state = seed;
  return make_case(name, g, icb, [&](int, int, int, int, int, bool) { return next_random(&state) % 100u < 40u; });
}

void check_view(const Case &c) {
  Checker k{c.name + " for_each_entry"};
  k.expect(c.view().nnz() == c.nnz(), "nnz", c.view().nnz(), c.nnz());
  long seen = 0, first_of_group_1 = -1;
  for_each_entry(c.view(), [&](const CsrEntry &e) {
    const bool in = seen < c.nnz();
    if (in) {
      const Ent &w = c.ents[(size_t)seen];
      k.expect(e.e == seen && e.grp == w.grp && e.m == w.m && e.col == w.col && c.colidx[e.grp][e.j] == w.col, "entry", seen);
      if (w.grp == 1 && first_of_group_1 < 0) first_of_group_1 = seen;
    }
    ++seen;
  });
  k.expect(seen == c.nnz(), "entries visited", seen, c.nnz());
  k.expect(c.view().group_base(0) == 0, "group_base(0)");
  if (c.g.d.group > 1 && first_of_group_1 >= 0)
    k.expect(c.view().group_base(1) == first_of_group_1, "group_base(1)", c.view().group_base(1), first_of_group_1);
}

void check_forward_transpose(const Case &c) {
  Checker k{c.name + " forward_transpose"};
  const Geometry &g = c.g;
  const int KH = g.d.KH, KW = g.d.KW, KK = KH * KW, cols = g.Mg * KK;
  std::vector<long> dense((size_t)g.d.group * g.Cg * cols, 0);
  for (const Ent &e : c.ents) {
    long &cell = dense[((size_t)e.grp * g.Cg + e.ic) * cols + (size_t)e.m * KK + (KH - 1 - e.kr) * KW + (KW - 1 - e.kc)];
    k.expect(cell == 0, "two entries at one transposed place", e.e);
    cell = e.e + 1;
  }
  std::vector<int> rowptr, colidx, tsrc, nnz_g;
  for (int grp = 0; grp < g.d.group; ++grp) {
    int in_group = 0;
    rowptr.push_back(0);
    for (int icl = 0; icl < g.Cg; ++icl) {
      for (int col = 0; col < cols; ++col)
        if (const long tag = dense[((size_t)grp * g.Cg + icl) * cols + col]) {
          colidx.push_back(col);
          tsrc.push_back((int)(tag - 1));
          ++in_group;
        }
      rowptr.push_back(in_group);
    }
    nnz_g.push_back(in_group);
  }
  const DerivedCsr t = forward_transpose(c.view());
  k.same(t.rowptr, rowptr, "rowptr'");
  k.same(t.colidx, colidx, "colidx'");
  k.same(t.src, tsrc, "tsrc");
  k.same(t.nnz_g, nnz_g, "nnz_g");
}

void check_gather_transpose(const Case &c) {
  Checker k{c.name + " gather_transpose"};
  const Geometry &g = c.g;
  std::vector<Ent> order = c.ents;
  std::stable_sort(order.begin(), order.end(), [&](const Ent &a, const Ent &b) {
    return std::make_tuple(a.grp * g.Cg + a.ic, a.m, a.kr, a.kc) < std::make_tuple(b.grp * g.Cg + b.ic, b.m, b.kr, b.kc);
  });
  std::vector<int> trow((size_t)g.d.C + 1, 0), ttap, tsrc;
  for (const Ent &e : order) {
    ++trow[(size_t)e.grp * g.Cg + e.ic + 1];
    ttap.push_back((e.m << 16) | (e.kr << 8) | e.kc);
    tsrc.push_back((int)e.e);
  }
  for (int ch = 0; ch < g.d.C; ++ch) trow[ch + 1] += trow[ch];
  if (ttap.empty()) ttap.push_back(0);      // (padded: never an empty upload)
  const GatherTables t = gather_transpose(c.view());
  k.same(t.trow, trow, "trow");
  k.same(t.ttap, ttap, "ttap");
  k.same(t.tsrc, tsrc, "tsrc");
  std::vector<int> perm = t.tsrc;
  std::sort(perm.begin(), perm.end());
  for (size_t i = 0; i < perm.size(); ++i) k.expect(perm[i] == (int)i, "tsrc is no permutation", (long)i, perm[i]);
  k.expect((long)perm.size() == c.nnz(), "tsrc length", (long)perm.size(), c.nnz());
}

// Tags through `pos` into an M x stride matrix, then a row scan: the tags must come back as 1 .. nnz, row by row.
void check_positions(const Case &c, int stride, const char *label) {
  Checker k{c.name + " dense_positions " + label};
  const Geometry &g = c.g;
  const std::vector<int> pos = dense_positions(c.view(), stride);
  k.expect((long)pos.size() == std::max<long>(c.nnz(), 1), "length", (long)pos.size());
  if (c.nnz() == 0) return k.expect(pos.size() == 1 && pos[0] == 0, "padding of the empty pattern");
  if (!k.ok) return;
  std::vector<long> dense((size_t)g.d.M * stride, 0);
  for (const Ent &e : c.ents) {
    const long at = pos[(size_t)e.e];
    k.expect(at >= 0 && at < (long)dense.size(), "position outside the matrix", e.e, at);
    if (!k.ok) return;
    k.expect(at == ((long)e.grp * g.Mg + e.m) * stride + e.col, "position is not (row, col)", e.e, at);
    k.expect(dense[(size_t)at] == 0, "two entries at one position", e.e, at);
    dense[(size_t)at] = e.e + 1;
  }
  long expect_tag = 1;
  for (const long tag : dense)
    if (tag) k.expect(tag == expect_tag++, "row scan out of CSR order", tag);
  k.expect(expect_tag == c.nnz() + 1, "entries lost", expect_tag);
}

void check_generic(const Case &c) {
  Checker k{c.name + " generic_tables"};
  const Geometry &g = c.g;
  const GenericTables t = generic_tables(c.view());
  std::vector<int> rowptr((size_t)g.d.M + 1, 0);
  for (const Ent &e : c.ents) ++rowptr[(size_t)e.grp * g.Mg + e.m + 1];
  for (int oc = 0; oc < g.d.M; ++oc) rowptr[oc + 1] += rowptr[oc];
  k.same(t.rowptr, rowptr, "rowptr");
  k.expect((long)t.taps.size() == std::max<long>(c.nnz(), 1), "taps length", (long)t.taps.size());
  if (c.nnz() == 0) return k.expect(t.taps.size() == 1 && t.taps[0] == 0, "padding of the empty pattern");
  if (!k.ok) return;
  for (const Ent &e : c.ents) {
    const int tap = t.taps[(size_t)e.e], ic = tap >> 16, kr = (tap >> 8) & 0xff, kc = tap & 0xff;
    k.expect((ic * g.d.KH + kr) * g.d.KW + kc == e.col && ic == e.ic && kr == e.kr && kc == e.kc, "tap does not rebuild col", e.e, tap);
  }
}

void check_staged(const Case &c) {
  Checker k{c.name + " staged_tables"};
  const Geometry &g = c.g;
  const int Wp = g.d.W + 2 * g.d.pad_w, cs = (g.d.H + 2 * g.d.pad_h) * Wp, nb = c.nblk;
  const StagedTables t = staged_tables(c.view(), c.icb, nb, cs, Wp);
  k.expect(t.blk.size() == (size_t)g.d.M * (nb + 1), "blk length", (long)t.blk.size());
  k.expect(t.off.size() == (size_t)c.nnz() + 2 * kStgBatch, "off length", (long)t.off.size());
  if (!k.ok) return;
  std::vector<long> row_begin((size_t)g.d.M + 1, 0);
  for (const Ent &e : c.ents) ++row_begin[(size_t)e.grp * g.Mg + e.m + 1];
  for (int oc = 0; oc < g.d.M; ++oc) row_begin[oc + 1] += row_begin[oc];
  for (int oc = 0; oc < g.d.M; ++oc) {
    const int *blk = t.blk.data() + (size_t)oc * (nb + 1);
    k.expect(blk[0] == row_begin[oc], "first block does not begin at the row", oc, blk[0]);
    k.expect(blk[nb] == row_begin[oc + 1], "last block does not end at the row's end", oc, blk[nb]);
    for (int b = 0; b < nb; ++b) k.expect(blk[b] <= blk[b + 1], "ranges not contiguous", oc, b);
    for (long e = row_begin[oc]; e < row_begin[oc + 1]; ++e)
      for (int b = 0; b < nb; ++b)
        k.expect((blk[b] <= e && e < blk[b + 1]) == (c.ents[(size_t)e].ic / c.icb == b), "entry in the wrong block", e, b);
  }
  for (const Ent &e : c.ents)
    k.expect(t.off[(size_t)e.e] == (e.ic % c.icb) * cs + e.kr * g.d.dil_h * Wp + e.kc * g.d.dil_w, "tap offset", e.e, t.off[(size_t)e.e]);
  for (size_t i = (size_t)c.nnz(); i < t.off.size(); ++i) k.expect(t.off[i] == 0, "read-ahead tail not zero", (long)i);
}

void check_entry_major(const Case &c, unsigned seed) {
  Checker k{c.name + " entry_major"};
  // a list like the update state's: sorted by (buffer, entry), an entry at most once per buffer
  unsigned state = seed;
  std::vector<int> src;
  std::vector<unsigned> off;
  std::vector<unsigned char> buf;
  typedef std::tuple<int, unsigned, int> Triple;
  std::vector<Triple> want;
  for (int b = 0; b < 3; ++b)
    for (long e = 0; e < c.nnz(); ++e)
      if (b == 0 || next_random(&state) % 100u < 60u) {
        src.push_back((int)e), off.push_back(next_random(&state) >> 8), buf.push_back((unsigned char)b);
        want.emplace_back((int)e, off.back(), b);
      }
  EntryMajor em;
  k.expect(entry_major(src, off, buf, c.nnz(), &em), "a good list was refused");
  if (!k.ok) return;
  const size_t nz = (size_t)std::max<long>(c.nnz(), 1), n = std::max<size_t>(src.size(), 1);
  k.expect(em.e_ptr.size() == nz + 1 && em.e_off.size() == n && em.e_buf.size() == n, "lengths", (long)em.e_ptr.size(), (long)em.e_off.size());
  if (!k.ok) return;
  k.expect(em.e_ptr[0] == 0 && em.e_ptr[nz] == (int)src.size(), "e_ptr ends", em.e_ptr[0], em.e_ptr[nz]);
  std::vector<Triple> got;
  for (size_t e = 0; e < nz; ++e) {
    k.expect(em.e_ptr[e] <= em.e_ptr[e + 1] && em.e_ptr[e + 1] <= (int)src.size(), "e_ptr not monotone", (long)e);
    if (!k.ok) return;
    for (int at = em.e_ptr[e]; at < em.e_ptr[e + 1]; ++at) {
      got.emplace_back((int)e, em.e_off[(size_t)at], (int)em.e_buf[(size_t)at]);
      if (at > em.e_ptr[e]) k.expect(em.e_buf[(size_t)at - 1] < em.e_buf[(size_t)at], "buffers do not ascend within an entry", (long)e);
    }
  }
  std::sort(got.begin(), got.end());
  std::sort(want.begin(), want.end());
  k.expect(got == want, "the expanded view is not the list");
  // a destination that names no CSR entry
  EntryMajor none;
  src.push_back((int)c.nnz()), off.push_back(0u), buf.push_back((unsigned char)2);
  k.expect(!entry_major(src, off, buf, c.nnz(), &none), "src = nnz was accepted");
  src.back() = -1;
  k.expect(!entry_major(src, off, buf, c.nnz(), &none), "src = -1 was accepted");
}

// The case's two real entry maps in a row (the transposed plan's order read through the gather order): values copied twice,
// once per map, equal the values read once through the composed map.  Then the identity on either side, and the refusals.
void check_compose(const Case &c) {
  Checker k{c.name + " compose_maps"};
  const long n = c.nnz();
  const std::vector<int> outer = forward_transpose(c.view()).src, inner = gather_transpose(c.view()).tsrc;
  std::vector<long> vals((size_t)n), once((size_t)n), twice((size_t)n);
  for (long e = 0; e < n; ++e) vals[(size_t)e] = 7 * e + 3;
  for (long j = 0; j < n; ++j) once[(size_t)j] = vals[(size_t)outer[(size_t)j]];
  for (long i = 0; i < n; ++i) twice[(size_t)i] = once[(size_t)inner[(size_t)i]];
  std::vector<int> out{-7};
  k.expect(compose_maps(&outer, &inner, n, &out), "two good maps were refused");
  k.expect((long)out.size() == n, "length", (long)out.size(), n);
  if (!k.ok) return;
  for (long i = 0; i < n; ++i) {
    k.expect(out[(size_t)i] >= 0 && out[(size_t)i] < n, "composed index outside the CSR", i, out[(size_t)i]);
    if (!k.ok) return;
    k.expect(vals[(size_t)out[(size_t)i]] == twice[(size_t)i], "the composed map reads another value", i, out[(size_t)i]);
  }
  k.expect(compose_maps(nullptr, &inner, n, &out), "identity outside was refused");
  k.same(out, inner, "identity outside");
  k.expect(compose_maps(&outer, nullptr, n, &out), "identity inside was refused");
  k.same(out, outer, "identity inside");
  k.expect(compose_maps(nullptr, nullptr, n, &out), "two identities were refused");
  k.expect((long)out.size() == n, "two identities: length", (long)out.size(), n);
  for (size_t i = 0; i < out.size(); ++i) k.expect(out[i] == (int)i, "two identities", (long)i, out[i]);
  // refused, and nothing written: an index of the inner map at n or below 0 (with and without an outer map), an outer
  // map of another length
  const std::vector<int> untouched{-7, -7, -7};
  std::vector<int> bad = inner;
  for (const int index : {(int)n, -1}) {
    bad.push_back(index);
    out = untouched;
    k.expect(!compose_maps(&outer, &bad, n, &out) && out == untouched, "a bad index was accepted, or something was written", index);
    k.expect(!compose_maps(nullptr, &bad, n, &out) && out == untouched, "a bad index under the identity was accepted", index);
    bad.pop_back();
  }
  bad = outer;
  bad.push_back(0);
  out = untouched;
  k.expect(!compose_maps(&bad, &inner, n, &out) && out == untouched, "an outer map of n + 1 elements was accepted");
}

void check_compose_by_hand() {
  Checker k{"by_hand compose_maps"};
  // four entries; a first-level plan that holds them in the order 2 0 3 1; a second-level copy of three of ITS entries
  const std::vector<int> outer{2, 0, 3, 1}, inner{3, 3, 0};
  std::vector<int> out;
  k.expect(compose_maps(&outer, &inner, 4, &out), "refused");
  k.same(out, std::vector<int>{1, 1, 2}, "outer[inner[k]]");
  // no entries at all: empty maps compose to an empty map, and the only index there is, 0, is already out of range
  const std::vector<int> none, zero{0};
  out = {5};
  k.expect(compose_maps(&none, &none, 0, &out) && out.empty(), "empty maps");
  out = {5};
  k.expect(compose_maps(nullptr, nullptr, 0, &out) && out.empty(), "empty identities");
  out = {5};
  k.expect(!compose_maps(&none, &zero, 0, &out) && out == std::vector<int>{5}, "index 0 of an empty map was accepted");
}

void check_stretched(const Case &c) {
  Checker k{c.name + " stretched_col"};
  const escoin_conv_desc &d = c.g.d;
  for (const Ent &e : c.ents)
    k.expect(stretched_col(e.col, d) == (e.ic * (d.H + d.pad_h) + e.kr) * (d.W + d.pad_w) + e.kc, "stretched column", e.e, stretched_col(e.col, d));
}

void check_case(const Case &c, unsigned seed) {
  check_view(c);
  check_forward_transpose(c);
  check_gather_transpose(c);
  check_positions(c, c.g.kdim, "kdim");
  check_positions(c, c.g.kdim + 5, "padded");     // (a row stride past kdim, like the MFMA kernel's matrix)
  check_generic(c);
  check_staged(c);
  check_entry_major(c, seed ^ 0x9e3779b9u);
  check_compose(c);
  check_stretched(c);
}

}  // namespace

int main() {
  // (a) grouped, asymmetric kernel and padding: kr vs kc, group-local vs global channels
  check_case(random_case("grouped", geometry(2, 4, 6, 3, 2, 6, 5, 1, 0, 1, 1), 1, 101u), 101u);
  // (b) dilated 3x3, blocks of two channels over five: the last block holds one
  check_case(random_case("dilated", geometry(1, 5, 3, 3, 3, 7, 7, 2, 2, 1, 2), 2, 202u), 202u);
  // (c) strided 5x5: the gather path's geometry
  check_case(random_case("strided", geometry(1, 3, 2, 5, 5, 9, 9, 2, 2, 2, 1), 3, 303u), 303u);
  // (d) an all-zero output row and an input channel without an entry
  {
    unsigned state = 404u;
    check_case(make_case("empty_rows", geometry(1, 4, 4, 3, 3, 6, 6, 1, 1, 1, 1), 2, [&](int, int m, int ic, int, int, bool) {
      const bool draw = next_random(&state) % 100u < 40u;
      return m != 2 && ic != 1 && draw;
    }), 404u);
  }
  // (e) no entry at all: the padded lengths, and nothing indexed
  check_case(make_case("empty", geometry(1, 2, 2, 3, 3, 5, 5, 1, 1, 1, 1), 1, [](int, int, int, int, int, bool) { return false; }), 505u);
  // (f) one entry per row, in the last column
  check_case(make_case("lone", geometry(1, 3, 4, 3, 3, 5, 5, 1, 1, 1, 1), 2, [](int, int, int, int, int, bool last) { return last; }), 606u);
  // (g) fully dense
  check_case(make_case("dense", geometry(1, 2, 2, 3, 3, 5, 5, 1, 1, 1, 1), 1, [](int, int, int, int, int, bool) { return true; }), 707u);
  check_compose_by_hand();
  if (g_failed) std::printf("%d checks FAILED\n", g_failed);
  return g_failed ? 1 : 0;
}
