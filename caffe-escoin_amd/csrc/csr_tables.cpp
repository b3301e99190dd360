// csr_tables.cpp -- the tables derived from a plan's host CSR (csr_tables.h).  No HIP, no device, no plan.
#include "csr_tables.h"

#include <algorithm>
#include <utility>

#include "align_rules.h"   // kStgBatch: the staged kernel's read-ahead

namespace escoin {

static size_t at_least_one(long n) { return (size_t)std::max<long>(n, 1); }

GenericTables generic_tables(const CsrView &v) {
  const Geometry &g = *v.g;
  GenericTables t;
  t.rowptr.resize((size_t)g.d.M + 1);
  t.taps.assign(at_least_one(v.nnz()), 0);
  long base = 0;
  for (int grp = 0; grp < g.d.group; ++grp) {
    for (int m = 0; m < g.Mg; ++m) t.rowptr[(size_t)grp * g.Mg + m] = (int)(base + (*v.rowptr)[grp][m]);
    base += (long)(*v.colidx)[grp].size();
  }
  t.rowptr[g.d.M] = (int)base;
  for_each_entry(v, [&](const CsrEntry &c) { t.taps[(size_t)c.e] = pack_tap(decode_tap(c.col, g.d.KH, g.d.KW)); });
  return t;
}

std::vector<int> dense_positions(const CsrView &v, int row_stride) {
  const Geometry &g = *v.g;
  std::vector<int> pos(at_least_one(v.nnz()), 0);
  for_each_entry(v, [&](const CsrEntry &c) {
    pos[(size_t)c.e] = (int)(((long)c.grp * g.Mg + c.m) * row_stride + c.col);
  });
  return pos;
}

GatherTables gather_transpose(const CsrView &v) {
  const Geometry &g = *v.g;
  const escoin_conv_desc &d = g.d;
  const long nnz = v.nnz();
  // a counting sort by input channel: stable, so a channel's entries keep the walk's (ocl, kr, kc) order
  std::vector<int> cnt((size_t)d.C + 1, 0);
  for_each_entry(v, [&](const CsrEntry &c) { ++cnt[(size_t)c.grp * g.Cg + decode_tap(c.col, d.KH, d.KW).ic + 1]; });
  for (int c = 0; c < d.C; ++c) cnt[c + 1] += cnt[c];
  GatherTables t;
  t.trow = cnt;
  t.ttap.assign(at_least_one(nnz), 0);
  t.tsrc.assign((size_t)nnz, 0);
  for_each_entry(v, [&](const CsrEntry &c) {
    const Tap tap = decode_tap(c.col, d.KH, d.KW);
    const size_t at = (size_t)cnt[(size_t)c.grp * g.Cg + tap.ic]++;
    t.ttap[at] = pack_tap(Tap{c.m, tap.kr, tap.kc});
    t.tsrc[at] = (int)c.e;
  });
  return t;
}

ForwardTranspose forward_transpose(const CsrView &v) {
  const Geometry &g = *v.g;
  const escoin_conv_desc &d = g.d;
  const int kk = d.KH * d.KW;
  ForwardTranspose t;
  t.rowptr.assign((size_t)d.group * (g.Cg + 1), 0);
  t.nnz_g.assign(d.group, 0);
  // per row of a group: (column', flat index of the entry).  The columns of a row are distinct, so the sorted order is a
  // function of the pattern alone.
  std::vector<std::vector<std::pair<int, int>>> rows((size_t)d.group * g.Cg);
  for_each_entry(v, [&](const CsrEntry &c) {
    const Tap tap = decode_tap(c.col, d.KH, d.KW);
    rows[(size_t)c.grp * g.Cg + tap.ic].emplace_back(c.m * kk + (d.KH - 1 - tap.kr) * d.KW + (d.KW - 1 - tap.kc), (int)c.e);
  });
  for (int grp = 0; grp < d.group; ++grp) {
    int *trp = t.rowptr.data() + (size_t)grp * (g.Cg + 1);
    for (int c = 0; c < g.Cg; ++c) {
      std::vector<std::pair<int, int>> &row = rows[(size_t)grp * g.Cg + c];
      std::sort(row.begin(), row.end());
      for (const auto &e : row) {
        t.colidx.push_back(e.first);
        t.tsrc.push_back(e.second);
      }
      trp[c + 1] = trp[c] + (int)row.size();
    }
    t.nnz_g[grp] = trp[g.Cg];
  }
  return t;
}

StagedTables staged_tables(const CsrView &v, int icb, int nblk, int cs, int Wp) {
  const Geometry &g = *v.g;
  const escoin_conv_desc &d = g.d;
  const int kk = d.KH * d.KW;
  StagedTables t;
  t.blk.resize((size_t)d.M * (nblk + 1));
  t.off.assign((size_t)v.nnz() + 2 * kStgBatch, 0);
  long base = 0;
  for (int grp = 0; grp < d.group; ++grp) {
    const std::vector<int> &rp = (*v.rowptr)[grp], &ci = (*v.colidx)[grp];
    for (int m = 0; m < g.Mg; ++m) {
      int *row = t.blk.data() + ((size_t)grp * g.Mg + m) * (nblk + 1);
      int j = rp[m];
      for (int b = 0; b <= nblk; ++b) {
        // the columns of a row ascend (set_csr checks it), so its input channels do
        while (b < nblk && j < rp[m + 1] && ci[j] / kk < b * icb) ++j;
        if (b == nblk) j = rp[m + 1];
        row[b] = (int)(base + j);
      }
    }
    base += (long)ci.size();
  }
  for_each_entry(v, [&](const CsrEntry &c) {
    const Tap tap = decode_tap(c.col, d.KH, d.KW);
    t.off[(size_t)c.e] = (tap.ic % icb) * cs + tap.kr * d.dil_h * Wp + tap.kc * d.dil_w;
  });
  return t;
}

WgmTables wgrad_mfma_tables(const CsrView &v, int tile_m, int tile_k) {
  const Geometry &g = *v.g;
  const escoin_conv_desc &d = g.d;
  const int mtiles = (g.Mg + tile_m - 1) / tile_m, ktiles = (g.kdim + tile_k - 1) / tile_k;
  WgmTables t;
  t.ent.assign(at_least_one((long)d.M * g.kdim), -1);
  t.tile_cnt.assign(at_least_one((long)d.group * mtiles * ktiles), 0);
  for_each_entry(v, [&](const CsrEntry &c) {
    t.ent[((size_t)c.grp * g.Mg + c.m) * g.kdim + c.col] = (int)c.e;
    ++t.tile_cnt[((size_t)c.grp * mtiles + c.m / tile_m) * ktiles + c.col / tile_k];
  });
  t.ktab.assign(at_least_one(4L * ktiles * tile_k), 0);
  for (int k = 0; k < g.kdim; ++k) {
    const Tap tap = decode_tap(k, d.KH, d.KW);
    const int dy = tap.kr * d.dil_h, dx = tap.kc * d.dil_w;
    t.ktab[4 * (size_t)k] = (tap.ic * d.H + dy) * d.W + dx;
    t.ktab[4 * (size_t)k + 1] = dy;
    t.ktab[4 * (size_t)k + 2] = dx;
    t.ktab[4 * (size_t)k + 3] = 1;
  }
  return t;
}

bool entry_major(const std::vector<int> &src, const std::vector<unsigned> &off, const std::vector<unsigned char> &buf,
                 long nnz, EntryMajor *out) {
  const size_t n = src.size(), nz = at_least_one(nnz);
  // a counting sort of the list by CSR entry: stable, so within an entry the list's order (its buffers ascend) is kept
  std::vector<int> ptr(nz + 1, 0);
  for (size_t k = 0; k < n; ++k) {
    if (src[k] < 0 || (long)src[k] >= nnz) return false;
    ++ptr[(size_t)src[k] + 1];
  }
  for (size_t i = 0; i < nz; ++i) ptr[i + 1] += ptr[i];
  out->e_ptr = ptr;
  out->e_off.assign(std::max<size_t>(n, 1), 0);
  out->e_buf.assign(std::max<size_t>(n, 1), 0);
  for (size_t k = 0; k < n; ++k) {
    const size_t at = (size_t)ptr[(size_t)src[k]]++;
    out->e_off[at] = off[k], out->e_buf[at] = buf[k];
  }
  return true;
}

int stretched_col(int col, const escoin_conv_desc &d) {
  const Tap tap = decode_tap(col, d.KH, d.KW);
  return (tap.ic * (d.H + d.pad_h) + tap.kr) * (d.W + d.pad_w) + tap.kc;
}

}  // namespace escoin
