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

DerivedCsr forward_transpose(const CsrView &v) {
  const Geometry &g = *v.g;
  const escoin_conv_desc &d = g.d;
  const int kk = d.KH * d.KW;
  DerivedCsr t;
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
        t.src.push_back(e.second);
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

PwTables pw_tables(const CsrView &v, const PwPlan &plan) {
  const Geometry &g = *v.g;
  PwTables t;
  t.tile.reserve(plan.tiles.size() * kPwTileWords);
  t.ent.reserve((size_t)v.nnz() + 1);
  t.pk.reserve((size_t)v.nnz() + 1);
  std::vector<long> base((size_t)g.d.group);
  for (int grp = 0; grp < g.d.group; ++grp) base[grp] = v.group_base(grp);
  for (const PwTile &pt : plan.tiles) {
    const std::vector<int> &rp = (*v.rowptr)[pt.grp], &ci = (*v.colidx)[pt.grp];
    const int first = (int)t.ent.size();
    for (int r = 0; r < pt.rows; ++r) {
      const int m = pt.row0 + r;
      // the columns of a row ascend (set_csr checks it), and a pointwise column is the group-local channel
      const int *lo = std::lower_bound(ci.data() + rp[m], ci.data() + rp[m + 1], pt.c0);
      for (const int *j = lo; j < ci.data() + rp[m + 1] && *j < pt.c0 + pt.chans; ++j) {
        t.ent.push_back((int)(base[pt.grp] + (j - ci.data())));
        t.pk.push_back((r << 16) | (pt.rows + (*j - pt.c0)));
      }
    }
    const int words[kPwTileWords] = {pt.grp, pt.row0, pt.rows, pt.c0, pt.chans, first, (int)t.ent.size() - first, 0};
    t.tile.insert(t.tile.end(), words, words + kPwTileWords);
  }
  if (t.tile.empty()) t.tile.assign(kPwTileWords, 0);
  if (t.ent.empty()) {
    t.ent.push_back(0);
    t.pk.push_back(0);
  }
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
  t.ktab = im2col_ktab(g, tile_k);
  return t;
}

std::vector<int> im2col_ktab(const Geometry &g, int tile_k) {
  const escoin_conv_desc &d = g.d;
  const int ktiles = (g.kdim + tile_k - 1) / tile_k;
  std::vector<int> ktab(at_least_one(4L * ktiles * tile_k), 0);
  for (int k = 0; k < g.kdim; ++k) {
    const Tap tap = decode_tap(k, d.KH, d.KW);
    const int dy = tap.kr * d.dil_h, dx = tap.kc * d.dil_w;
    ktab[4 * (size_t)k] = (tap.ic * d.H + dy) * d.W + dx;
    ktab[4 * (size_t)k + 1] = dy;
    ktab[4 * (size_t)k + 2] = dx;
    ktab[4 * (size_t)k + 3] = 1;
  }
  return ktab;
}

DgmTables dgrad_mfma_tables(const CsrView &v, const DgmPlan &plan) {
  const Geometry &g = *v.g;
  const escoin_conv_desc &d = g.d;
  const int P = plan.phases_h * plan.phases_w;
  const long opix = (long)g.OH * g.OW;
  DgmTables t;
  t.phase.assign(8 * (size_t)P, 0);
  t.tap_ptr.assign((size_t)P + 1, 0);
  // a tap's rank among the taps of its residue, per axis: its place in the phase's ascending tap list
  std::vector<int> rank_h(d.KH), rank_w(d.KW);
  for (int kr = 0; kr < d.KH; ++kr) {
    rank_h[kr] = 0;
    for (int q = 0; q < kr; ++q) rank_h[kr] += (int)((long)q * d.dil_h % d.stride_h == (long)kr * d.dil_h % d.stride_h);
  }
  for (int kc = 0; kc < d.KW; ++kc) {
    rank_w[kc] = 0;
    for (int q = 0; q < kc; ++q) rank_w[kc] += (int)((long)q * d.dil_w % d.stride_w == (long)kc * d.dil_w % d.stride_w);
  }
  t.col.assign(at_least_one(4 * plan.cols_total), 0);
  std::vector<int> col0((size_t)P, 0);
  long cols = 0;
  for (int ph = 0; ph < P; ++ph) {
    const DgmPhase &f = plan.phase[(size_t)ph];
    const int rh = ph / plan.phases_w, rw = ph - rh * plan.phases_w;
    const int ntaps = f.taps_h * f.taps_w;
    col0[(size_t)ph] = (int)cols;
    int *row = t.phase.data() + 8 * (size_t)ph;
    row[0] = f.h0, row[1] = f.w0, row[2] = f.rows, row[3] = f.cols, row[4] = f.kp, row[5] = f.ksteps, row[6] = (int)cols, row[7] = ntaps;
    for (int kr = 0; kr < d.KH; ++kr)
      for (int kc = 0; kc < d.KW; ++kc) {
        if ((long)kr * d.dil_h % d.stride_h != rh || (long)kc * d.dil_w % d.stride_w != rw) continue;
        t.taps.push_back(kr << 8 | kc);
        const int tap = rank_h[kr] * f.taps_w + rank_w[kc];
        const int dh = (f.h0 + d.pad_h - kr * d.dil_h) / d.stride_h, dw = (f.w0 + d.pad_w - kc * d.dil_w) / d.stride_w;
        for (int ocl = 0; ocl < g.Mg; ++ocl) {
          int *c = t.col.data() + 4 * (size_t)(cols + (long)ocl * ntaps + tap);
          c[0] = (int)(ocl * opix), c[1] = dh, c[2] = dw, c[3] = 1;
        }
      }
    t.tap_ptr[(size_t)ph + 1] = (int)t.taps.size();
    cols += (long)f.ksteps * plan.step_k;
  }
  if (t.taps.empty()) t.taps.push_back(0);
  // the entries' places, and which steps of which (group, phase, channel tile) hold one
  t.pos.assign(at_least_one(v.nnz()), 0);
  const size_t lists = (size_t)d.group * P * plan.ctiles;
  std::vector<std::vector<char>> has(lists);
  for_each_entry(v, [&](const CsrEntry &c) {
    const Tap tap = decode_tap(c.col, d.KH, d.KW);
    const int ph = (int)((long)tap.kr * d.dil_h % d.stride_h) * plan.phases_w + (int)((long)tap.kc * d.dil_w % d.stride_w);
    const DgmPhase &f = plan.phase[(size_t)ph];
    const int k = c.m * (f.taps_h * f.taps_w) + rank_h[tap.kr] * f.taps_w + rank_w[tap.kc];
    const int ct = tap.ic / plan.tile_c;
    t.pos[(size_t)c.e] = (int)((((long)c.grp * plan.ctiles + ct) * plan.cols_total + col0[(size_t)ph] + k) * plan.tile_c + tap.ic % plan.tile_c);
    std::vector<char> &h = has[((size_t)c.grp * P + ph) * plan.ctiles + ct];
    if (h.empty()) h.assign((size_t)f.ksteps, 0);
    h[(size_t)(k / plan.step_k)] = 1;
  });
  t.live_ptr.assign(lists + 1, 0);
  for (size_t l = 0; l < lists; ++l) {
    for (size_t s = 0; s < has[l].size(); ++s)
      if (has[l][s]) t.live.push_back((int)s);
    t.live_ptr[l + 1] = (int)t.live.size();
  }
  if (t.live.empty()) t.live.push_back(0);
  return t;
}

DerivedCsr s2d_csr(const CsrView &v, const S2dPlan &sp) {
  const Geometry &g = *v.g;
  const escoin_conv_desc &d = g.d;
  const int kh = sp.inner.KH, kw = sp.inner.KW;
  DerivedCsr t;
  t.rowptr.assign((size_t)d.group * (g.Mg + 1), 0);
  t.nnz_g.assign(d.group, 0);
  t.colidx.reserve((size_t)v.nnz());
  t.src.reserve((size_t)v.nnz());
  // per row: (inner column, flat index of the outer entry), sorted -- the columns of a row are distinct, so the order is
  // a function of the pattern alone
  std::vector<std::pair<int, int>> row;
  long base = 0;
  for (int grp = 0; grp < d.group; ++grp) {
    const std::vector<int> &rp = (*v.rowptr)[grp], &ci = (*v.colidx)[grp];
    int *irp = t.rowptr.data() + (size_t)grp * (g.Mg + 1);
    for (int m = 0; m < g.Mg; ++m) {
      row.clear();
      for (int j = rp[m]; j < rp[m + 1]; ++j) {
        const Tap tap = decode_tap(ci[j], d.KH, d.KW);
        const int c_in = (tap.ic * sp.PH + tap.kr % d.stride_h) * sp.PW + tap.kc % d.stride_w;
        row.emplace_back((c_in * kh + tap.kr / d.stride_h) * kw + tap.kc / d.stride_w, (int)(base + j));
      }
      std::sort(row.begin(), row.end());
      for (const auto &e : row) {
        t.colidx.push_back(e.first);
        t.src.push_back(e.second);
      }
      irp[m + 1] = irp[m] + (int)row.size();
    }
    t.nnz_g[grp] = irp[g.Mg];
    base += (long)ci.size();
  }
  return t;
}

DerivedCsr d2s_csr(const CsrView &v, const D2sPlan &dp) {
  const Geometry &g = *v.g;      // the mirror convolution's: g.Mg = the bottom's channels per group, g.Cg = the top's
  const escoin_conv_desc &d = g.d;
  const int kh = dp.inner.KH, kw = dp.inner.KW, sh = dp.sh, sw = dp.sw;
  const int rows_g = g.Cg * dp.P;
  DerivedCsr t;
  t.rowptr.assign((size_t)d.group * (rows_g + 1), 0);
  t.nnz_g.assign(d.group, 0);
  t.colidx.resize((size_t)v.nnz());
  t.src.resize((size_t)v.nnz());
  // a counting sort by inner row, then each row by (inner column, outer entry): the columns of a row are distinct, so the
  // order is a function of the pattern alone
  std::vector<std::pair<int, int>> row;
  long base = 0;
  for (int grp = 0; grp < d.group; ++grp) {
    const std::vector<int> &rp = (*v.rowptr)[grp], &ci = (*v.colidx)[grp];
    int *irp = t.rowptr.data() + (size_t)grp * (rows_g + 1);
    auto inner_row = [&](int col) {
      const Tap tap = decode_tap(col, d.KH, d.KW);
      return (tap.ic * sh + tap.kr % sh) * sw + tap.kc % sw;
    };
    for (size_t j = 0; j < ci.size(); ++j) ++irp[inner_row(ci[j]) + 1];
    for (int r = 0; r < rows_g; ++r) irp[r + 1] += irp[r];
    std::vector<int> at(irp, irp + rows_g);
    for (int cl = 0; cl < g.Mg; ++cl)
      for (int j = rp[cl]; j < rp[cl + 1]; ++j) {
        const Tap tap = decode_tap(ci[j], d.KH, d.KW);
        const size_t k = (size_t)base + (size_t)at[inner_row(ci[j])]++;
        t.colidx[k] = (cl * kh + (kh - 1 - tap.kr / sh)) * kw + (kw - 1 - tap.kc / sw);
        t.src[k] = (int)(base + j);
      }
    for (int r = 0; r < rows_g; ++r) {
      row.clear();
      for (int k = irp[r]; k < irp[r + 1]; ++k) row.emplace_back(t.colidx[(size_t)base + k], t.src[(size_t)base + k]);
      std::sort(row.begin(), row.end());
      for (int k = irp[r]; k < irp[r + 1]; ++k) {
        t.colidx[(size_t)base + k] = row[(size_t)(k - irp[r])].first;
        t.src[(size_t)base + k] = row[(size_t)(k - irp[r])].second;
      }
    }
    t.nnz_g[grp] = irp[rows_g];
    base += (long)ci.size();
  }
  return t;
}

bool compose_maps(const std::vector<int> *outer, const std::vector<int> *inner, long n, std::vector<int> *out) {
  if (n < 0 || (outer && (long)outer->size() != n)) return false;
  std::vector<int> r(inner ? inner->size() : (size_t)n);
  for (size_t k = 0; k < r.size(); ++k) {
    const int j = inner ? (*inner)[k] : (int)k;
    if (j < 0 || (long)j >= n) return false;
    r[k] = outer ? (*outer)[(size_t)j] : j;
  }
  out->swap(r);
  return true;
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
