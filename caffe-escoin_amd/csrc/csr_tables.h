// csr_tables.h -- every integer table the library derives from a plan's host CSR, and the one walk over that CSR they
// are built with.  Pure C++ (no HIP, no escoin_plan), like align_rules.h: a builder takes the CSR and plain integers and
// returns plain vectors, so that the indices that decide which device word a weight is written to and which LDS float a
// tap reads are checked on a machine without a GPU (tests/test_csr_tables.py).  The .hip files call these and do the
// device work: upload, synchronise.
//
// Lengths: DeviceBuffer::upload allocates what it is handed, and a kernel argument may not be a null pointer, so the
// tables that an empty pattern would leave empty are padded to one (zero) element: generic_tables' taps,
// dense_positions, gather_transpose's ttap.  staged_tables' off is padded by two batches of zeros, which the staged
// kernel's walk reads ahead into.  wgrad_mfma_tables' ent has M * kdim elements whatever the pattern; dgrad_mfma_tables'
// taps, col, pos and live are padded to one element.  The host-side
// lists (tsrc) have exactly nnz elements.
#ifndef ESCOIN_CSR_TABLES_H_
#define ESCOIN_CSR_TABLES_H_

#include <cstddef>
#include <vector>

#include "geometry.h"

namespace escoin {

// The host CSR of a plan, per conv group (escoin_plan::rowptr / colidx): rows are the group's Mg output channels,
// columns the taps of its Cg input channels, ascending within a row.
struct CsrView {
  const Geometry *g;
  const std::vector<std::vector<int>> *rowptr, *colidx;   // [group][Mg + 1], [group][nnz of the group]
  long nnz() const {
    long n = 0;
    for (const auto &c : *colidx) n += (long)c.size();
    return n;
  }
  // flat index (groups concatenated) of group grp's first entry
  long group_base(int grp) const {
    long n = 0;
    for (int k = 0; k < grp; ++k) n += (long)(*colidx)[k].size();
    return n;
  }
};

// Entry j of group grp's CSR: in row m (group-local output channel), at column col; e = its flat index.
struct CsrEntry {
  int grp, m, j;
  long e;
  int col;
};

// The walk: every entry once, in CSR order (group, row, column), which is the order of e.
template <typename F>
inline void for_each_entry(const CsrView &v, F &&fn) {
  long e = 0;
  for (int grp = 0; grp < v.g->d.group; ++grp) {
    const std::vector<int> &rp = (*v.rowptr)[grp], &ci = (*v.colidx)[grp];
    for (int m = 0; m < v.g->Mg; ++m)
      for (int j = rp[m]; j < rp[m + 1]; ++j, ++e) fn(CsrEntry{grp, m, j, e, ci[j]});
  }
}

// Per-group arrays of the CSR (its values) in flat order, at least min_size elements long.
template <typename T>
inline std::vector<T> flat_entries(const std::vector<std::vector<T>> &per_group, size_t min_size = 0) {
  std::vector<T> out;
  for (const auto &v : per_group) out.insert(out.end(), v.begin(), v.end());
  if (out.size() < min_size) out.resize(min_size);
  return out;
}

// The generic kernel's device CSR (also the entry weight-gradient kernel's): rowptr [M + 1] absolute, taps
// [max(nnz, 1)] = pack_tap(ic, kr, kc).
struct GenericTables { std::vector<int> rowptr, taps; };
GenericTables generic_tables(const CsrView &v);

// [max(nnz, 1)]: (grp * Mg + m) * row_stride + col -- the entry's position in a dense M x row_stride matrix.
// row_stride = kdim: its position in blobs_[0] (wpos); row_stride = dense_lda(kdim): in the MFMA kernel's matrix.
std::vector<int> dense_positions(const CsrView &v, int row_stride);

// The gather kernel's transposed CSR: per global input channel c the entries of rows trow[c] .. trow[c + 1], in
// ascending (ocl, kr, kc) -- the order the original rows visit them in when they are walked oc by oc.
// trow [C + 1], ttap [max(nnz, 1)] = pack_tap(ocl, kr, kc), tsrc [nnz] = the flat index of the entry at that place
// (its value: values_flat[tsrc[k]]).  The CPU mode's data gradient walks the same trow / tsrc.
struct GatherTables { std::vector<int> trow, ttap, tsrc; };
GatherTables gather_transpose(const CsrView &v);

// The CSR of a derived plan (escoin_plan.h DerivedPlan) in set_csr's form -- rowptr group-relative, colidx [nnz], nnz_g
// [group] -- and its entry map src [nnz]: entry k holds the value of this CSR's entry src[k] (values_flat[src[k]]).
struct DerivedCsr { std::vector<int> rowptr, colidx, nnz_g, src; };

// The CSR of the transposed forward plan (the data gradient as a stride-1 forward of top_diff), in set_csr's form:
// per group, row = input channel icl, entry (ocl, icl, kr, kc) at column ocl*KH*KW + (KH-1-kr)*KW + (KW-1-kc), ascending
// within the row.  rowptr [group * (Cg + 1)]; src [nnz]: the flat index of the entry at that place.
DerivedCsr forward_transpose(const CsrView &v);

// The staged weight-gradient kernel's tables for blocks of icb input channels, nblk per conv group, cs floats per staged
// channel, rows of Wp floats: blk [M * (nblk + 1)], blk[oc * (nblk + 1) + b] = the flat index where output channel oc's
// entries of block b begin (b = nblk: where the row ends); off [nnz + 2 * kStgBatch], the entry's tap as a float offset
// inside the staged block's LDS tile, (icl % icb) * cs + kr * dil_h * Wp + kc * dil_w, then zeros.
struct StagedTables { std::vector<int> blk, off; };
StagedTables staged_tables(const CsrView &v, int icb, int nblk, int cs, int Wp);

// The MFMA weight-gradient kernel's tables for tiles of tile_m output channels x tile_k columns, mtiles x ktiles per conv
// group: ent [max(M * kdim, 1)], ent[(grp * Mg + m) * kdim + col] = the flat index of the CSR entry at that (row, column),
// -1 where the pattern has none -- the inverse of dense_positions(v, kdim); tile_cnt [group * mtiles * ktiles], the
// entries inside tile (grp, mt, kt) at [(grp * mtiles + mt) * ktiles + kt] (a workgroup whose tile holds none leaves at
// once); ktab [4 * ktiles * tile_k], the im2col decode of column k as four ints: the element offset of its tap inside a
// conv group's image (ic * H + kr * dil_h) * W + kc * dil_w, dy = kr * dil_h, dx = kc * dil_w, 1; the columns at or
// past kdim (the last tile's padding) carry {0, 0, 0, 0}: "no such column".
struct WgmTables { std::vector<int> ent, tile_cnt, ktab; };
WgmTables wgrad_mfma_tables(const CsrView &v, int tile_m, int tile_k);
// That ktab alone: a function of the geometry, no CSR (the dense weight gradient's state, dense_wgrad.hip, needs no more).
std::vector<int> im2col_ktab(const Geometry &g, int tile_k);

// The pointwise weight-gradient kernel's tables for a tiling of align_rules.h pw_plan made ON THIS PATTERN (its tiles' item
// counts are then the counts found here).  tile [kPwTileWords * max(tiles, 1)]: per tile, in the plan's order, {group,
// first row, rows, first channel, channels, first item, items, 0}.  A tile's items are its entries in CSR order -- lane l
// of the workgroup takes items l, l + 256, ... -- and item i has ent[i] = the entry's flat index and pk[i] = (G row << 16) |
// bottom row, both rows of the tile's LDS image: G row = m - first row in [0, rows), bottom row = rows + (c - first
// channel) in [rows, rows + channels).  ent and pk have max(nnz, 1) elements: every entry is an item of exactly one tile.
constexpr int kPwTileWords = 8;
struct PwPlan;
struct PwTables { std::vector<int> tile, ent, pk; };
PwTables pw_tables(const CsrView &v, const PwPlan &plan);

// The MFMA data-gradient kernel's tables for a tile plan of align_rules.h dgm_plan (P phases, phase index = row residue *
// stride_w + column residue; ctiles channel tiles of tile_c per conv group; steps of step_k columns):
//   phase    [8 * P]: {h0, w0, rows, cols, kp, ksteps, col0, ntaps} -- the phase's bottom pixels are (h0 + stride_h * hh,
//            w0 + stride_w * ww), hh < rows, ww < cols; kp = Mg * ntaps columns in ksteps steps; col0 = its first column in
//            `col` and in the matrices;
//   tap_ptr  [P + 1], taps [max(sum of ntaps, 1)]: the phase's taps kr << 8 | kc, ascending -- the (kr, kc) with
//            kr * dil_h % stride_h and kc * dil_w % stride_w equal to the phase's residues (host side only);
//   col      [4 * cols_total]: column k of a phase, k = ocl * ntaps + t, at col0 + k as four ints {ocl * OH * OW, dh, dw, 1}:
//            tap t of pixel (hh, ww) reads G[ocl][hh + dh][ww + dw], dh = (h0 + pad_h - kr * dil_h) / stride_h (exact), dw
//            likewise; the columns at or past kp (the last step's padding) carry {0, 0, 0, 0};
//   the phase matrices: one transposed dense copy of the weights, mat_floats floats, zero where the pattern has no entry.
//            Block (grp, ct) holds cols_total rows of tile_c floats: the weight of (column col0 + k of the phase, input
//            channel ct * tile_c + i) at ((grp * ctiles + ct) * cols_total + col0 + k) * tile_c + i -- a step's 64 x 32
//            block is contiguous, and so is what a wave loads of it;
//   pos      [max(nnz, 1)]: the one matrix element that holds CSR entry e (how weight updates reach the matrix);
//   live_ptr [group * P * ctiles + 1], live [max(total, 1)]: per (grp, phase, ct), at (grp * P + phase) * ctiles + ct, the
//            ascending steps whose 64 x 32 weight block holds a CSR entry.  An empty list: the tile's pixels are zeros.
struct DgmPlan;
struct DgmTables { std::vector<int> phase, tap_ptr, taps, col, pos, live_ptr, live; };
DgmTables dgrad_mfma_tables(const CsrView &v, const DgmPlan &plan);

// The CSR of the inner stride-1 plan of option "s2d" (align_rules.h s2d_plan), in set_csr's form: per group, row = output
// channel ocl, entry (ocl, ic, kr, kc) at column (c' * KH' + kr / stride_h) * KW' + kc / stride_w with c' = (ic * PH +
// kr % stride_h) * PW + kc % stride_w (group-local), ascending within the row -- a permutation of the outer order inside
// each row.  rowptr [group * (Mg + 1)] group-relative, colidx [nnz], nnz_g [group], src [nnz]: inner entry k holds the
// value of outer entry src[k] (flat index, groups concatenated).  The map is injective; an inner position without a
// preimage is never an entry.
struct S2dPlan;
DerivedCsr s2d_csr(const CsrView &v, const S2dPlan &sp);

// The CSR of the inner stride-1 plan of option "deconv" (align_rules.h d2s_plan), in set_csr's form.  `v` is the layer's own
// CSR, held in the mirror convolution's geometry (dp.mirror): per group, row = bottom channel cl, column = ml * KH * KW +
// kr * KW + kc.  Entry (cl, ml, kr, kc) becomes the entry of inner row m' = (ml * sh + kr % sh) * sw + kc % sw (group-local,
// Mg * P rows per group) at column (cl * KH' + (KH' - 1 - kr / sh)) * KW' + (KW' - 1 - kc / sw), ascending within the row.
// rowptr [group * (Mg * P + 1)] group-relative, colidx [nnz], nnz_g [group], src [nnz]: inner entry k holds the value of
// outer entry src[k] (flat index, groups concatenated).  The map is injective; the rows of phases without a tap are empty.
struct D2sPlan;
DerivedCsr d2s_csr(const CsrView &v, const D2sPlan &dp);

// Two entry maps in a row, out[k] = outer[inner[k]]: entry k holds the value of entry inner[k] of a plan of n entries, whose
// entry j holds that of entry outer[j].  A null side is the identity over [0, n).  false, and *out as it was: `outer` has
// not n elements, or an index of `inner` lies outside [0, n).
bool compose_maps(const std::vector<int> *outer, const std::vector<int> *inner, long n, std::vector<int> *out);

// A scatter list (destination k: CSR entry src[k], element off[k] of buffer buf[k]) entry-major: entry e's destinations
// are e_off[k] / e_buf[k] for k in [e_ptr[e], e_ptr[e + 1]), in the order of the list.  e_ptr [max(nnz, 1) + 1], e_off
// and e_buf [max(n, 1)] for a list of n.  false (and nothing built): a destination names no CSR entry.
struct EntryMajor {
  std::vector<int> e_ptr;
  std::vector<unsigned> e_off;
  std::vector<unsigned char> e_buf;
};
bool entry_major(const std::vector<int> &src, const std::vector<unsigned> &off, const std::vector<unsigned char> &buf,
                 long nnz, EntryMajor *out);

// Column col of the CSR as the reference stretches it for its padded input image (base_conv_layer.cpp:99-105).
int stretched_col(int col, const escoin_conv_desc &d);

}  // namespace escoin
#endif  // ESCOIN_CSR_TABLES_H_
