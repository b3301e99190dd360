// aligned_form.h -- the persisted aligned form: the blob escoin_plan_export_aligned writes and escoin_plan_import_aligned
// reads (a broadcast receiver and --load-aligned trust it).  Pure C++ (no HIP, no escoin_plan): everything that knows the
// byte layout lives here, once -- sizes, writers and the parsers whose checks decide whether bytes from another process
// become a plan's CSR and the machine code its kernel calls.  The parsers are functions of the bytes, the geometry and
// what the caller says about its device and plan (CodeFit), so they run, and are fuzzed under sanitizers, on a machine
// without a GPU (tests/test_aligned_form.py).  The .hip files do the device work around them: escoin_capi.hip validates
// and uploads the CSR, sconv_tiled.hip loads the code.
//
//   [AlignedHdr][desc][nnz_per_group][rowptr][colidx][values][code section]
//   code section: [AlignedJitHdr][28 ints of the Tiling][unit_off][chan][code words]      (absent: no generated code)
//
// The sections sit at arbitrary byte offsets: every field is read and written with memcpy.
#ifndef ESCOIN_ALIGNED_FORM_H_
#define ESCOIN_ALIGNED_FORM_H_

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "align_rules.h"
#include "geometry.h"
#include "stream_builder.h"

namespace escoin {

// ---- the outer container ---------------------------------------------------------------------------------------------
constexpr uint32_t kAlignedMagic = 0x4E474C41u;   // "ALGN"
constexpr uint32_t kAlignedVersion = 2u;          // 2: content tags over the CSR and the code section (round 6)
struct AlignedHdr {
  uint32_t magic, version;
  uint64_t total_bytes, nnz, jit_bytes;
  // Content tags: 64-bit hashes of the CSR section (descriptor included) and of the generated-code section, and a
  // third one binding the two -- the code was generated FROM this CSR.  A blob whose sections come from different
  // exports (a torn or spliced broadcast, a stale cache file patched with new weights) is refused instead of running
  // code that disagrees with its CSR.  Not a security boundary: an integrity check against accidents.
  uint64_t csr_tag, jit_tag, pair_tag;
};

// 4 x 64-bit multiply-rotate lanes over 32-byte stripes (the shape of XXH64's main loop): ~10 GB/s on a host core, so
// tagging the 54 MB of the 16 ResNet layers costs ~5 ms per side.  seed: 1 the CSR section, 2 the code section.
uint64_t content_tag(const void *data, size_t n, uint64_t seed);
uint64_t pair_tag_of(uint64_t csr_tag, uint64_t jit_tag);

// Bytes of the blob of a layer with nnz nonzeros and a serialised code section of code_section_bytes.
size_t aligned_bytes(const Geometry &g, uint64_t nnz, size_t code_section_bytes);
// Fills buf (aligned_bytes(...) bytes) from the host CSR and the serialised code section, tags included.
void aligned_write(const Geometry &g, const CsrIndex &rowptr, const CsrIndex &colidx, const CsrValues &values,
                   const std::vector<char> &code_section, void *buf);

// What aligned_parse found: rc != ESCOIN_OK with its message (nothing else is then valid), or the pieces of the blob.
struct AlignedForm {
  int rc = ESCOIN_OK;
  std::string error;
  escoin_conv_desc d;                    // the exporting plan's descriptor
  std::vector<int> nnz_per_group, rowptr, colidx;      // as escoin_plan_set_csr takes them (not yet validated as a CSR)
  std::vector<float> values;
  const char *code_section = nullptr;    // inside buf; code_section_bytes == 0: none
  size_t code_section_bytes = 0;
  bool same_geom = false;                // the code section only counts for the geometry it was generated for (the LDS
                                         // offsets in the code are that H x W's) and the same batch
};
// g: the importing plan's.  The weights' own geometry must match (C, M, kernel, group); batch, bias and ReLU are the
// importing plan's business.  Both content tags are checked before a byte of either section is trusted.
AlignedForm aligned_parse(const void *buf, size_t bytes, const Geometry &g);

// ---- the code section: the persisted form of a generated-code plan -----------------------------------------------------
// Valid for the library build that wrote it (kAlignedJitVersion covers the register contract between the kernel body
// and the generated code) on a device with the same number of compute units and the same ISA.
constexpr uint32_t kAlignedJitMagic = 0x54494A45u;    // "EJIT"
constexpr uint32_t kAlignedJitVersion = 6001u;        // bump with jit_codegen.h's register contract / TiledArgs
struct AlignedJitHdr {
  uint32_t magic, version, n_cu, n_tiling_ints;
  int32_t nbuf, jit_pref, dma_period, lds_budget, tiling_batch, jit_chain;
  int32_t jit_self_zero, reserved0;   // jit_self_zero: always 1 (the code initialises its accumulators); a blob with 0 does not fit
  float density;
  int32_t n_dense_groups;          // the code was generated with these conv groups on the MFMA kernel (their units
  uint64_t dense_mask;             // are empty): an importer that splits the groups differently must not load it
  int64_t jit_rows, jit_records;
  uint64_t code_bytes, reserved1, n_unit_off, n_chan;
  char isa[32];                    // the exporting device's gcnArchName ("gfx950:sramecc+:xnack-")
};
constexpr int kTilingInts = 28;    // every field of Tiling, as an int32 each (aligned_form.cpp pins it to sizeof(Tiling))

struct CodeSection {
  Tiling tiling;
  int nbuf = 0, jit_pref = 0, dma_period = 0, lds_budget = 0, tiling_batch = 0;
  bool chained = false;
  float density = 0.f;
  int n_dense_groups = 0;
  uint64_t dense_mask = 0;
  long jit_rows = 0, jit_records = 0;
  std::vector<uint32_t> unit_off, chan, code;
};
// What only the device or the plan knows: the blob fits when all of it equals what the exporter recorded.
struct CodeFit {
  int n_cu = 0;
  std::string isa;                 // the device's gcnArchName (its first 31 characters count)
  int tiling_batch = 0;            // the importing plan's option
  int n_dense_groups = 0;          // the split of the conv groups the importing plan's options give: it is part of the
  uint64_t dense_mask = 0;         // code (dense groups have empty units)
};

// The section of s as written on a device of n_cu compute units and ISA `isa`.
std::vector<char> code_section_write(const CodeSection &s, int n_cu, const std::string &isa);
// true: the section is one of this build, this geometry and `fit`, every count and index in it is in range, and *s holds
// it (one copy of the code words).  false: it does not fit -- the caller aligns from the CSR instead.
bool code_section_parse(const char *blob, size_t bytes, const Geometry &g, const CodeFit &fit, CodeSection *s);

}  // namespace escoin
#endif  // ESCOIN_ALIGNED_FORM_H_
