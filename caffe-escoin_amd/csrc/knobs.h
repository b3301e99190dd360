// knobs.h -- the library's environment switches, by build flavour.
//
// The PRODUCT build (csrc/Makefile, what __graft_entry__.build() makes) reads two environment variables and
// neither can change a result: ESCOIN_VERBOSE (diagnostics on stderr) and TMPDIR (where the code object manager
// may put temporaries, jit_module.cpp).  Everything else is a compile-time constant there: ESC_KNOB("NAME", d)
// is the literal d, and the name does not even reach the object file (tests/test_capi_cpu.py greps for it).
//
//   -DESCOIN_EXPERIMENTS  (tools/mkabl.sh exp -> libescoin_exp.so): the overrides below are live.  Results stay
//                         within the parity tolerance but may differ in the last bits (another tiling or summation
//                         order); for sweeps and A/B runs.
//   -DESCOIN_STAMPS       (tools/mkabl.sh stamps -> libescoin_stamps.so): implies the above, plus the in-kernel stamp
//                         profiles of the tiled and dense kernels (ESCOIN_PROF=1; -DESCOIN_PROF_STARTUP moves the
//                         tiled kernel's stamps to its start-up).  A profiling run synchronises; results stay right.
//
// Every ESC_KNOB name used in csrc/, one line each (tests/test_capi_cpu.py checks that this list and the sources agree):
//   ESCOIN_WAVES             waves per tiled workgroup (1, 2, 4, 8) instead of 8
//   ESCOIN_LDS_KB            LDS budget of one plane buffer in KiB (4..64) instead of 64 and the per-layer choices
//   ESCOIN_NBUF              plane / staging buffers of the stream kernel: 3 instead of 2
//   ESCOIN_JIT_NBUF          plane buffers of the generated-code kernel: 2 or 3 instead of the per-layer rule
//   ESCOIN_HALF_WG           two 4-wave workgroups per CU for pointwise layers: 0 never, 1 wherever they fit
//   ESCOIN_JIT_DMA_PERIOD    largest quad-table period of the code's own plane DMA (2048)
//   ESCOIN_JIT_DMA_SPREAD    percent of a unit's rows the next block's DMA pieces are spread over (70 / 100 rule)
//   ESCOIN_FILL_WAVES        plane DMA issued by the first n waves of a workgroup only (0: every wave)
//   ESCOIN_XCD_MAP           workgroup columns grouped by XCD: 0 never, 1 wherever there is more than one column
//   ESCOIN_XCD_MIN_CODE_KB   generated code size from which the columns are grouped by XCD (2 MiB)
//   ESCOIN_NT_STORE_MB       pointwise top blobs of at least this many MiB written with non-temporal stores (off)
//   ESCOIN_JIT_YOUNG_PRIO    priority of the second-dispatched half of the waves in generated code (1)
//   ESCOIN_JIT_PRIO_ROWS     rows between s_setprio switches in generated code (4; 0: none)
//   ESCOIN_JIT_PRIO_WAVES    waves whose units switch priority (half the workgroup)
//   ESCOIN_JIT_PREFETCH      code touches in generated code: 0 off, 1 on (per-layer rule)
//   ESCOIN_JIT_DEPTH         rows read ahead in generated code with a tile B (1 or 2; 2)
//   ESCOIN_JIT_DEPTH1        rows read ahead in generated code without a tile B (1..13; 5)
//   ESCOIN_JIT_HI_SETS       extra input sets in tile B's free accumulators (0..24; 24)
//   ESCOIN_DENSE_STREAMK     stream-K on the dense kernel: 0 off, 1 on (per-layer rule)
//   ESCOIN_DMA_GBPS          plane-DMA rate the tiling cost model assumes, GB/s per CU (19)
//   ESCOIN_FORCE_PASSES      tiling: workgroup columns per conv group (0: the model's choice)
//   ESCOIN_FORCE_NSEG        tiling: images per tile (0: the model's choice)
//   ESCOIN_FORCE_TPL         tiling: quads per lane (1 or 2)
//   ESCOIN_PROF              stamps flavour only: 1 = record and print the in-kernel stamp profile
#ifndef ESCOIN_KNOBS_H_
#define ESCOIN_KNOBS_H_

#include <cstdlib>

#if defined(ESCOIN_STAMPS) && !defined(ESCOIN_EXPERIMENTS)
#define ESCOIN_EXPERIMENTS 1
#endif

#ifdef ESCOIN_EXPERIMENTS
namespace escoin {
inline long knob_long(const char *name, long dflt) {
  const char *e = getenv(name);
  return e ? atol(e) : dflt;
}
inline double knob_double(const char *name, double dflt) {
  const char *e = getenv(name);
  return e ? atof(e) : dflt;
}
}  // namespace escoin
#define ESC_KNOB(name, dflt) (::escoin::knob_long("ESCOIN_" name, (dflt)))
#define ESC_KNOB_F(name, dflt) (::escoin::knob_double("ESCOIN_" name, (dflt)))
#define ESC_KNOB_SET(name) (getenv("ESCOIN_" name) != nullptr)
#else
#define ESC_KNOB(name, dflt) ((long)(dflt))
#define ESC_KNOB_F(name, dflt) ((double)(dflt))
#define ESC_KNOB_SET(name) (false)
#endif

#endif  // ESCOIN_KNOBS_H_
