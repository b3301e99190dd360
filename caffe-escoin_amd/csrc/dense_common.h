// dense_common.h -- what the dense forward kernels (dense_mfma.hip: fp32 products; dense_bf16.hip: plan option
// "dense_math" = ESCOIN_MATH_BF16) share: the GEMM view's pixel tile, the launch's argument block.
#pragma once
#include <hip/hip_runtime.h>

namespace escoin {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4d __attribute__((ext_vector_type(4)));

constexpr int kBN = 128;      // pixels per output tile

struct DenseArgs {
  const float *__restrict__ in;
  const float *__restrict__ w;     // dense (M + 128) x lda, zero-padded: rows of lda = K rounded up to 32
  const float *__restrict__ bias;
  const int2 *__restrict__ ktab;   // [K rounded up to 32]: {element offset of tap k in the image, dy | dx << 16}
  float *__restrict__ out;
  int n_images, C, H, W, M, OH, OW;
  int pad_h, pad_w, stride_h, stride_w;
  int Cg, Mg, K, lda, P, relu;
  int n_ptiles, n_mtiles, n_groups;        // tiles: pixel x channel x conv group (of this launch)
  unsigned in_bytes, w_bytes;              // buffer descriptor ranges
  int vec_out;                             // OH*OW % 4 == 0 and top 16-byte aligned: 16-byte stores through LDS
  unsigned long long group_mask;           // conv groups this launch covers (all ones: every group)
  unsigned long long *prof;                // ESCOIN_STAMPS builds: stamp profile [workgroup][wave][8] (ESC_DPROF)
  // stream-K (STREAMK instantiations): every workgroup takes an equal, contiguous run of (tile, k-step) units;
  // a tile cut by a run boundary is finished by the workgroup holding its last k-steps, which adds the others'
  // partial accumulators from `sk_ws` ([workgroup][wave][16 quads][64 lanes] floats x 4) once their `sk_flag`
  // words (zeroed by the launch function before every launch) carry 1
  float *sk_ws;
  unsigned *sk_flag;     // [0 .. gridDim.x): published flags; [gridDim.x]: set when a bounded spin gave up
  unsigned *sk_fail;     // the same give-up, sticky, in pinned HOST memory: the next escoin_forward on the plan fails loudly
};

}  // namespace escoin
