// probe_smfmac.hip -- operand layout of gfx950's v_smfmac_f32_32x32x32_bf16 (2:4 structured-sparse A, dense B).
// One wave.  Per experiment ONE A value is 1 (lane la, element ea of the 8 the lane holds), its 2-bit index field is v,
// every other A value is 0 and every other field 0.  B lane l holds, in element e, the small integer
// 1 + e + 16 * (l / 32) (pass 0: tells WHICH B value of which lane half met the A value) or 1 + l % 32 (pass 1: tells which
// column a lane's B values belong to).  The whole 32 x 32 C is copied out and the host prints, per experiment, the rows
// that are not zero and the value found there: row = the A lane's row, value = the B element the index field selected.
// Three forms are run: (cbsz, abid) = (0, 0) with the fields in bits 0..15 of the index register, (0, 1) with the fields
// in bits 16..31, and (0, 1) with the fields in bits 0..15 (must then read the zero fields of the upper half).
//   hipcc --offload-arch=gfx950 -O2 -o probe_smfmac probe_smfmac.hip && ./probe_smfmac
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x16 __attribute__((ext_vector_type(16)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kLanes[4] = {0, 5, 32, 37};
constexpr int kExp = 4 * 8 * 4;      // (la, ea, v)
constexpr int kForms = 3, kPasses = 2;

// out[((form * kPasses + pass) * kExp + exp) * 1024 + reg * 64 + lane]
__global__ void probe(float *out) {
  const int lane = threadIdx.x;
  for (int pass = 0; pass < kPasses; ++pass) {
    bf16x16 b;
    for (int e = 0; e < 16; ++e) b[e] = (__bf16)(float)(pass == 0 ? 1 + e + 16 * (lane / 32) : 1 + lane % 32);
    for (int x = 0; x < kExp; ++x) {
      const int la = x / 32 == 0 ? kLanes[0] : x / 32 == 1 ? kLanes[1] : x / 32 == 2 ? kLanes[2] : kLanes[3];
      const int ea = (x / 4) % 8, v = x % 4;
      bf16x8 a;
      for (int e = 0; e < 8; ++e) a[e] = (__bf16)((lane == la && e == ea) ? 1.f : 0.f);
      const int lo = lane == la ? v << (2 * ea) : 0;
      const f32x16 z = {0};
      const f32x16 c0 = __builtin_amdgcn_smfmac_f32_32x32x32_bf16(a, b, z, lo, 0, 0);
      const f32x16 c1 = __builtin_amdgcn_smfmac_f32_32x32x32_bf16(a, b, z, lo << 16, 0, 1);
      const f32x16 c2 = __builtin_amdgcn_smfmac_f32_32x32x32_bf16(a, b, z, lo, 0, 1);
      for (int r = 0; r < 16; ++r) {
        out[((size_t)(0 * kPasses + pass) * kExp + x) * 1024 + r * 64 + lane] = c0[r];
        out[((size_t)(1 * kPasses + pass) * kExp + x) * 1024 + r * 64 + lane] = c1[r];
        out[((size_t)(2 * kPasses + pass) * kExp + x) * 1024 + r * 64 + lane] = c2[r];
      }
    }
  }
}

int main() {
  const size_t n = (size_t)kForms * kPasses * kExp * 1024;
  float *d;
  if (hipMalloc(&d, n * 4) != hipSuccess) return 2;
  hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, d);
  std::vector<float> h(n);
  if (hipMemcpy(h.data(), d, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return 3;
  const char *forms[kForms] = {"abid 0, fields in bits 0..15", "abid 1, fields in bits 16..31", "abid 1, fields in bits 0..15"};
  for (int f = 0; f < kForms; ++f) {
    printf("== %s\n", forms[f]);
    for (int x = 0; x < kExp; ++x) {
      printf("A lane %2d elem %d field %d:", kLanes[x / 32], (x / 4) % 8, x % 4);
      for (int pass = 0; pass < kPasses; ++pass) {
        const float *c = &h[((size_t)(f * kPasses + pass) * kExp + x) * 1024];
        // C/D layout of the 32x32 instructions: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
        int rows = 0;
        for (int row = 0; row < 32; ++row) {
          const int reg = (row & 3) + 4 * (row >> 3), half = (row >> 2) & 1;
          const float c0 = c[reg * 64 + 32 * half], c7 = c[reg * 64 + 32 * half + 7];
          if (c0 != 0.f || c7 != 0.f) {
            if (pass == 0) printf("  row %2d: B value %2.0f (half %d elem %2d)", row, c0, ((int)c0 - 1) / 16, ((int)c0 - 1) % 16);
            else printf("  | columns 0, 7 see B lanes %2.0f, %2.0f", c0 - 1, c7 - 1);
            ++rows;
          }
        }
        if (!rows) printf("  (C all zero)");
      }
      printf("\n");
    }
  }
  return 0;
}
