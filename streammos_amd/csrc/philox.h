// Philox4x32-10 and the float32 Box-Muller the seeded draws of the training-side kernels use (csrc/train_prep.hip,
// csrc/copy_paste.hip).  One definition: the same bits in both.
#pragma once
#include "smos_common.h"

namespace smos {

// ---- Philox4x32-10 (Salmon et al., SC'11), written out in plain 32/64-bit integer arithmetic ----
struct Philox4 {
  uint32_t v[4];
};

__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                          uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  Philox4 o;
  o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
  return o;
}

// Box-Muller in float32 (cosine branch): u1 in (0, 1], u2 in [0, 1), both exact in float32.
__device__ __forceinline__ float box_muller_f32(uint32_t w1, uint32_t w2) {
  const float u1 = __fmul_rn((float)((w1 >> 8) + 1u), 5.9604644775390625e-8f);
  const float u2 = __fmul_rn((float)(w2 >> 8), 5.9604644775390625e-8f);
  const float r = sqrtf(__fmul_rn(-2.0f, logf(u1)));
  return __fmul_rn(r, cosf(__fmul_rn(6.2831855f, u2)));
}

}  // namespace smos
