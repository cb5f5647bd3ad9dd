// The align_corners=True interpolation taps of the decoder's conv_1 path: one definition for the forward (csrc/upconv.hip)
// and for its adjoint (csrc/upconv_bwd.hip), so that the backward applies exactly the float32 weights the forward applied.
#pragma once
#include "smos_common.h"

namespace smos {

struct Lerp {
  int i0, step;     // source index and 0/1 step to the second tap
  float w0, w1;
};

__device__ __forceinline__ Lerp lerp_of(int dst, int n_src, int n_dst) {
  const float r = n_dst > 1 ? (float)(n_src - 1) / (float)(n_dst - 1) : 0.0f;
  const float s = r * dst;
  Lerp l;
  l.i0 = (int)s;
  l.step = (l.i0 < n_src - 1) ? 1 : 0;
  l.w1 = s - l.i0;
  l.w0 = 1.0f - l.w1;
  return l;
}

// one bilinear tap pair added to four channels
__device__ __forceinline__ void lerp_add(float4& acc, float w0, float w1, const float4& a0, const float4& a1) {
  acc.x += w0 * a0.x + w1 * a1.x; acc.y += w0 * a0.y + w1 * a1.y;
  acc.z += w0 * a0.z + w1 * a1.z; acc.w += w0 * a0.w + w1 * a1.w;
}

}  // namespace smos
