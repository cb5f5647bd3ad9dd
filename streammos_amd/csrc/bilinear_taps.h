// Position side of the grid -> point bilinear gather: geometry, the float32 pixel position and the four taps.  One
// definition for the forward and the atomic backward (csrc/bilinear_gather.hip) and for the fixed-order backward
// (csrc/segsum.hip) and for the fused training transfers (csrc/gather_scatter_train.hip): the same taps and weights to the bit.
#pragma once
#include "smos_common.h"

namespace smos {

struct BilGeom {
  int64_t gs_b, gs_c, gs_h, gs_w;  // grid strides
  int64_t os_b, os_c, os_n;        // out strides
  int32_t H, W, K;
  float sy, sx;
};

struct Taps {
  int64_t o[4];
  float w[4];
  int y0, x0;  // cell of the north-west tap (-5, -5: not a finite position near the map)
};

// pixel position exactly as backbone.py:467-468 + ATen's grid_sampler_unnormalize(align_corners=True)
__device__ __forceinline__ float pixel_pos(float c, float s, int size) {
  const float sm1 = (float)(size - 1);
  float gn = __fsub_rn(__fdiv_rn(__fmul_rn(__fmul_rn(2.0f, c), s), sm1), 1.0f);
  return __fmul_rn(__fdiv_rn(__fadd_rn(gn, 1.0f), 2.0f), sm1);
}

__device__ __forceinline__ Taps make_taps(const float* __restrict__ crow, const BilGeom& g) {
  Taps t;
  const float iy = pixel_pos(crow[0], g.sy, g.H);
  const float ix = pixel_pos(crow[1], g.sx, g.W);
  const float fy = floorf(iy), fx = floorf(ix);
  // weights in ATen's order: nw, ne, sw, se (GridSampler: nw = (ix_se - ix) * (iy_se - iy), ...)
  const float wx1 = ix - fx, wx0 = (fx + 1.0f) - ix;
  const float wy1 = iy - fy, wy0 = (fy + 1.0f) - iy;
  t.w[0] = wx0 * wy0;
  t.w[1] = wx1 * wy0;
  t.w[2] = wx0 * wy1;
  t.w[3] = wx1 * wy1;
  // NaN / far-away coordinates (the reference's -1000 / -4000 padding rows) fail every range test
  const bool finite = (iy > -2.0f) && (iy < (float)(g.H + 1)) && (ix > -2.0f) && (ix < (float)(g.W + 1));
  const int y0 = finite ? (int)fy : -5, x0 = finite ? (int)fx : -5;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = y0 + (k >> 1), x = x0 + (k & 1);
    const bool in = (y >= 0) && (y < g.H) && (x >= 0) && (x < g.W);
    t.o[k] = in ? (int64_t)y * g.gs_h + (int64_t)x * g.gs_w : (int64_t)-1;
    if (!in) t.w[k] = 0.0f;
  }
  t.y0 = y0;
  t.x0 = x0;
  return t;
}

// ---- wave tiles of the row-atomic backward (bil_bwd_rows, and gst_bwd_rows of csrc/gather_scatter_train.hip) ----
constexpr int kBt = 32;      // points per wave tile
constexpr int kBPitch = 66;  // floats per LDS row: the fill's lane (p, h) writes bank (2 p + 2 j + h) mod 64, all different

__device__ __forceinline__ void bwd_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float lane_f(float v, int i) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), i));
}

}  // namespace smos
