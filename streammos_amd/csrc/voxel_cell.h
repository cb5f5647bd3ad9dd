// Cell side of the point -> grid max-pool scatter: the geometry and the cell a point falls into.  One definition for the
// scatter kernels (csrc/voxel_maxpool.hip) and the fused training transfers (csrc/gather_scatter_train.hip).
#pragma once
#include "smos_common.h"

namespace smos {

struct VmpGeom {
  int32_t D;
  int64_t size[4];
  int64_t sstride[4];  // spatial strides of out (elements)
  float scale[4];
  int64_t out_b, out_c;      // batch / channel stride of out
  int64_t fs_b, fs_c, fs_n;  // feature strides
};

// Flat spatial offset of a point, or -1 when it is dropped.
// reference: point_deep_cuda_kernel.cu:39-47 -- int64(float(coord) * scale), kept iff 0 <= cell < size.
// trunc(p) >= 0  <=>  p > -1 and trunc(p) < size  <=>  p < size (size is an integer).
__device__ __forceinline__ int64_t cell_offset(const float* __restrict__ ind_row, const VmpGeom& g) {
  int64_t off = 0;
  bool ok = true;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    if (d < g.D) {
      float p = __fmul_rn(ind_row[d], g.scale[d]);
      bool in = (p > -1.0f) && (p < (float)g.size[d]);
      ok = ok && in;
      off += (int64_t)(in ? (int)p : 0) * g.sstride[d];
    }
  }
  return ok ? off : (int64_t)-1;
}

}  // namespace smos
