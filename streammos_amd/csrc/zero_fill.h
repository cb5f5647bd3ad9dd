// Zero fill of a [B,C,H,W] gradient destination that arrives uninitialised at any strides: one dense block is a memset,
// anything else a strided fill.  One definition for the backward of the bilinear gather (csrc/bilinear_gather.hip) and of the
// fused training transfers (csrc/gather_scatter_train.hip).
#pragma once
#include "smos_common.h"

namespace smos {

// dims sorted by stride, the smallest last
struct ZeroGeom {
  int64_t size[4], stride[4];
};
static __global__ __launch_bounds__(kBlock) void bil_bwd_zero(float* __restrict__ p, ZeroGeom z, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = i, off = 0;
#pragma unroll
    for (int d = 3; d >= 0; --d) {
      const int64_t q = r / z.size[d];
      off += (r - q * z.size[d]) * z.stride[d];
      r = q;
    }
    p[off] = 0.0f;
  }
}

// `what` names the entry point in error messages
static int zero_destination(float* dst, const int64_t* dst_stride, const int64_t (&size)[4], hipStream_t s, const char* what) {
  ZeroGeom z;
  int order[4] = {0, 1, 2, 3};
  for (int i = 1; i < 4; ++i)
    for (int j = i; j > 0 && dst_stride[order[j]] > dst_stride[order[j - 1]]; --j) {
      const int tmp = order[j]; order[j] = order[j - 1]; order[j - 1] = tmp;
    }
  bool dense = true;
  int64_t expect = 1;
  for (int d = 3; d >= 0; --d) {
    z.size[d] = size[order[d]];
    z.stride[d] = dst_stride[order[d]];
    SMOS_REQUIRE(z.stride[d] >= 0, "%s: negative destination stride", what);
    if (z.size[d] > 1) {
      dense = dense && z.stride[d] == expect;
      expect *= z.size[d];
    }
  }
  const int64_t total = size[0] * size[1] * size[2] * size[3];
  if (dense) {
    if (hipMemsetAsync(dst, 0, (size_t)total * sizeof(float), s) != hipSuccess) return check_launch(what);
    return SMOS_OK;
  }
  hipLaunchKernelGGL(bil_bwd_zero, dim3(grid_for(total, kBlock, 256 * 16)), dim3(kBlock), 0, s, dst, z, total);
  return check_launch(what);
}

}  // namespace smos
