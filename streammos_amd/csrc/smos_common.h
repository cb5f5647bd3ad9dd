// Shared helpers for the gfx950 kernels of libsmos_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/smos.h"

namespace smos {

constexpr int kWave = 64;          // CDNA wavefront
constexpr int kBlock = 256;        // 4 waves, one per SIMD
constexpr int kMaxGrid = 256 * 8;  // 256 CUs x 8 resident blocks: grid-stride beyond that

// Largest element count a 32-bit grid-stride loop (`for (int i = ...; i < total; i += gridDim.x * blockDim.x)`) may be
// given: the counter of the last iteration is up to one grid stride past `total` and must still be a positive int
// (grids are capped at 256 * 32 blocks of kBlock threads = 2^21 elements per stride).
constexpr int64_t kMaxTotal32 = (1LL << 31) - (1LL << 22);

void set_error(const char* fmt, ...);

inline int grid_for(int64_t work_items, int block = kBlock, int64_t cap = kMaxGrid) {
  int64_t g = (work_items + block - 1) / block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return SMOS_ERR_LAUNCH;
  }
  return SMOS_OK;
}

#define SMOS_REQUIRE(cond, ...)          \
  do {                                   \
    if (!(cond)) {                       \
      smos::set_error(__VA_ARGS__);      \
      return SMOS_ERR_ARG;               \
    }                                    \
  } while (0)

// Launch facts of one kernel on ONE device: CU count, the dynamic-LDS opt-in (hipFuncAttributeMaxDynamicSharedMemorySize
// is a per-device attribute) and, if asked for, the resident blocks per CU.  Looked up per (kernel, current device) under
// a mutex, so a process that drives several GPUs -- or several threads -- gets each device set up exactly once.
struct KernelSetup {
  int cus = 0;
  int per_cu = 0;   // hipOccupancyMaxActiveBlocksPerMultiprocessor (0 when not requested)
};
int kernel_setup(const void* fn, size_t dyn_lds_bytes, int occupancy_block, KernelSetup* out, const char* what);

// smos_debug_set_conv_grid_cap: upper bound on the grid of the persistent convolution kernels, of stem_gemm (csrc/stem.hip), of
// pointnet_scatter (csrc/point_fused.hip), of gather_scatter_cl / _cl4 (csrc/cl_kernels.hip), of point_head (csrc/point_head.hip), of tta_argmax (csrc/vote.hip), of the fixed-order backward sums (csrc/segsum.hip), of the fused training transfers (csrc/gather_scatter_train.hip) and of the chunk-striding kernels of both fused training ops
// (csrc/point_mlp_train.hip, csrc/point_head_train.hip, through chunk_grid of csrc/chunk_sums.h) (0 = none).  A test hook: it makes a block walk several work items on shapes small
// enough to check against float64, on any CU count.
int64_t conv_grid_cap(int64_t cap);

// One row of the 4x4 pose difference times (x, y, z, 1) in float64, in the operation order of the dgemm micro-kernel
// numpy's ``mat.dot`` runs for datasets/utils.py:116-126 (one accumulator per output element, k = 0..3, fused
// multiply-adds): written with the round-to-nearest intrinsics so that -ffp-contract has nothing to decide.  The result
// is rounded to float32 once by the caller, as the reference's ``pcds_out[..., :3] = pcds_tmp[..., :3]`` does.
__device__ __forceinline__ double pose_row_f64(const double* m, double x, double y, double z) {
  return __dadd_rn(__fma_rn(m[2], z, __fma_rn(m[1], y, __dmul_rn(m[0], x))), m[3]);
}

// BilinearSample (networks/backbone.py:453-475) on a channels-last map, position side: grid_sample's float32 normalise /
// un-normalise round trip, then the four taps (k = 2 dy + dx) as pixel offsets y * Wg + x (-1: the tap lies outside the map, zeros
// padding) and weights.  One definition for gather_scatter_cl / _cl4 (csrc/cl_kernels.hip) and for the point head that gathers
// its own BEV rows (csrc/point_head.hip): the same bits everywhere.
__device__ __forceinline__ float pix_cl(float c, float s, int size) {
  const float sm1 = (float)(size - 1);
  const float gn = __fsub_rn(__fdiv_rn(__fmul_rn(__fmul_rn(2.0f, c), s), sm1), 1.0f);
  return __fmul_rn(__fdiv_rn(__fadd_rn(gn, 1.0f), 2.0f), sm1);
}

__device__ __forceinline__ void bilinear_taps_cl(float cy, float cx, float gsy, float gsx, int Hg, int Wg, int (&off)[4], float (&wt)[4]) {
  const float iy = pix_cl(cy, gsy, Hg), ix = pix_cl(cx, gsx, Wg);
  const float fy = floorf(iy), fx = floorf(ix);
  const float wx1 = ix - fx, wx0 = (fx + 1.0f) - ix, wy1 = iy - fy, wy0 = (fy + 1.0f) - iy;
  const bool fin = (iy > -2.0f) && (iy < (float)(Hg + 1)) && (ix > -2.0f) && (ix < (float)(Wg + 1));
  const int y0 = fin ? (int)fy : -5, x0 = fin ? (int)fx : -5;
  const float w4[4] = {wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = y0 + (k >> 1), xx = x0 + (k & 1);
    const bool in = (y >= 0) && (y < Hg) && (xx >= 0) && (xx < Wg);
    off[k] = in ? y * Wg + xx : -1;
    wt[k] = in ? w4[k] : 0.0f;
  }
}

// The value side for four channels: the sum over the taps that exist, in tap order (an absent tap is skipped by a select on the
// value, whatever its load returned).
__device__ __forceinline__ float4 bilinear_sum_cl(const float4 (&g)[4], const int (&off)[4], const float (&wt)[4]) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool has = off[k] >= 0;
    v.x = has ? v.x + g[k].x * wt[k] : v.x;
    v.y = has ? v.y + g[k].y * wt[k] : v.y;
    v.z = has ? v.z + g[k].z * wt[k] : v.z;
    v.w = has ? v.w + g[k].w * wt[k] : v.w;
  }
  return v;
}

struct Scale4 {
  float v[4];
};

}  // namespace smos
