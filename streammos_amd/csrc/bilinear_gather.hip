// Grid -> point bilinear gather for gfx950.
// Replaces networks/backbone.py:453-475 (BilinearSample: F.grid_sample(bilinear, zeros,
// align_corners=True) on a grid built as 2*coord*scale/(size-1) - 1).  The float32 normalise /
// un-normalise round trip of that formulation is reproduced operation by operation (__f*_rn
// intrinsics, so the compiler neither contracts nor reassociates it): the sampling position then
// matches the reference's to the last bit and only the four-tap blend differs by FMA rounding.
//
// Backward (smos_bilinear_gather_bwd): grad_grid += w_k * grad_out over the same four taps, taken from the same make_taps.
// Main form bil_bwd_rows: channels-last destination, lane = channel, so one atomic wave-instruction adds one contiguous
// row segment (the shape at which MI355X's memory-side float atomics reach their chip-wide rate); runs of consecutive
// points in one cell are summed in registers first.  Fallback bil_bwd_points: lane = point, 4-byte atomics at any strides.
// The sums depend on the arrival order of the atomics: last bits can differ from run to run.
#include "smos_common.h"
#include "bilinear_taps.h"
#include "zero_fill.h"

namespace smos {

// lane = point, loop over channels: scattered tap reads (neighbouring points share cache lines),
// coalesced writes when out is channel-major [B,C,N]
__global__ __launch_bounds__(kBlock) void bil_points(const float* __restrict__ grid, const float* __restrict__ coord,
                                                     float* __restrict__ out, BilGeom g, int64_t B, int64_t C,
                                                     int64_t N, int c_chunk) {
  const int64_t total = B * N;
  const int c0 = blockIdx.y * c_chunk;
  const int c1 = (int)min((int64_t)(c0 + c_chunk), C);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / N, n = i - b * N;
    const Taps t = make_taps(coord + i * g.K, g);
    const float* __restrict__ gb = grid + b * g.gs_b;
    float* __restrict__ ob = out + b * g.os_b + n * g.os_n;
    for (int c = c0; c < c1; ++c) {
      const float* gc = gb + (int64_t)c * g.gs_c;
      float acc = 0.0f;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (t.o[k] >= 0) acc += gc[t.o[k]] * t.w[k];
      ob[(int64_t)c * g.os_c] = acc;
    }
  }
}

// lane = channel, a group of kG lanes per point: channels-last grid and point-major out -> every tap
// and every store is one contiguous row
template <int kG>
__global__ __launch_bounds__(kBlock) void bil_rows(const float* __restrict__ grid, const float* __restrict__ coord,
                                                   float* __restrict__ out, BilGeom g, int64_t B, int64_t C,
                                                   int64_t N) {
  constexpr int kGroups = kBlock / kG;
  const int lane = threadIdx.x % kG, grp = threadIdx.x / kG;
  const int64_t total = B * N;
  for (int64_t i = (int64_t)blockIdx.x * kGroups + grp; i < total; i += (int64_t)gridDim.x * kGroups) {
    const int64_t b = i / N, n = i - b * N;
    const Taps t = make_taps(coord + i * g.K, g);
    const float* __restrict__ gb = grid + b * g.gs_b;
    float* __restrict__ ob = out + b * g.os_b + n * g.os_n;
    for (int c = lane; c < C; c += kG) {
      float acc = 0.0f;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (t.o[k] >= 0) acc += gb[t.o[k] + c] * t.w[k];
      ob[c] = acc;
    }
  }
}


// ---- backward ----
// lane = point, loop over channels: 4-byte atomics at the destination's strides (C < 8, or a destination that is not
// channels-last).  BilGeom: gs_* = grad_grid strides, os_* = grad_out strides.  The trip count is the same for every
// lane; a lane past the end works on the last point (clamped address) and its adds are masked: no load sits under a
// lane-dependent branch.
__global__ __launch_bounds__(kBlock) void bil_bwd_points(const float* __restrict__ gout, const float* __restrict__ coord,
                                                         float* __restrict__ ggrid, BilGeom g, int64_t B, int64_t C,
                                                         int64_t N) {
  const int64_t total = B * N;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < total; base += (int64_t)gridDim.x * blockDim.x) {
    const bool has = base + threadIdx.x < total;
    const int64_t i = has ? base + threadIdx.x : total - 1;
    const int64_t b = i / N, n = i - b * N;
    const Taps t = make_taps(coord + i * g.K, g);
    const float* __restrict__ gp = gout + b * g.os_b + n * g.os_n;
    float* __restrict__ db = ggrid + b * g.gs_b;
    for (int64_t c = 0; c < C; ++c) {
      const float x = gp[c * g.os_c];
      float* dc = db + c * g.gs_c;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (has && t.o[k] >= 0) atomicAdd(dc + t.o[k], t.w[k] * x);
    }
  }
}

// A wave owns tiles of kBt consecutive points of one sample.  Lane = point prepares the taps once per tile; then, per chunk
// of 64 channels, lane = channel walks the tile's points: the weights and the cell come from the point's lane by
// v_readlane (wave-uniform), runs of points in one cell are summed in registers, and a run ends with up to four row atomics.
// kStage: grad_out is channel-major, so the tile goes through wave-private LDS (filled along n, read out along c);
// otherwise (stride_c == 1) the rows are read directly.  Every load is unconditional: a lane without a point or a channel
// reads a clamped address and its value is dropped by a select.
template <bool kStage>
__global__ __launch_bounds__(kBlock) void bil_bwd_rows(const float* __restrict__ gout, const float* __restrict__ coord,
                                                       float* __restrict__ ggrid, BilGeom g, int64_t B, int64_t C,
                                                       int64_t N) {
  __shared__ float lds[kStage ? kBlock / kWave : 1][kStage ? kBt * kBPitch : 1];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int p = lane & (kBt - 1), hh = lane >> 5;
  float* tile = lds[kStage ? wave : 0];
  const int64_t tiles_per = (N + kBt - 1) / kBt, n_tiles = B * tiles_per;
  constexpr int kWaves = kBlock / kWave;
  for (int64_t tl = (int64_t)blockIdx.x * kWaves + wave; tl < n_tiles; tl += (int64_t)gridDim.x * kWaves) {
    const int64_t b = tl / tiles_per, n0 = (tl - b * tiles_per) * kBt;
    const int n_valid = (int)min((int64_t)kBt, N - n0);
    const bool has = p < n_valid;
    const int64_t np = n0 + (has ? p : 0);
    Taps t = make_taps(coord + (b * N + np) * g.K, g);
    if (!has) {
      t.y0 = -5;
      t.x0 = -5;
#pragma unroll
      for (int k = 0; k < 4; ++k) t.w[k] = 0.0f;
    }
    const bool any = has && (t.o[0] >= 0 || t.o[1] >= 0 || t.o[2] >= 0 || t.o[3] >= 0);
    if (__ballot(any) == 0) continue;      // padding tail of a scan: nothing to add
    // the shuffles are their own statements (inside a short-circuit expression they would run with lanes masked off)
    const int y_after = __shfl_down(t.y0, 1), x_after = __shfl_down(t.x0, 1);
    const uint32_t tails = (uint32_t)__ballot(hh == 0 && (p == kBt - 1 || t.y0 != y_after || t.x0 != x_after));
    for (int64_t c0 = 0; c0 < C; c0 += kWave) {
      const int cn = (int)min((int64_t)kWave, C - c0);
      const bool chan = lane < cn;
      float v[kBt];
      if (kStage) {
        const float* __restrict__ src = gout + b * g.os_b + np * g.os_n + c0 * g.os_c;
        const int jn = (cn + 1) >> 1;
#pragma unroll 8
        for (int j = 0; j < jn; ++j) {
          const int c = 2 * j + hh;
          const float x = src[(int64_t)(c < cn ? c : 0) * g.os_c];
          tile[p * kBPitch + c] = has ? x : 0.0f;
        }
        bwd_wave_sync();
        // a lane >= cn reads columns this chunk never filled: whatever it sums is dropped by `chan` at the atomics
#pragma unroll
        for (int i = 0; i < kBt; ++i) v[i] = tile[i * kBPitch + lane];
        bwd_wave_sync();
      } else {
        const float* __restrict__ src = gout + b * g.os_b + c0 + (chan ? lane : 0);
#pragma unroll
        for (int i = 0; i < kBt; ++i) {
          const float x = src[(n0 + (i < n_valid ? i : 0)) * g.os_n];
          v[i] = i < n_valid ? x : 0.0f;
        }
      }
      float* __restrict__ dst = ggrid + b * g.gs_b + c0 + lane;
      // A tap outside the map (weight zeroed) is outside for the whole run, since a run is one cell: if a non-finite
      // grad_out turns 0 * v into NaN there, that acc[k] is never added anywhere and is reset with the run.
      float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int i = 0; i < kBt; ++i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = fmaf(lane_f(t.w[k], i), v[i], acc[k]);
        if ((tails >> i) & 1) {
          const int yi = __builtin_amdgcn_readlane(t.y0, i), xi = __builtin_amdgcn_readlane(t.x0, i);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int y = yi + (k >> 1), x = xi + (k & 1);
            if (y >= 0 && y < g.H && x >= 0 && x < g.W && chan) atomicAdd(dst + (int64_t)y * g.gs_h + (int64_t)x * g.gs_w, acc[k]);
            acc[k] = 0.0f;
          }
        }
      }
    }
  }
}

}  // namespace smos

using namespace smos;

extern "C" int smos_bilinear_gather_fwd(const float* grid, const int64_t* grid_stride, const float* coord, int32_t K,
                                        float* out, const int64_t* out_stride, int64_t B, int64_t C, int64_t H,
                                        int64_t W, int64_t N, const float* scale, smos_stream_t stream) {
  SMOS_REQUIRE(B >= 0 && C >= 0 && N >= 0 && H > 0 && W > 0, "bilinear_gather: bad sizes");
  SMOS_REQUIRE(H < (1 << 24) && W < (1 << 24), "bilinear_gather: grid too large");
  SMOS_REQUIRE(K >= 2, "bilinear_gather: coord needs >= 2 columns, got %d", (int)K);
  if (B == 0 || C == 0 || N == 0) return SMOS_OK;
  SMOS_REQUIRE(grid && coord && out && grid_stride && out_stride && scale, "bilinear_gather: null pointer");
  BilGeom g;
  g.gs_b = grid_stride[0]; g.gs_c = grid_stride[1]; g.gs_h = grid_stride[2]; g.gs_w = grid_stride[3];
  g.os_b = out_stride[0]; g.os_c = out_stride[1]; g.os_n = out_stride[2];
  g.H = (int)H; g.W = (int)W; g.K = K; g.sy = scale[0]; g.sx = scale[1];
  hipStream_t s = (hipStream_t)stream;
  const int64_t pts = B * N;
  if (g.gs_c == 1 && g.os_c == 1 && C >= 8) {
    int G = 8;
    while (G < 64 && G < C) G <<= 1;
    dim3 gr(grid_for(pts * G, kBlock, 256 * 16));
    switch (G) {
      case 8: hipLaunchKernelGGL((bil_rows<8>), gr, dim3(kBlock), 0, s, grid, coord, out, g, B, C, N); break;
      case 16: hipLaunchKernelGGL((bil_rows<16>), gr, dim3(kBlock), 0, s, grid, coord, out, g, B, C, N); break;
      case 32: hipLaunchKernelGGL((bil_rows<32>), gr, dim3(kBlock), 0, s, grid, coord, out, g, B, C, N); break;
      default: hipLaunchKernelGGL((bil_rows<64>), gr, dim3(kBlock), 0, s, grid, coord, out, g, B, C, N); break;
    }
  } else {
    int chunks = 1;
    if (pts < (1 << 20) && C >= 16) {
      chunks = (int)(((int64_t)(1 << 20) + pts - 1) / pts);
      if (chunks > C / 8) chunks = (int)(C / 8);
      if (chunks < 1) chunks = 1;
    }
    const int c_chunk = (int)((C + chunks - 1) / chunks);
    chunks = (int)((C + c_chunk - 1) / c_chunk);
    hipLaunchKernelGGL(bil_points, dim3(grid_for(pts, kBlock, 256 * 16), chunks), dim3(kBlock), 0, s, grid, coord,
                       out, g, B, C, N, c_chunk);
  }
  return check_launch("bilinear_gather_fwd");
}

extern "C" int smos_bilinear_gather_bwd(const float* grad_out, const int64_t* grad_out_stride, const float* coord, int32_t K,
                                        float* grad_grid, const int64_t* grad_grid_stride, int64_t B, int64_t C, int64_t H,
                                        int64_t W, int64_t N, const float* scale, smos_stream_t stream) {
  SMOS_REQUIRE(B >= 0 && C >= 0 && N >= 0 && H > 0 && W > 0, "bilinear_gather_bwd: bad sizes");
  SMOS_REQUIRE(H < (1 << 24) && W < (1 << 24), "bilinear_gather_bwd: grid too large");
  SMOS_REQUIRE(K >= 2, "bilinear_gather_bwd: coord needs >= 2 columns, got %d", (int)K);
  if (B == 0 || C == 0) return SMOS_OK;
  SMOS_REQUIRE(grad_grid && grad_grid_stride, "bilinear_gather_bwd: null pointer");
  BilGeom g;
  g.gs_b = grad_grid_stride[0]; g.gs_c = grad_grid_stride[1]; g.gs_h = grad_grid_stride[2]; g.gs_w = grad_grid_stride[3];
  hipStream_t s = (hipStream_t)stream;

  // the destination arrives uninitialised
  const int64_t size[4] = {B, C, H, W};
  if (int rc = zero_destination(grad_grid, grad_grid_stride, size, s, "bilinear_gather_bwd zero")) return rc;
  if (N == 0) return SMOS_OK;
  SMOS_REQUIRE(grad_out && coord && grad_out_stride && scale, "bilinear_gather_bwd: null pointer");
  g.os_b = grad_out_stride[0]; g.os_c = grad_out_stride[1]; g.os_n = grad_out_stride[2];
  g.H = (int)H; g.W = (int)W; g.K = K; g.sy = scale[0]; g.sx = scale[1];
  if (g.gs_c == 1 && C >= 8) {
    const int64_t tiles = B * ((N + kBt - 1) / kBt);
    const dim3 gr(grid_for(tiles, kBlock / kWave, kMaxGrid));
    if (g.os_c == 1)
      hipLaunchKernelGGL((bil_bwd_rows<false>), gr, dim3(kBlock), 0, s, grad_out, coord, grad_grid, g, B, C, N);
    else
      hipLaunchKernelGGL((bil_bwd_rows<true>), gr, dim3(kBlock), 0, s, grad_out, coord, grad_grid, g, B, C, N);
  } else {
    hipLaunchKernelGGL(bil_bwd_points, dim3(grid_for(B * N, kBlock, 256 * 16)), dim3(kBlock), 0, s, grad_out, coord, grad_grid,
                       g, B, C, N);
  }
  return check_launch("bilinear_gather_bwd");
}
