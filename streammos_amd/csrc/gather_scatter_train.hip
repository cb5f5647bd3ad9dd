// Training form of a cross-view transfer for gfx950: grid -> point bilinear gather followed by the point -> grid max-pool
// scatter (CENet_Transformer._cross_view: BilinearSample, then VoxelMaxPool), forward and backward, without the [B,C,N]
// tensor between the two.
//
// Forward (gst_fwd): lane = point.  The position and taps come from make_taps (csrc/bilinear_taps.h), the target cell from
// cell_offset (csrc/voxel_cell.h); the value is blend4 below, which is bil_points' / bil_rows' sum to the bit; it goes into the
// zero-filled target by vmp_fwd_points' rule (v > 0: integer atomic max, v < 0: raise the flag, after which the launches
// gst_fwd<1> and <2> redo the reference algorithm).  The point values are stored only where the caller wants them.
//
// Backward: the point gradient x[b,c,n] is grad_out[cell] where the point is kept and its recomputed value equals out[cell]
// (ties all win, a 0 in a cell whose maximum is 0 wins: vmp_bwd_points' test on the same float32 number), else 0, plus
// grad_pts where the point values were handed on.  gst_bwd_rows then is bil_bwd_rows with x produced in the wave instead of
// loaded, and a run's row atomic left out where its sum is exactly 0 (the destination starts at 0); gst_bwd_points is
// bil_bwd_points in the same way; gst_point_grad writes x itself for the fixed-order sum of csrc/segsum.hip.
// Every load is unconditional: a lane without a point or a channel reads a clamped address and its value is dropped by a
// select.
#include "smos_common.h"
#include "bilinear_taps.h"
#include "voxel_cell.h"
#include "zero_fill.h"

namespace smos {

// The four-tap sum of the gather: acc = fma(g_k, w_k, acc) over the taps inside the map, in tap order, from +0 -- what the
// loops of bil_points and bil_rows compile to under -ffp-contract=on.  Written with the intrinsic, so that the forward and
// the backward of this file get the same number whatever the compiler would contract: the backward's v == out is exact.
__device__ __forceinline__ float blend4(const float (&gv)[4], const Taps& t) {
  float acc = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) acc = t.o[k] >= 0 ? __fmaf_rn(gv[k], t.w[k], acc) : acc;
  return acc;
}

// the value of one (point, channel): gc = the channel's plane of the point's sample
__device__ __forceinline__ float gather_value(const float* __restrict__ gc, const Taps& t) {
  float gv[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) gv[k] = gc[t.o[k] >= 0 ? t.o[k] : 0];
  return blend4(gv, t);
}

// Strides of the tensors that live on the target grid.  The cell itself travels as (y << 24) | x: VmpGeom::sstride is
// {1 << 24, 1} here (sizes are below 2^24), so one cell_offset serves tensors of different strides.
struct CellMaps {
  int64_t out_b, out_c, out_h, out_w;   // the forward's result
  int64_t go_b, go_c, go_h, go_w;       // its gradient
};
constexpr int kCellShift = 24;
__device__ __forceinline__ int64_t cell_at(int64_t cell, int64_t sh, int64_t sw) {
  return (cell >> kCellShift) * sh + (cell & ((1 << kCellShift) - 1)) * sw;
}

// The point tensors ([B,C,N]: the forward's values, grad_pts, x) use BilGeom::os_*.
struct PointGrad {
  const float* grid;
  const float* gcoord;
  const float* scoord;
  const float* out;
  const float* gout;
  const float* gpts;                    // null: the point values were not handed on
  int64_t gp_b, gp_c, gp_n;
  int32_t Ks;
};

// x of point (b, n), channel c.  `cell` < 0: the point is dropped.
__device__ __forceinline__ float point_grad(const PointGrad& a, const BilGeom& g, const CellMaps& m, const Taps& t, int64_t cell,
                                            int64_t b, int64_t n, int64_t c) {
  const int64_t cc = cell < 0 ? 0 : cell;
  const float v = gather_value(a.grid + b * g.gs_b + c * g.gs_c, t);
  const float o = a.out[b * m.out_b + c * m.out_c + cell_at(cc, m.out_h, m.out_w)];
  const float go = a.gout[b * m.go_b + c * m.go_c + cell_at(cc, m.go_h, m.go_w)];
  float x = (cell >= 0 && v == o) ? go : 0.0f;
  if (a.gpts) x = __fadd_rn(x, a.gpts[b * a.gp_b + c * a.gp_c + n * a.gp_n]);
  return x;
}

// ---------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------
// kPass 0: the fast pass (positive values by integer max, flag on a negative one); 1, 2: the exact passes behind the flag
// (vmp_fwd_signed: a racing member store, then signed max / unsigned min on the bit pattern).  BilGeom: gs_* = grid strides,
// os_* = strides of the point values; VmpGeom: the target's own strides.
template <int kPass>
__global__ __launch_bounds__(kBlock) void gst_fwd(const float* __restrict__ grid, const float* __restrict__ gcoord,
                                                  const float* __restrict__ scoord, float* __restrict__ out,
                                                  float* __restrict__ pts, int* flag, BilGeom g, VmpGeom v, int Ks, int64_t B,
                                                  int64_t C, int64_t N, int c_chunk) {
  if (kPass > 0 && *reinterpret_cast<const volatile int*>(flag) == 0) return;
  const int64_t total = B * N;
  const int64_t c0 = (int64_t)blockIdx.y * c_chunk;
  const int64_t c1 = min(c0 + c_chunk, C);
  int saw_neg = 0;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < total; base += (int64_t)gridDim.x * blockDim.x) {
    const bool has = base + threadIdx.x < total;
    const int64_t i = has ? base + threadIdx.x : total - 1;
    const int64_t b = i / N, n = i - b * N;
    const Taps t = make_taps(gcoord + i * g.K, g);
    const int64_t cell = cell_offset(scoord + i * Ks, v);
    const bool keep = has && cell >= 0;
    const float* __restrict__ gb = grid + b * g.gs_b;
    float* __restrict__ ob = out + b * v.out_b + (cell < 0 ? 0 : cell);
    for (int64_t c = c0; c < c1; ++c) {
      const float val = gather_value(gb + c * g.gs_c, t);
      float* p = ob + c * v.out_c;
      if (kPass == 0) {
        if (pts && has) pts[b * g.os_b + c * g.os_c + n * g.os_n] = val;
        if (keep && val > 0.0f)
          atomicMax(reinterpret_cast<int*>(p), __float_as_int(val));
        else if (keep && val < 0.0f)
          saw_neg = 1;
      } else if (kPass == 1) {
        if (keep) *p = val;
      } else if (keep && val == val) {
        if (val >= 0.0f)
          atomicMax(reinterpret_cast<int*>(p), __float_as_int(val));
        else
          atomicMin(reinterpret_cast<unsigned int*>(p), __float_as_uint(val));
      }
    }
  }
  if (kPass == 0 && saw_neg) *flag = 1;
}

// ---------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------
// x as a tensor: lane = point, loop over a chunk of channels.  BilGeom: gs_* = grid strides, os_* = strides of x.
__global__ __launch_bounds__(kBlock) void gst_point_grad(PointGrad a, float* __restrict__ x, BilGeom g, VmpGeom v, CellMaps m,
                                                         int64_t B, int64_t C, int64_t N, int c_chunk) {
  const int64_t total = B * N;
  const int64_t c0 = (int64_t)blockIdx.y * c_chunk;
  const int64_t c1 = min(c0 + c_chunk, C);
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < total; base += (int64_t)gridDim.x * blockDim.x) {
    const bool has = base + threadIdx.x < total;
    const int64_t i = has ? base + threadIdx.x : total - 1;
    const int64_t b = i / N, n = i - b * N;
    const Taps t = make_taps(a.gcoord + i * g.K, g);
    const int64_t cell = cell_offset(a.scoord + i * a.Ks, v);
    for (int64_t c = c0; c < c1; ++c) {
      const float xv = point_grad(a, g, m, t, cell, b, n, c);
      if (has) x[b * g.os_b + c * g.os_c + n * g.os_n] = xv;
    }
  }
}

// lane = point, loop over channels: 4-byte atomics at the destination's strides (C < 8, or a destination that is not
// channels-last), as bil_bwd_points.  BilGeom: gs_* = the strides of grid, which grad_grid has its own of (dg_*).
struct DstStrides {
  int64_t b, c, h, w;
};
__global__ __launch_bounds__(kBlock) void gst_bwd_points(PointGrad a, float* __restrict__ ggrid, DstStrides d, BilGeom g, VmpGeom v,
                                                         CellMaps m, int64_t B, int64_t C, int64_t N) {
  const int64_t total = B * N;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < total; base += (int64_t)gridDim.x * blockDim.x) {
    const bool has = base + threadIdx.x < total;
    const int64_t i = has ? base + threadIdx.x : total - 1;
    const int64_t b = i / N, n = i - b * N;
    const Taps t = make_taps(a.gcoord + i * g.K, g);
    const int64_t cell = cell_offset(a.scoord + i * a.Ks, v);
    float* __restrict__ db = ggrid + b * d.b;
    for (int64_t c = 0; c < C; ++c) {
      const float xv = point_grad(a, g, m, t, cell, b, n, c);
      float* dc = db + c * d.c;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float term = t.w[k] * xv;
        const int y = t.y0 + (k >> 1), x = t.x0 + (k & 1);
        if (has && t.o[k] >= 0 && term != 0.0f) atomicAdd(dc + (int64_t)y * d.h + (int64_t)x * d.w, term);
      }
    }
  }
}

// bil_bwd_rows (csrc/bilinear_gather.hip) with the tile's x values produced here: lane (p, hh) computes x of point p for the
// channels 2 j + hh of the chunk and writes them into the wave's LDS tile, which is then read out along c.  From there on
// the walk is bil_bwd_rows', except that a run's atomic is issued only where its sum is not 0.
__global__ __launch_bounds__(kBlock) void gst_bwd_rows(PointGrad a, float* __restrict__ ggrid, DstStrides d, BilGeom g, VmpGeom v,
                                                       CellMaps m, int64_t B, int64_t C, int64_t N) {
  __shared__ float lds[kBlock / kWave][kBt * kBPitch];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int p = lane & (kBt - 1), hh = lane >> 5;
  float* tile = lds[wave];
  const int64_t tiles_per = (N + kBt - 1) / kBt, n_tiles = B * tiles_per;
  constexpr int kWaves = kBlock / kWave;
  for (int64_t tl = (int64_t)blockIdx.x * kWaves + wave; tl < n_tiles; tl += (int64_t)gridDim.x * kWaves) {
    const int64_t b = tl / tiles_per, n0 = (tl - b * tiles_per) * kBt;
    const int n_valid = (int)min((int64_t)kBt, N - n0);
    const bool has = p < n_valid;
    const int64_t np = n0 + (has ? p : 0);
    const Taps t = make_taps(a.gcoord + (b * N + np) * g.K, g);
    const int64_t cell = cell_offset(a.scoord + (b * N + np) * a.Ks, v);
    // what the walk reads from other lanes: a lane without a point has no cell and no weight
    float w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = has ? t.w[k] : 0.0f;
    const int y0 = has ? t.y0 : -5, x0 = has ? t.x0 : -5;
    const bool any = has && (t.o[0] >= 0 || t.o[1] >= 0 || t.o[2] >= 0 || t.o[3] >= 0);
    if (__ballot(any) == 0) continue;      // padding tail of a scan: nothing to add
    // the shuffles are their own statements (inside a short-circuit expression they would run with lanes masked off)
    const int y_after = __shfl_down(y0, 1), x_after = __shfl_down(x0, 1);
    const uint32_t tails = (uint32_t)__ballot(hh == 0 && (p == kBt - 1 || y0 != y_after || x0 != x_after));
    for (int64_t c0 = 0; c0 < C; c0 += kWave) {
      const int cn = (int)min((int64_t)kWave, C - c0);
      const bool chan = lane < cn;
      const int jn = (cn + 1) >> 1;
#pragma unroll 4
      for (int j = 0; j < jn; ++j) {
        const int c = 2 * j + hh;
        const float xv = point_grad(a, g, m, t, cell, b, np, c0 + (c < cn ? c : 0));
        tile[p * kBPitch + c] = has ? xv : 0.0f;
      }
      bwd_wave_sync();
      // a lane >= cn reads columns this chunk never filled: whatever it sums is dropped by `chan` at the atomics
      float xs[kBt];
#pragma unroll
      for (int i = 0; i < kBt; ++i) xs[i] = tile[i * kBPitch + lane];
      bwd_wave_sync();
      float* __restrict__ dst = ggrid + b * d.b + c0 + lane;
      // A tap outside the map (weight zeroed) is outside for the whole run, since a run is one cell: if a non-finite
      // x turns 0 * x into NaN there, that acc[k] is never added anywhere and is reset with the run.
      float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int i = 0; i < kBt; ++i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = fmaf(lane_f(w[k], i), xs[i], acc[k]);
        if ((tails >> i) & 1) {
          const int yi = __builtin_amdgcn_readlane(y0, i), xi = __builtin_amdgcn_readlane(x0, i);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int y = yi + (k >> 1), x = xi + (k & 1);
            if (y >= 0 && y < g.H && x >= 0 && x < g.W && chan && acc[k] != 0.0f)
              atomicAdd(dst + (int64_t)y * d.h + (int64_t)x * d.w, acc[k]);
            acc[k] = 0.0f;
          }
        }
      }
    }
  }
}

// channel chunks over blockIdx.y, so that few points still fill the chip (as smos_bilinear_gather_fwd does for bil_points)
static int channel_chunks(int64_t pts, int64_t C, int* c_chunk) {
  int chunks = 1;
  if (pts < (1 << 20) && C >= 16) {
    chunks = (int)(((int64_t)(1 << 20) + pts - 1) / pts);
    if (chunks > C / 8) chunks = (int)(C / 8);
    if (chunks < 1) chunks = 1;
  }
  *c_chunk = (int)((C + chunks - 1) / chunks);
  return (int)((C + *c_chunk - 1) / *c_chunk);
}

struct Shapes {
  int64_t B, C, Hg, Wg, N, Ho, Wo;
};

static int check_shapes(const char* what, const Shapes& s, int32_t Kg, int32_t Ks) {
  SMOS_REQUIRE(s.B >= 0 && s.C >= 0 && s.N >= 0 && s.Hg > 0 && s.Wg > 0 && s.Ho > 0 && s.Wo > 0, "%s: bad sizes", what);
  SMOS_REQUIRE(s.Hg < (1 << 24) && s.Wg < (1 << 24) && s.Ho < (1 << 24) && s.Wo < (1 << 24), "%s: grid too large", what);
  SMOS_REQUIRE(Kg >= 2 && Ks >= 2, "%s: coordinates need >= 2 columns, got %d and %d", what, (int)Kg, (int)Ks);
  return SMOS_OK;
}

static BilGeom gather_geom(const int64_t* grid_stride, const int64_t* point_stride, const Shapes& s, int32_t Kg, const float* gscale) {
  BilGeom g;
  g.gs_b = grid_stride[0]; g.gs_c = grid_stride[1]; g.gs_h = grid_stride[2]; g.gs_w = grid_stride[3];
  g.os_b = point_stride ? point_stride[0] : 0; g.os_c = point_stride ? point_stride[1] : 0; g.os_n = point_stride ? point_stride[2] : 0;
  g.H = (int)s.Hg; g.W = (int)s.Wg; g.K = Kg; g.sy = gscale[0]; g.sx = gscale[1];
  return g;
}

// sh, sw: the spatial strides cell_offset multiplies the cell by
static VmpGeom scatter_geom(const Shapes& s, const float* sscale, int64_t sh, int64_t sw) {
  VmpGeom v;
  v.D = 2;
  for (int k = 0; k < 4; ++k) {
    v.size[k] = 1; v.sstride[k] = 0; v.scale[k] = 0.f;
  }
  v.size[0] = s.Ho; v.size[1] = s.Wo; v.sstride[0] = sh; v.sstride[1] = sw; v.scale[0] = sscale[0]; v.scale[1] = sscale[1];
  v.out_b = v.out_c = v.fs_b = v.fs_c = v.fs_n = 0;
  return v;
}

// the operands of both backward entries after their checks
struct BwdArgs {
  PointGrad a;
  BilGeom g;
  VmpGeom v;
  CellMaps m;
};
static int bwd_args(const char* what, BwdArgs& r, const float* grid, const int64_t* grid_stride, const float* gcoord, int32_t Kg,
                    const float* gscale, const float* scoord, int32_t Ks, const float* sscale, const float* out,
                    const int64_t* out_stride, const float* grad_out, const int64_t* grad_out_stride, const float* grad_pts,
                    const int64_t* grad_pts_stride, const int64_t* x_stride, const Shapes& s) {
  SMOS_REQUIRE(grid && grid_stride && gcoord && gscale && scoord && sscale && out && out_stride && grad_out && grad_out_stride,
               "%s: null pointer", what);
  SMOS_REQUIRE(!grad_pts || grad_pts_stride, "%s: grad_pts without strides", what);
  r.g = gather_geom(grid_stride, x_stride, s, Kg, gscale);
  r.v = scatter_geom(s, sscale, (int64_t)1 << kCellShift, 1);
  r.m.out_b = out_stride[0]; r.m.out_c = out_stride[1]; r.m.out_h = out_stride[2]; r.m.out_w = out_stride[3];
  r.m.go_b = grad_out_stride[0]; r.m.go_c = grad_out_stride[1]; r.m.go_h = grad_out_stride[2]; r.m.go_w = grad_out_stride[3];
  r.a.grid = grid; r.a.gcoord = gcoord; r.a.scoord = scoord; r.a.out = out; r.a.gout = grad_out; r.a.gpts = grad_pts;
  r.a.gp_b = grad_pts ? grad_pts_stride[0] : 0; r.a.gp_c = grad_pts ? grad_pts_stride[1] : 0; r.a.gp_n = grad_pts ? grad_pts_stride[2] : 0;
  r.a.Ks = Ks;
  return SMOS_OK;
}

}  // namespace smos

using namespace smos;

extern "C" int smos_gather_scatter_train_fwd(const float* grid, const int64_t* grid_stride, const float* gcoord, int32_t Kg,
                                             const float* gscale, const float* scoord, int32_t Ks, const float* sscale, float* out,
                                             const int64_t* out_stride, float* pts, const int64_t* pts_stride, int64_t B,
                                             int64_t C, int64_t Hg, int64_t Wg, int64_t N, int64_t Ho, int64_t Wo,
                                             int32_t* flag_ws, smos_stream_t stream) {
  const char* what = "gather_scatter_train_fwd";
  const Shapes sh = {B, C, Hg, Wg, N, Ho, Wo};
  if (int rc = check_shapes(what, sh, Kg, Ks)) return rc;
  if (B == 0 || C == 0 || N == 0) return SMOS_OK;
  SMOS_REQUIRE(grid && grid_stride && gcoord && gscale && scoord && sscale && out && out_stride && flag_ws, "%s: null pointer", what);
  SMOS_REQUIRE(!pts || pts_stride, "%s: pts without strides", what);
  const BilGeom g = gather_geom(grid_stride, pts ? pts_stride : nullptr, sh, Kg, gscale);
  VmpGeom v = scatter_geom(sh, sscale, out_stride[2], out_stride[3]);
  v.out_b = out_stride[0];
  v.out_c = out_stride[1];
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(flag_ws, 0, sizeof(int32_t), s) != hipSuccess) return check_launch("gather_scatter_train_fwd memset");
  int c_chunk;
  const int chunks = channel_chunks(B * N, C, &c_chunk);
  const dim3 gr((unsigned)conv_grid_cap(grid_for(B * N, kBlock, 256 * 16)), chunks);
  hipLaunchKernelGGL((gst_fwd<0>), gr, dim3(kBlock), 0, s, grid, gcoord, scoord, out, pts, (int*)flag_ws, g, v, (int)Ks, B, C, N, c_chunk);
  // the exact passes return at once while the flag is clear
  hipLaunchKernelGGL((gst_fwd<1>), gr, dim3(kBlock), 0, s, grid, gcoord, scoord, out, pts, (int*)flag_ws, g, v, (int)Ks, B, C, N, c_chunk);
  hipLaunchKernelGGL((gst_fwd<2>), gr, dim3(kBlock), 0, s, grid, gcoord, scoord, out, pts, (int*)flag_ws, g, v, (int)Ks, B, C, N, c_chunk);
  return check_launch(what);
}

extern "C" int smos_gather_scatter_train_bwd(const float* grid, const int64_t* grid_stride, const float* gcoord, int32_t Kg,
                                             const float* gscale, const float* scoord, int32_t Ks, const float* sscale,
                                             const float* out, const int64_t* out_stride, const float* grad_out,
                                             const int64_t* grad_out_stride, const float* grad_pts, const int64_t* grad_pts_stride,
                                             float* grad_grid, const int64_t* grad_grid_stride, int64_t B, int64_t C, int64_t Hg,
                                             int64_t Wg, int64_t N, int64_t Ho, int64_t Wo, smos_stream_t stream) {
  const char* what = "gather_scatter_train_bwd";
  const Shapes sh = {B, C, Hg, Wg, N, Ho, Wo};
  if (int rc = check_shapes(what, sh, Kg, Ks)) return rc;
  if (B == 0 || C == 0) return SMOS_OK;
  SMOS_REQUIRE(grad_grid && grad_grid_stride, "%s: null pointer", what);
  hipStream_t s = (hipStream_t)stream;
  const int64_t size[4] = {B, C, Hg, Wg};
  if (int rc = zero_destination(grad_grid, grad_grid_stride, size, s, "gather_scatter_train_bwd zero")) return rc;
  if (N == 0) return SMOS_OK;
  BwdArgs r;
  if (int rc = bwd_args(what, r, grid, grid_stride, gcoord, Kg, gscale, scoord, Ks, sscale, out, out_stride, grad_out,
                        grad_out_stride, grad_pts, grad_pts_stride, nullptr, sh))
    return rc;
  const DstStrides d = {grad_grid_stride[0], grad_grid_stride[1], grad_grid_stride[2], grad_grid_stride[3]};
  if (d.c == 1 && C >= 8) {
    const int64_t tiles = B * ((N + kBt - 1) / kBt);
    const dim3 gr((unsigned)conv_grid_cap(grid_for(tiles, kBlock / kWave, kMaxGrid)));
    hipLaunchKernelGGL(gst_bwd_rows, gr, dim3(kBlock), 0, s, r.a, grad_grid, d, r.g, r.v, r.m, B, C, N);
  } else {
    const dim3 gr((unsigned)conv_grid_cap(grid_for(B * N, kBlock, 256 * 16)));
    hipLaunchKernelGGL(gst_bwd_points, gr, dim3(kBlock), 0, s, r.a, grad_grid, d, r.g, r.v, r.m, B, C, N);
  }
  return check_launch(what);
}

extern "C" int smos_gather_scatter_train_point_grad(const float* grid, const int64_t* grid_stride, const float* gcoord, int32_t Kg,
                                                    const float* gscale, const float* scoord, int32_t Ks, const float* sscale,
                                                    const float* out, const int64_t* out_stride, const float* grad_out,
                                                    const int64_t* grad_out_stride, const float* grad_pts,
                                                    const int64_t* grad_pts_stride, float* x, const int64_t* x_stride, int64_t B,
                                                    int64_t C, int64_t Hg, int64_t Wg, int64_t N, int64_t Ho, int64_t Wo,
                                                    smos_stream_t stream) {
  const char* what = "gather_scatter_train_point_grad";
  const Shapes sh = {B, C, Hg, Wg, N, Ho, Wo};
  if (int rc = check_shapes(what, sh, Kg, Ks)) return rc;
  if (B == 0 || C == 0 || N == 0) return SMOS_OK;
  SMOS_REQUIRE(x && x_stride, "%s: null pointer", what);
  BwdArgs r;
  if (int rc = bwd_args(what, r, grid, grid_stride, gcoord, Kg, gscale, scoord, Ks, sscale, out, out_stride, grad_out,
                        grad_out_stride, grad_pts, grad_pts_stride, x_stride, sh))
    return rc;
  int c_chunk;
  const int chunks = channel_chunks(B * N, C, &c_chunk);
  const dim3 gr((unsigned)conv_grid_cap(grid_for(B * N, kBlock, 256 * 16)), chunks);
  hipLaunchKernelGGL(gst_point_grad, gr, dim3(kBlock), 0, (hipStream_t)stream, r.a, x, r.g, r.v, r.m, B, C, N, c_chunk);
  return check_launch(what);
}
