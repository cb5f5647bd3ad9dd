// Fused point-side kernel of the inference engine (gfx950).
//
//   pointnet_scatter : per-point MLP 7 -> 64 -> 64 (BatchNorm folded, ReLU) on the matrix cores (exact-f32 MFMA, both
//                      layers chained in registers) and max-scattered straight into the channels-last BEV grid
//                      -- the (BS*T, 64, N) feature tensor of the reference (491 MB written by point_pre and
//                      read back by VoxelMaxPool, models/StreamMOS.py:101-102) never exists.
//
// The cross-view gather + scatter kernels of the engine are channels-last and live in csrc/cl_kernels.hip.
//
// The result tile is computed with lane = point, staged in LDS and leaves with lane = channel, so every store / atomic
// is one contiguous row -- the shape at which MI355X's memory-side atomics run at full rate -- instead of 64
// scattered 4-byte atomics.  Values <= 0 are skipped against the zero-filled grid exactly as in
// voxel_maxpool.hip (the features are post-ReLU).
#include "smos_common.h"

namespace smos {

__device__ __forceinline__ int cell_2d(const float* __restrict__ row, float sy, float sx, int H, int W) {
  // same rule as voxel_maxpool.hip::cell_offset (reference: point_deep_cuda_kernel.cu:39-47)
  const float py = __fmul_rn(row[0], sy), px = __fmul_rn(row[1], sx);
  const bool ok = (py > -1.0f) && (py < (float)H) && (px > -1.0f) && (px < (float)W);
  return ok ? (int)py * W + (int)px : -1;
}

// ---------------------------------------------------------------------------------------------
// PointNet(7 -> 64 -> 64) + scatter
// ---------------------------------------------------------------------------------------------
struct PnsArgs {
  const float* xyzi;   // [S, 7, N]
  const float* coord;  // [S, N, K]
  const float* w1;     // [64, 7]  (BN folded)
  const float* b1;     // [64]
  const float* w2;     // [64, 64]
  const float* b2;     // [64]
  float* bev;          // [B, H, W, T*64] zero-filled; or, with row_of, compact rows [n_rows, T*64]
  const int32_t* row_of;  // null, or [B, H, W] row of every occupied cell (csrc/stem.hip): scatter into compact rows
  float* pts_out;      // [B, N, *] rows of the t == 0 sample (row pitch po_n), or null
  const int32_t* n_live;  // device, or null: points [*n_live, N) of the t == 0 scans are the padding tail: their rows are not wanted
  int64_t bev_sb, po_b, po_n;
  int S, T, N, K, H, W, tiles_per_sample;
};

// Matrix-core formulation.  Both layers are computed TRANSPOSED, C = W * X with the output channel on the MFMA row
// and the point on the MFMA column (v_mfma_f32_32x32x2_f32: exact f32, the fp32 vector rate):
//   * the weights are the A operand: one VGPR per (32-channel block, k-step), 8 + 64 registers loaded ONCE per wave and
//     kept for the whole persistent loop -- no per-tile weight traffic at all (the scalar-load version re-streams 18 KB
//     per tile through a 16 KB scalar cache that it thrashes; measured: 0.40 ms, 0.26 ms with half the weights);
//   * the points are the B operand: lane l holds feature 2s + (l >> 5) of point (l & 31), read straight from the
//     channel-major input; feature 7 is the constant 1 that carries the folded layer-1 bias;
//   * a 32x32 result tile has its point on the lane and its channels in the 16 accumulator registers, which IS the B
//     operand layout of the next layer: register r of lane half h is channel 8(r>>2) + 4h + (r&3), so layer 2 walks the
//     hidden channels in that order (its A operand is loaded with the same permutation) and takes relu(C1) with no lane
//     movement and no LDS.
// The 32-point x 64-channel output tile goes through LDS once (point-major rows, pitch 68) and leaves with lane =
// channel: every store / atomic is one contiguous 256-byte row.
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kNt = 32;        // points per MFMA column tile
constexpr int kPitchM = 68;    // floats per LDS row (64 channels + 4: conflict-free 128-bit row writes)

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(kBlock) void pointnet_scatter(PnsArgs a) {
  __shared__ float lds_tile[kBlock / kWave][kNt * kPitchM];
  __shared__ float lds_b2[64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int col = lane & 31, hh = lane >> 5;
  float w1a[2][4], w2a[2][32];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = 2 * s + hh;
      w1a[mt][s] = k < 7 ? a.w1[(mt * 32 + col) * 7 + k] : a.b1[mt * 32 + col];
    }
#pragma unroll
    for (int s = 0; s < 32; ++s) {
      const int r = s & 15;
      const int k = (s >> 4) * 32 + 8 * (r >> 2) + 4 * hh + (r & 3);
      w2a[mt][s] = a.w2[(mt * 32 + col) * 64 + k];
    }
  }
  if (threadIdx.x < 64) lds_b2[threadIdx.x] = a.b2[threadIdx.x];
  __syncthreads();

  // tile bookkeeping is wave-uniform 32-bit arithmetic (the host checks that the tile count fits): it stays on the
  // scalar unit, which matters because VALU instructions issue through the same port as the MFMAs
  const int nt_per_sample = (a.N + kNt - 1) / kNt;
  const int n_nt = a.S * nt_per_sample;
  float* tile = lds_tile[wave];
  const int nt_step = (int)gridDim.x * (kBlock / kWave);
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);

  // inputs of one column tile: 4 features per lane + the two grid coordinates of the lane's point
  struct TileIn {
    float x[4], cy, cx;      // as loaded: the selects that turn them into operands are applied where they are consumed --
    bool has;                // applied here, hipcc hoists them right behind the loads and the prefetch is waited for at once
  };
  // Every load of the software pipeline is an UNCONDITIONAL raw buffer load: a lane without a point uses an offset past
  // the end of the buffer and reads 0.  Written as "has ? ptr[i] : 0" the loads sit under lane-dependent branches, hipcc's
  // wait-count pass loses track of them and puts s_waitcnt vmcnt(0) in front of the next vector-memory-dependent
  // instruction -- here right behind the prefetch, so every tile sat through a full memory latency before its matrix
  // phase (ISA: vmcnt(0) 30 instructions after the loads; MFMA busy 36 %).
  const __amdgpu_buffer_rsrc_t xsrd = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.xyzi), 0, a.S * 7 * a.N * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t csrd = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.coord), 0, a.S * a.N * a.K * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrd = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<int32_t*>(a.row_of), 0, a.row_of ? (a.S / a.T) * a.H * a.W * 4 : 0, 0x00020000);
  constexpr unsigned kOob = 0x80000000u;
  auto fetch = [&](int nt, TileIn& in) {
    // tile nt = column tile nt / S of sample nt % S (sample fastest): a wave's tiles nt, nt + step, .. then spread evenly over
    // the point range of every sample, so every wave meets the same share of the scans' padding tails (sample-major order
    // left a wave 15 to 20 live tiles of its 29)
    const bool live = nt < n_nt;
    const int s = live ? nt % a.S : 0;
    const int n0 = live ? (nt / a.S) * kNt : 0;
    const bool has = live & (n0 + col < a.N);
    const unsigned xoff = (unsigned)((s * 7 + hh) * a.N + n0 + col) * 4u;      // feature f = 2 q + hh of the lane's point
    const unsigned fstep = (unsigned)a.N * 8u;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool ok = has & (2 * q + hh < 7);
      in.x[q] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xsrd, ok ? xoff + fstep * q : kOob, 0, 0));
    }
    const unsigned coff = has ? (unsigned)((s * a.N + n0 + col) * a.K) * 4u : kOob;
    in.cy = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(csrd, coff, 0, 0));
    in.cx = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(csrd, coff + 4u, 0, 0));      // (the last argument is the cache policy)
    in.has = has;
  };

  // target slot of the lane's point: its cell of the dense grid, or (compact target) the row of that cell -- looked up
  // here, per lane and inside the prefetch shadow, not in the serial flush loop.  Equal cells <=> equal rows, so the
  // run detection works on either.
  // split in two: the request (cell from the coordinates + the row lookup issued) and the resolve (first use of the
  // looked-up row), so that a whole matrix phase lies between them
  auto cell_request = [&](const TileIn& in, int tile, int& c, int& r) {
    const float yx[2] = {in.has ? in.cy : -1.0f, in.has ? in.cx : -1.0f};   // -1 is outside the half-open test of cell_2d
    c = cell_2d(yx, 1.0f, 1.0f, a.H, a.W);
    const unsigned roff = (c >= 0) ? (unsigned)(((tile % a.S) / a.T) * a.H * a.W + c) * 4u : kOob;
    r = (int)__builtin_amdgcn_raw_buffer_load_b32(rsrd, roff, 0, 0);      // no row table: zero-sized buffer, reads 0
  };
  auto cell_resolve = [&](int c, int r) { return ((a.row_of != nullptr) & (c >= 0)) ? r : c; };
  const int n_live = a.n_live ? min(max(*a.n_live, 0), a.N) : a.N;
  int nt = (int)blockIdx.x * (kBlock / kWave) + wave_u;
  TileIn cur, nxt;
  fetch(nt, cur);
  fetch(nt + nt_step, nxt);
  int cell;
  {
    int c0, r0;
    cell_request(cur, nt, c0, r0);
    cell = cell_resolve(c0, r0);
    // everything the loop carries has landed before the first trip: otherwise the loop header inherits pending loads from
    // this path, and the wait the compiler puts there is, on the back edge, a wait for the previous tile's atomics
    asm volatile("" : "+v"(cur.x[0]), "+v"(cur.x[1]), "+v"(cur.x[2]), "+v"(cur.x[3]), "+v"(nxt.x[0]), "+v"(nxt.x[1]), "+v"(nxt.x[2]),
                 "+v"(nxt.x[3]), "+v"(nxt.cy), "+v"(nxt.cx), "+v"(cell));
  }
  for (; nt < n_nt; nt += nt_step) {
    // Software pipeline, two tiles deep: the inputs of tile + 2 and the row lookup of tile + 1 (whose coordinates arrived
    // during the previous matrix phase) are requested here and waited for after this tile's matrix phase, BEFORE this
    // tile's stores and atomics are issued.  The vector-memory counter of gfx9 retires in order and the number of atomics
    // is data dependent, so a wait placed after them is a wait for all of them (vmcnt(0)) -- with a one-deep pipeline the
    // looked-up row of the next tile was exactly such a wait at the loop's back edge.
    TileIn nn;
    fetch(nt + 2 * nt_step, nn);
    int c_next, r_next;
    cell_request(nxt, nt + nt_step, c_next, r_next);
    const int s = nt % a.S;
    const int n0 = (nt / a.S) * kNt;
    const int b = s / a.T, t = s - b * a.T;
    float xk[4] = {cur.x[0], cur.x[1], cur.x[2], hh ? 1.0f : cur.x[3]};      // feature 7 = 1 carries the folded layer-1 bias
    // the shuffle is its own statement: inside the short-circuit expression it would run with lane 31 masked off, and
    // a lane that reads a masked-off lane gets 0 -- indistinguishable from cell 0
    const int cell_after = __shfl_down(cell, 1);
    const uint32_t tails = (uint32_t)__ballot(hh == 0 && (col == kNt - 1 || cell != cell_after));
    // a tile none of whose points falls into the grid (the padding tail of a scan: 25-40 % of the rows) produces nothing
    // unless its point rows are wanted (t == 0): skip the matrix work, keep the software pipeline moving
    if (!(a.pts_out && t == 0 && n0 < n_live) && __ballot(cell >= 0) == 0) {
      // (waited for on this path too: the register copies of the rotation sit in the shared loop latch, and a wait placed
      // there would run on the main path as well -- as a wait for its atomics)
      asm volatile("" : "+v"(nn.x[0]), "+v"(nn.x[1]), "+v"(nn.x[2]), "+v"(nn.x[3]), "+v"(nn.cy), "+v"(nn.cx), "+v"(r_next));
      cell = cell_resolve(c_next, r_next);
      cur = nxt;
      nxt = nn;
      continue;
    }

    f32x16 c1[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) c1[mt][r] = 0.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) c1[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1a[mt][q], xk[q], c1[mt], 0, 0, 0);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) c1[mt][r] = fmaxf(c1[mt][r], 0.0f);

    f32x16 c2[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 bias = *reinterpret_cast<const float4*>(&lds_b2[mt * 32 + 8 * g + 4 * hh]);
        c2[mt][4 * g + 0] = bias.x; c2[mt][4 * g + 1] = bias.y; c2[mt][4 * g + 2] = bias.z; c2[mt][4 * g + 3] = bias.w;
      }
#pragma unroll
    for (int q = 0; q < 32; ++q)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
        c2[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(w2a[mt][q], c1[q >> 4][q & 15], c2[mt], 0, 0, 0);

    float* row = tile + col * kPitchM + 4 * hh;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<float4*>(row + mt * 32 + 8 * g) =
            make_float4(fmaxf(c2[mt][4 * g], 0.0f), fmaxf(c2[mt][4 * g + 1], 0.0f), fmaxf(c2[mt][4 * g + 2], 0.0f),
                        fmaxf(c2[mt][4 * g + 3], 0.0f));
    wave_sync();

    // lane = channel: 32 points, each one 256-byte row.  All 32 LDS reads are issued before the first use, the point
    // rows leave first, then same-cell runs are reduced in registers and flushed with one row atomic per run; the run
    // ends are a wave-uniform bit mask, so the control flow is scalar.
    const int n_valid = min(kNt, a.N - n0);
    const unsigned ulane = lane;   // zero-extended lane offset: lets the stores use the scalar-base addressing form
    float v[kNt];
#pragma unroll
    for (int i = 0; i < kNt; ++i) v[i] = tile[i * kPitchM + lane];
    // the prefetch is waited for here (tied to the last LDS read so that the scheduler cannot hoist the wait)
    asm volatile("" : "+v"(nn.x[0]), "+v"(nn.x[1]), "+v"(nn.x[2]), "+v"(nn.x[3]), "+v"(nn.cy), "+v"(nn.cx), "+v"(r_next), "+v"(v[kNt - 1]));
    const int cell_next = cell_resolve(c_next, r_next);
    if (a.pts_out && t == 0) {
      float* prow = a.pts_out + (int64_t)b * a.po_b + (int64_t)n0 * a.po_n;   // wave-uniform
      if (n_valid == kNt) {
#pragma unroll
        for (int i = 0; i < kNt; ++i) (prow + (int64_t)i * a.po_n)[ulane] = v[i];
      } else {
#pragma unroll
        for (int i = 0; i < kNt; ++i)
          if (i < n_valid) (prow + (int64_t)i * a.po_n)[ulane] = v[i];
      }
    }
    // wave-uniform target of this (sample, scan): the sample's slab of the dense grid, or the compact row table
    float* gsample = a.bev + (a.row_of ? (int64_t)0 : (int64_t)b * a.bev_sb) + t * 64;
    const int64_t cell_pitch = (int64_t)a.T * 64;
    float best = 0.0f;
#pragma unroll
    for (int i = 0; i < kNt; ++i) {
      best = fmaxf(best, v[i]);
      if ((tails >> i) & 1) {
        const int ci = __builtin_amdgcn_readlane(cell, i);
        if (ci >= 0 && best > 0.0f)
          atomicMax(reinterpret_cast<int*>(gsample + (int64_t)ci * cell_pitch) + ulane, __float_as_int(best));
        best = 0.0f;
      }
    }
    wave_sync();
    cur = nxt;
    nxt = nn;
    cell = cell_next;
  }
}

}  // namespace smos

using namespace smos;

static int pointnet_scatter_launch(const float* xyzi, const float* coord, int32_t K, const float* w1, const float* b1,
                                   const float* w2, const float* b2, float* bev, const int32_t* row_of, float* pts_out,
                                   const int32_t* n_live, int64_t po_b, int64_t po_n, int64_t B, int64_t T, int64_t N, int64_t H, int64_t W, int32_t cin,
                                   int32_t cmid, int32_t cout, smos_stream_t stream) {
  if (cin != 7 || cmid != 64 || cout != 64) {
    set_error("pointnet_scatter: built for the 7 -> 64 -> 64 point MLP (got %d -> %d -> %d)", (int)cin, (int)cmid, (int)cout);
    return SMOS_ERR_UNSUPPORTED;
  }
  SMOS_REQUIRE(B > 0 && T > 0 && N > 0 && H > 0 && W > 0 && K >= 2, "pointnet_scatter: bad sizes");
  SMOS_REQUIRE(xyzi && coord && w1 && b1 && w2 && b2 && bev, "pointnet_scatter: null pointer");
  SMOS_REQUIRE(H * W < (1LL << 31) && (!pts_out || po_n >= 64), "pointnet_scatter: bad geometry");
  SMOS_REQUIRE(B * T * 7 * N * 4 < (1LL << 31) && B * T * N * K * 4 < (1LL << 31) && B * H * W * 4 < (1LL << 31),
               "pointnet_scatter: an input larger than 2 GiB (32-bit buffer offsets)");
  PnsArgs a;
  a.xyzi = xyzi; a.coord = coord; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.bev = bev; a.row_of = row_of; a.pts_out = pts_out;
  a.n_live = n_live;
  a.bev_sb = H * W * T * 64; a.po_b = po_b; a.po_n = po_n;
  a.S = (int)(B * T); a.T = (int)T; a.N = (int)N; a.K = K; a.H = (int)H; a.W = (int)W;
  a.tiles_per_sample = (int)((N + kNt - 1) / kNt);
  // persistent waves: exactly as many blocks as are resident at once
  KernelSetup ks;
  if (int rc = kernel_setup(reinterpret_cast<const void*>(&pointnet_scatter), 0, kBlock, &ks, "pointnet_scatter")) return rc;
  const int64_t resident = conv_grid_cap((int64_t)ks.per_cu * ks.cus);      // (the test hook's cap: several trips per wave)
  const int64_t n_nt = (int64_t)a.S * ((N + kNt - 1) / kNt);
  SMOS_REQUIRE(n_nt < (1LL << 30), "pointnet_scatter: too many points for 32-bit tile indices");
  const int64_t want = (n_nt + 3) / 4;
  hipLaunchKernelGGL(pointnet_scatter, dim3((unsigned)(want < resident ? want : resident)), dim3(kBlock), 0,
                     (hipStream_t)stream, a);
  return check_launch("pointnet_scatter");
}

extern "C" int smos_pointnet_scatter(const float* xyzi, const float* coord, int32_t K, const float* w1, const float* b1,
                                     const float* w2, const float* b2, float* bev, float* pts_out, int64_t po_b,
                                     int64_t po_n, int64_t B, int64_t T, int64_t N, int64_t H, int64_t W, int32_t cin,
                                     int32_t cmid, int32_t cout, smos_stream_t stream) {
  return pointnet_scatter_launch(xyzi, coord, K, w1, b1, w2, b2, bev, nullptr, pts_out, nullptr, po_b, po_n, B, T, N, H, W, cin, cmid,
                                 cout, stream);
}

// n_live (device int32, may be null): the first *n_live points of the current (t == 0) scan of every sample are real; the point
// rows of its padding tail are not written (nothing reads them once the point head knows the same count).
extern "C" int smos_pointnet_scatter_rows(const float* xyzi, const float* coord, int32_t K, const float* w1, const float* b1,
                                          const float* w2, const float* b2, float* rows, const int32_t* row_of, float* pts_out,
                                          int64_t po_b, int64_t po_n, int64_t B, int64_t T, int64_t N, int64_t H, int64_t W,
                                          int32_t cin, int32_t cmid, int32_t cout, const int32_t* n_live, smos_stream_t stream) {
  SMOS_REQUIRE(row_of, "pointnet_scatter_rows: null row table");
  return pointnet_scatter_launch(xyzi, coord, K, w1, b1, w2, b2, rows, row_of, pts_out, n_live, po_b, po_n, B, T, N, H, W, cin, cmid,
                                 cout, stream);
}
