// Fused point head for gfx950: CatFusion + PredBranch (networks/backbone.py:387-413, 188-196; models/StreamMOS.py:107-113)
//     rows [P, 192] -> 1x1 192->96 + ReLU -> 1x1 96->64 + ReLU -> 1x1 64->M3 (+bias)        (BatchNorm folded)
// as ONE kernel on the matrix cores.  The three layers are chained in the transposed form of pointnet_scatter
// (point_fused.hip): C = W * X with the output channel on the MFMA row and the point on the column, so that a layer's
// 32x32 result tiles (point on the lane, channels in the accumulator registers) ARE the B operands of the next layer --
// the 96- and 64-channel intermediates (245 + 164 MB at the validation shape) never leave the registers.
//   A operands (weights): all three layers resident in LDS (72 + 24 + 8 KB) in MFMA operand order, prepared on the host;
//   layer 1 B operand: the row is [pn 64 | bev 64 | rv 64]; lane (p, h) holds channels 32h .. 32h+31 of each of the three,
//   streamed from its row in three K-thirds of 8 float4 -- the same walk for both lane halves, one source per third;
//   layer 2 / 3 walk their input channels in accumulator order: register r of tile mt, lane half h = channel
//   32 mt + 8 (r >> 2) + 4 h + (r & 3).
// Output: logits [B, M3, N] (the reference's (B, 3, N, 1) layout), 32 contiguous floats per channel and tile.
// point_head<true> (smos_point_head_gather) builds the middle third itself: the decoder's grid -> point bilinear gather
// (gather_scatter_cl4 without a scatter target) with the position arithmetic and the tap sum of smos_common.h, so the logits
// equal those of the gather launch followed by point_head<false> bit for bit, and nobody writes or reads the BEV third of the
// rows.  The 32 tap loads of a lane are requested behind the first third's row loads and summed behind its MFMAs.
#include "smos_common.h"

namespace smos {

typedef float f32x16 __attribute__((ext_vector_type(16)));
// Diagnostic builds only (tools/ablate_head.sh): -DSMOS_HEAD_ABLATE=<bits> removes 1 the row and tap loads, 2 the layer-1 MFMAs, 4 layers
// 2 / 3, 8 the logit stores to time what is left; results are wrong.  The shipped library is built without it.
#ifdef SMOS_HEAD_ABLATE
#define HEAD_AB(bit) ((SMOS_HEAD_ABLATE) & (bit))
#else
#define HEAD_AB(bit) 0
#endif
constexpr int kHeadBlock = 512;
constexpr int kK1 = 192, kM1 = 96, kM2 = 64;
constexpr int kS1 = kK1 / 2, kS2 = kM1 / 2, kS3 = kM2 / 2;           // k-steps (two k per MFMA)
constexpr int kA1 = (kM1 / 32) * kS1 * 64, kA2 = (kM2 / 32) * kS2 * 64, kA3 = kS3 * 64;   // floats
constexpr int kHeadLds = kA1 + kA2 + kA3 + kM1 + kM2 + 32;            // + biases

struct HeadArgs {
  const float* rows;     // [P, *] row pitch rp
  const float* wprep;    // kHeadLds floats: A1 | A2 | A3 | b1 | b2 | b3 (padded to 32)
  float* out;            // [B, M3, N]
  const int32_t* n_live; // device: points [*n_live, N) of every sample are the padding tail of the scan (null: none)
  int64_t rp;
  int B, N, M3;
  // point_head<true> only: the channels-last map the middle third is gathered from, as smos_gather_scatter_cl takes it
  const float* grid;     // [B, Hg, Wg, *] pixel pitch gp floats (channel offset applied), 64 channels read
  const float* gcoord;   // sample b, point n at gcoord + b * gbs + n * Kg
  int64_t gp, gbs;
  int Kg, Hg, Wg, grid_bytes;
  float gsy, gsx;
};

constexpr int kThirds = 3, kTSteps = kS1 / kThirds, kTVec = kTSteps / 4;   // 32 k-steps = 8 float4 per lane and third

// K-steps [kS0, kS1e) of one K-third of layer 1 on the lane's 8 float4 of that third.
template <int kS0 = 0, int kS1e = kTSteps>
__device__ __forceinline__ void head_l1_third(const float* A1, int third, int lane, const float4 (&x4)[kTVec], f32x16 (&c1)[kM1 / 32]) {
  int off = third * kTSteps * 64 + lane;
#pragma unroll
  for (int s = kS0; s < kS1e; ++s) {
    // as in layers 2 / 3: the LDS offset re-materialised every 8 steps keeps the weight reads of a third from being hoisted
    if (s % 8 == 0) asm volatile("" : "+v"(off), "+v"(c1[0]), "+v"(c1[1]), "+v"(c1[2]));
    const float4 v = x4[s >> 2];
    const float x = (s & 3) == 0 ? v.x : (s & 3) == 1 ? v.y : (s & 3) == 2 ? v.z : v.w;
#pragma unroll
    for (int mt = 0; mt < kM1 / 32; ++mt) {
      if (HEAD_AB(2)) c1[mt][s & 15] += A1[(mt * kS1 + s) * 64 + off] * x;
      else c1[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(A1[(mt * kS1 + s) * 64 + off], x, c1[mt], 0, 0, 0);
    }
  }
}

__device__ __forceinline__ float4 head_as_float4(__attribute__((ext_vector_type(4))) unsigned v) {
  return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}

template <bool kGather>
__global__ __launch_bounds__(kHeadBlock) void point_head(HeadArgs a) {
  extern __shared__ float lds[];
  for (int i = threadIdx.x; i < kHeadLds; i += kHeadBlock) lds[i] = a.wprep[i];
  __syncthreads();
  const float* A1 = lds;
  const float* A2 = lds + kA1;
  const float* A3 = A2 + kA2;
  const float* B1 = A3 + kA3;
  const float* B2 = B1 + kM1;
  const float* B3 = B2 + kM2;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int col = lane & 31, hh = lane >> 5;
  constexpr int kWaves = kHeadBlock / 64;
  const int n_live = a.n_live ? min(max(*a.n_live, 0), a.N) : a.N;
  // The padding tail (datasets/data_StreamMOS.py:568-571 pads every scan to frame_point_num with points at -1000 that
  // val_StreamMOS.py:113 cuts off again): its logits are never read; they are written as zeros, by all threads alike.  The
  // waves then share the LIVE tiles only -- dealing out all tiles round-robin left a wave 5 to 7 live ones of its ~10.
  const int live_tiles = (n_live + 31) / 32, tail0 = live_tiles * 32;
  if (tail0 < a.N) {
    const int64_t per = (int64_t)a.M3 * (a.N - tail0), total = (int64_t)a.B * per;
    for (int64_t i = (int64_t)blockIdx.x * kHeadBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kHeadBlock) {
      const int b = (int)(i / per);
      const int64_t r = i - (int64_t)b * per;
      const int ch = (int)(r / (a.N - tail0));
      a.out[((int64_t)b * a.M3 + ch) * a.N + tail0 + (r - (int64_t)ch * (a.N - tail0))] = 0.0f;
    }
  }
  // every tap load goes through this descriptor: an absent tap uses an offset past its end and reads 0 (no load under a branch)
  const __amdgpu_buffer_rsrc_t gsrd =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.grid), 0, kGather ? a.grid_bytes : 0, 0x00020000);
  const int n_tiles = a.B * live_tiles, tile_step = gridDim.x * kWaves;
  // a lane's coordinate pair is requested one tile ahead, so that the tap loads of a tile do not wait for it
  auto coord_of = [&](int lt) {
    const int b = lt / live_tiles, n = (lt - b * live_tiles) * 32 + col;
    return a.gcoord + (int64_t)b * a.gbs + (int64_t)(n < a.N ? n : 0) * a.Kg;
  };
  float cy = 0.f, cx = 0.f;
  if (kGather && blockIdx.x * kWaves + wave < n_tiles) {
    const float* cr = coord_of(blockIdx.x * kWaves + wave);
    cy = cr[0]; cx = cr[1];
  }
  for (int lt = blockIdx.x * kWaves + wave; lt < n_tiles; lt += tile_step) {
    const int b = lt / live_tiles;
    const int n = (lt - b * live_tiles) * 32 + col;
    const bool valid = n < a.N;
    // third t of the lane's K walk = floats [64 t + 32 hh, + 32) of the row
    const float4* src = reinterpret_cast<const float4*>(a.rows + ((int64_t)b * a.N + (valid ? n : 0)) * a.rp + hh * kTSteps);

    // ---- layer 1: 192 -> 96, K streamed in three thirds
    float4 cur[kTVec], nxt[kTVec];
#pragma unroll
    for (int j = 0; j < kTVec; ++j) cur[j] = HEAD_AB(1) ? make_float4((float)lane, 1.f, 2.f, (float)j) : src[j];
    // the lane's 32 BEV channels are gathered in two halves of 4 float4 x 4 taps (all eight at once do not fit the registers)
    float4 tap[kTVec / 2][4];
    int toff[4];
    float twt[4];
    unsigned tbyte[4];
    auto request_taps = [&](int half) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < kTVec / 2; ++j)
          tap[j][k] = HEAD_AB(1) ? make_float4((float)lane, 1.f, (float)k, (float)j)
                                 : head_as_float4(__builtin_amdgcn_raw_buffer_load_b128(gsrd, tbyte[k] + 16u * (half * (kTVec / 2) + j), 0, 0));
    };
    if (kGather) {
      bilinear_taps_cl(cy, cx, a.gsy, a.gsx, a.Hg, a.Wg, toff, twt);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        tbyte[k] = toff[k] >= 0 ? (unsigned)((((int64_t)b * a.Hg * a.Wg + toff[k]) * a.gp + hh * kTSteps) * 4) : 0x80000000u;
      request_taps(0);
      const float* cr = coord_of(lt + tile_step < n_tiles ? lt + tile_step : lt);
      cy = cr[0]; cx = cr[1];
    }
    f32x16 c1[kM1 / 32];
#pragma unroll
    for (int mt = 0; mt < kM1 / 32; ++mt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 bias = *reinterpret_cast<const float4*>(B1 + mt * 32 + 8 * g + 4 * hh);
        c1[mt][4 * g] = bias.x; c1[mt][4 * g + 1] = bias.y; c1[mt][4 * g + 2] = bias.z; c1[mt][4 * g + 3] = bias.w;
      }
    if (kGather) {
      // (the scheduling barriers keep hipcc from moving a half's sums, and with them the wait for its taps, in front of the
      // MFMAs that are there to cover them)
      head_l1_third<0, kTSteps / 2>(A1, 0, lane, cur, c1);        // covers the first half of the taps
      __builtin_amdgcn_sched_barrier(0);
      float4 bev[kTVec];
#pragma unroll
      for (int j = 0; j < kTVec / 2; ++j) bev[j] = bilinear_sum_cl(tap[j], toff, twt);
      request_taps(1);
      __builtin_amdgcn_sched_barrier(0);
      head_l1_third<kTSteps / 2, kTSteps>(A1, 0, lane, cur, c1);  // covers the second half
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < kTVec; ++j) nxt[j] = HEAD_AB(1) ? make_float4((float)lane, 2.f, 2.f, (float)j) : src[2 * (kTSteps / 2) + j];
#pragma unroll
      for (int j = 0; j < kTVec / 2; ++j) bev[kTVec / 2 + j] = bilinear_sum_cl(tap[j], toff, twt);
      head_l1_third(A1, 1, lane, bev, c1);                         // covers the rv third
      head_l1_third(A1, 2, lane, nxt, c1);
    } else {
#pragma unroll 1
      for (int qt = 0; qt < kThirds; ++qt) {
        if (qt + 1 < kThirds) {
#pragma unroll
          for (int j = 0; j < kTVec; ++j)
            nxt[j] = HEAD_AB(1) ? make_float4((float)lane, (float)qt, 2.f, (float)j) : src[(qt + 1) * (kTSteps / 2) + j];
        }
        head_l1_third(A1, qt, lane, cur, c1);
#pragma unroll
        for (int j = 0; j < kTVec; ++j) cur[j] = nxt[j];
      }
    }

    // ---- layer 2: 96 -> 64 on relu(c1), input channels in accumulator order
    f32x16 c2[kM2 / 32];
    int a2_off = lane, a3_off = lane;
#pragma unroll
    for (int mt = 0; mt < kM2 / 32; ++mt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 bias = *reinterpret_cast<const float4*>(B2 + mt * 32 + 8 * g + 4 * hh);
        c2[mt][4 * g] = bias.x; c2[mt][4 * g + 1] = bias.y; c2[mt][4 * g + 2] = bias.z; c2[mt][4 * g + 3] = bias.w;
      }
#pragma unroll
    for (int s = 0; s < (HEAD_AB(4) ? 2 : kS2); ++s) {
      // every 8 steps the LDS offset is re-materialised behind the accumulators: keeps the scheduler from hoisting all
      // 96 weight reads of the layer to its top (which spills)
      if (s % 8 == 0) asm volatile("" : "+v"(a2_off), "+v"(c2[0]), "+v"(c2[1]));
      const float x = fmaxf(c1[s >> 4][s & 15], 0.0f);
#pragma unroll
      for (int mt = 0; mt < kM2 / 32; ++mt)
        c2[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(A2[(mt * kS2 + s) * 64 + a2_off], x, c2[mt], 0, 0, 0);
    }

    // ---- layer 3: 64 -> M3 (<= 32 rows, zero padded) on relu(c2)
    f32x16 c3;
#pragma unroll
    for (int r = 0; r < 16; ++r) c3[r] = 0.0f;
#pragma unroll
    for (int s = 0; s < (HEAD_AB(4) ? 2 : kS3); ++s) {
      if (s % 8 == 0) asm volatile("" : "+v"(a3_off), "+v"(c3));
      c3 = __builtin_amdgcn_mfma_f32_32x32x2f32(A3[s * 64 + a3_off], fmaxf(c2[s >> 4][s & 15], 0.0f), c3, 0, 0, 0);
    }

    // row i of the result = 8 (r >> 2) + 4 h + (r & 3): lane half h, register r
    if (valid && !(HEAD_AB(8) && c3[0] != 12345.678f)) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ch = 8 * (r >> 2) + 4 * hh + (r & 3);
        if (ch < a.M3) a.out[((int64_t)b * a.M3 + ch) * a.N + n] = n < n_live ? c3[r] + B3[ch] : 0.0f;   // tail inside a live tile
      }
    }
  }
}

}  // namespace smos

using namespace smos;

extern "C" int64_t smos_point_head_weight_floats(void) { return kHeadLds; }

template <bool kGather>
static int launch_point_head(HeadArgs a, int64_t K1, int64_t M1, int64_t M2, smos_stream_t stream) {
  SMOS_REQUIRE(K1 == kK1 && M1 == kM1 && M2 == kM2 && a.M3 >= 1 && a.M3 <= 32, "point_head: built for 192 -> 96 -> 64 -> (<=32)");
  SMOS_REQUIRE(a.B > 0 && a.N > 0 && a.rp >= K1 && a.rp % 4 == 0 && (int64_t)a.B * ((a.N + 31) / 32) < (1LL << 31), "point_head: bad sizes");
  SMOS_REQUIRE(a.rows && a.wprep && a.out && (reinterpret_cast<uintptr_t>(a.rows) & 15) == 0, "point_head: null / unaligned pointer");
  KernelSetup ks;
  if (int rc = kernel_setup(reinterpret_cast<const void*>(&point_head<kGather>), kHeadLds * sizeof(float), 0, &ks, "point_head")) return rc;
  const int cus = ks.cus;
  const int64_t tiles = (int64_t)a.B * ((a.N + 31) / 32);
  const int64_t want = (tiles + 7) / 8;
  const int64_t blocks = conv_grid_cap(want < cus ? want : cus);   // (the test hook's cap: several tiles per wave)
  hipLaunchKernelGGL(point_head<kGather>, dim3((unsigned)blocks), dim3(kHeadBlock), kHeadLds * sizeof(float), (hipStream_t)stream, a);
  return check_launch("point_head");
}

static bool fits_int(int64_t v) { return v > 0 && v < (1LL << 31); }

// n_live (device int32, may be null): the first *n_live points of every sample are real, the rest is the scan's padding tail,
// whose logits are written as zeros without being computed.
extern "C" int smos_point_head(const float* rows, int64_t row_pitch, const float* wprep, float* out, int64_t B, int64_t N,
                               int64_t K1, int64_t M1, int64_t M2, int64_t M3, const int32_t* n_live, smos_stream_t stream) {
  SMOS_REQUIRE(fits_int(B) && fits_int(N) && M3 <= 32, "point_head: bad sizes");
  HeadArgs a = {};
  a.rows = rows; a.wprep = wprep; a.out = out; a.n_live = n_live; a.rp = row_pitch; a.B = (int)B; a.N = (int)N; a.M3 = (int)M3;
  return launch_point_head<false>(a, K1, M1, M2, stream);
}

// The same with channels [64, 128) of every row taken from `grid` by the bilinear gather of smos_gather_scatter_cl instead
// of from the row: floats [64, 128) of `rows` are neither read nor written.
extern "C" int smos_point_head_gather(const float* rows, int64_t row_pitch, const float* wprep, float* out, int64_t B, int64_t N,
                                      int64_t K1, int64_t M1, int64_t M2, int64_t M3, const int32_t* n_live, const float* grid,
                                      int64_t grid_pitch, int64_t Hg, int64_t Wg, const float* gcoord, int32_t Kg,
                                      int64_t g_batch_stride, const float* gscale, smos_stream_t stream) {
  SMOS_REQUIRE(fits_int(B) && fits_int(N) && M3 <= 32, "point_head: bad sizes");
  SMOS_REQUIRE(grid && gcoord && gscale && (reinterpret_cast<uintptr_t>(grid) & 15) == 0 && grid_pitch >= 64 && grid_pitch % 4 == 0,
               "point_head_gather: null / unaligned grid or bad pitch (64 channels are read)");
  SMOS_REQUIRE(Hg > 0 && Wg > 0 && Kg >= 2 && g_batch_stride >= 0, "point_head_gather: bad grid size / coordinate view");
  // the taps are addressed by 32-bit byte offsets from the grid's first byte
  const int64_t grid_bytes = ((B * Hg * Wg - 1) * grid_pitch + 64) * 4;
  SMOS_REQUIRE(Hg * Wg < (1LL << 31) && grid_bytes < (1LL << 31), "point_head_gather: grid of 2 GiB or more");
  HeadArgs a = {};
  a.rows = rows; a.wprep = wprep; a.out = out; a.n_live = n_live; a.rp = row_pitch; a.B = (int)B; a.N = (int)N; a.M3 = (int)M3;
  a.grid = grid; a.gcoord = gcoord; a.gp = grid_pitch; a.gbs = g_batch_stride; a.Kg = Kg; a.Hg = (int)Hg; a.Wg = (int)Wg;
  a.grid_bytes = (int)grid_bytes; a.gsy = gscale[0]; a.gsx = gscale[1];
  return launch_point_head<true>(a, K1, M1, M2, stream);
}
