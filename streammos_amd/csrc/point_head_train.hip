// Training point head: CatFusion + PredBranch of the module graph
//     cat(a, b, c) [B,192,N,1] -> dropout 0.2 -> 1x1 192->96 -> BN1 -> ReLU -> 1x1 96->64 -> BN2 -> ReLU -> dropout 0.2 -> 1x1 64->3 + bias
// as one forward and one backward entry, batch statistics included.  The inputs are the three channel-major [B,64,N,1]
// features; nothing of the chain is stored: every pass recomputes it from the inputs, the packed keep bits and the folded
// statistics ("fold"), so what lives between forward and backward is the inputs, 32 bytes of keep bits per point and fold.
//
//   forward, training   z1 sums about the first point -> BN1 statistics | z2 sums likewise -> BN2 statistics | logits
//   forward, eval       fold the running statistics | logits
//   backward            pass 1: dbeta2, dgamma2, dW3, db3 | pass 2: dW2, dbeta1, dgamma1 | pass 3: dW1, input gradients
//
// Arithmetic: the chain runs as fp32 FMA chains on the vector unit, one point per lane, weights wave-uniform (scalar
// loads); loads along N coalesce per channel plane.  The two weight gradients that are GEMMs over the points (dW2 64x96,
// dW1 96x192) go through v_mfma_f32_32x32x2_f32 with the points on K: a wave's 64 points are staged point-major in LDS and
// every wave of the block accumulates its own 32x32 tiles of the result over all staged points.
//
// Reductions: the fixed-order sums of csrc/chunk_sums.h over chunks of kPhChunk = 1024 points; the bits of every result
// depend on the data alone.
//
// Accuracy: layer 1 runs on xt - xt(first point), so z1 is formed about its value at the first point from differences
// of the inputs; the z2 sums are taken about z2 at the first point; both are corrected in float64.  In the chain a mean is
// subtracted as a float pair (hi, lo) before scaling.
//
// Keep bits: 8 words per point in word planes (masks[w * P + p]): bit k & 31 of word k >> 5 keeps input channel k (w < 6),
// bit j & 31 of word 6 + (j >> 5) keeps channel j of the second dropout.  Generated bits: Philox4x32-10 with key = the two
// halves of seed[0] and counter (p, 8 w + i, lo(seed[1]), hi(seed[1])); output word v of call i decides bit 4 i + v; a bit
// is kept iff its 32-bit draw is below kKeepBelow = 3435973837 = ceil(0.8 * 2^32), a keep probability of 0.8 + 4.7e-11.
#include "chunk_sums.h"
#include "philox.h"

namespace smos {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kPhChunk = 1024;                 // points per chunk of partial sums
constexpr int kPhBlock = 256;
constexpr int kK = 192, kM1 = 96, kM2 = 64, kM3 = 3;
constexpr uint32_t kKeepBelow = 3435973837u;
constexpr int kPH = kM1 + 1, kPX = kK + 1, kPZ = kM2 + 1;      // odd LDS row pitches: a lane's own row is conflict-free
constexpr int kColsS1 = 2 * kM1, kColsS2 = 2 * kM2;
constexpr int kColsB1 = 2 * kM2 + kM3 * kM2 + 4;               // dbeta2 | dgamma2 | dW3 | db3 (padded)
constexpr int kColsB2 = kM2 * kM1 + 2 * kM1;                   // dW2 | dbeta1 | dgamma1
constexpr int kColsB3 = kM1 * kK;                              // dW1
constexpr int kLds2 = (3 * 64 * kPH + 4 * 64 * kPZ) * 4;
constexpr int kLds3 = 256 * kPH * 4;       // >= (64 * kPH + 64 * kPX) * 4

// the folded block (floats)
enum : int {
  F_W1T = 0,                                  // [k][j]: W1 transposed, so that a k-step reads 96 consecutive weights
  F_W2 = kK * kM1, F_W3 = F_W2 + kM2 * kM1, F_B3 = F_W3 + kM3 * kM2,       // copies: the chain reads one read-only block
  F_G1 = F_B3 + 4, F_BE1 = F_G1 + kM1, F_G2 = F_BE1 + kM1, F_BE2 = F_G2 + kM2,
  F_X0 = F_BE2 + kM2,                         // xt of the first point: layer 1 runs on xt - xt0
  F_MU1H = F_X0 + kK, F_MU1L = F_MU1H + kM1, F_R1 = F_MU1L + kM1,
  F_MU2H = F_R1 + kM1, F_MU2L = F_MU2H + kM2, F_R2 = F_MU2L + kM2, F_SH2 = F_R2 + kM2,
  F_END = F_SH2 + kM2
};
// float64 statistics the forward leaves: mean and biased variance of z1 and z2 as normalised with
enum : int { D_MU1 = 0, D_VAR1 = kM1, D_MU2 = 2 * kM1, D_VAR2 = 2 * kM1 + kM2, D_END = 2 * kM1 + 2 * kM2 };
// work buffer: the coefficients of the backward are doubles, dbeta / P and dgamma / P of both batch norms
enum : int { C_B2 = 0, C_G2 = kM2, C_B1 = 2 * kM2, C_G1 = 2 * kM2 + kM1 };

struct PhIn {
  const float* xa; const float* xb; const float* xc;   // [B,64,N] with channel pitch pa / pb / pc
  int64_t pa, pb, pc;
  const uint32_t* mask;                                  // 8 word planes of P, or null: nothing dropped
  float scale;                                           // 1 / keep probability (1 without masks)
  int64_t P, N;
};

struct PhParams {
  const float* w1; const float* g1; const float* be1; float* rm1; float* rv1;
  const float* w2; const float* g2; const float* be2; float* rm2; float* rv2;
  const float* w3; const float* b3;
  double eps[2], mom[2];
};

// eight input channels of a point and their keep bits: group g = channels [8 g, 8 g + 8) of the concatenation
struct PhX {
  float v[8];
  uint32_t m;
};

__device__ __forceinline__ void ph_load8(const PhIn& in, const ChunkPoint& pt, int g, PhX& o) {
  const int i = g >> 3;
  const float* base = i == 0 ? in.xa : i == 1 ? in.xb : in.xc;
  const int64_t pitch = i == 0 ? in.pa : i == 1 ? in.pb : in.pc;
  const float* src = base + (pt.s * 64 + (g & 7) * 8) * pitch + pt.n;
#pragma unroll
  for (int c = 0; c < 8; ++c) o.v[c] = src[c * pitch];
  uint32_t word = 0xffffffffu;
  if (in.mask) word = in.mask[(int64_t)(g >> 2) * in.P + pt.pc];       // (wave-uniform branch)
  o.m = word >> ((g & 3) * 8);
}

__device__ __forceinline__ float ph_xt(const PhIn& in, const PhX& x, int c) { return ((x.m >> c) & 1u) ? x.v[c] * in.scale : 0.0f; }

// z1c = W1 (xt - xt0) = z1 - z1(first point), the next group's loads in flight behind the current group's 8 x 96 FMAs.  The
// difference is taken on the inputs: a channel with mean 1000 and spread 0.01 enters at its spread, so z1c is as exact as
// its own size allows and the mean that BN1 subtracts (fold: the mean of z1c, or running_mean - z1(first point)) is small.
__device__ __forceinline__ void ph_z1(const PhIn& in, const float* __restrict__ fold, const ChunkPoint& pt, float (&z)[kM1]) {
#pragma unroll
  for (int j = 0; j < kM1; ++j) z[j] = 0.0f;
  PhX cur, nxt;
  ph_load8(in, pt, 0, cur);
#pragma unroll 1
  for (int g = 0; g < kK / 8; ++g) {
    ph_load8(in, pt, g + 1 < kK / 8 ? g + 1 : g, nxt);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float xt = ph_xt(in, cur, c) - fold[F_X0 + g * 8 + c];
      const float* wr = fold + F_W1T + (g * 8 + c) * kM1;
#pragma unroll
      for (int j = 0; j < kM1; ++j) z[j] = fmaf(wr[j], xt, z[j]);
    }
    cur = nxt;
  }
}

__device__ __forceinline__ void ph_zhat1(const float* __restrict__ fold, float (&z)[kM1]) {
#pragma unroll
  for (int j = 0; j < kM1; ++j) z[j] = ((z[j] - fold[F_MU1H + j]) - fold[F_MU1L + j]) * fold[F_R1 + j];
}

__device__ __forceinline__ void ph_h1(const float* __restrict__ fold, const float (&zh)[kM1], float (&h)[kM1]) {
#pragma unroll
  for (int j = 0; j < kM1; ++j) h[j] = fmaxf(fmaf(fold[F_G1 + j], zh[j], fold[F_BE1 + j]), 0.0f);
}

__device__ __forceinline__ float ph_z2(const float* __restrict__ wr, const float (&h)[kM1]) {
  float z = 0.0f;
#pragma unroll
  for (int k = 0; k < kM1; ++k) z = fmaf(wr[k], h[k], z);
  return z;
}

// keep bit j of the second dropout from the point's two words
__device__ __forceinline__ bool ph_keep2(uint32_t m0, uint32_t m1, int j) { return (((j < 32 ? m0 : m1) >> (j & 31)) & 1u) != 0; }

__device__ __forceinline__ void ph_mask2(const PhIn& in, const ChunkPoint& pt, uint32_t& m0, uint32_t& m1) {
  m0 = m1 = 0xffffffffu;
  if (in.mask) {
    m0 = in.mask[6 * in.P + pt.pc];
    m1 = in.mask[7 * in.P + pt.pc];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ph_prep(PhParams q, PhIn in, float* __restrict__ fold) {
  const int i = blockIdx.x * 256 + threadIdx.x;      // over W1 [j][k]
  if (i < kM1 * kK) fold[F_W1T + (i % kK) * kM1 + i / kK] = q.w1[i];
  if (i < kM2 * kM1) fold[F_W2 + i] = q.w2[i];
  if (i < kM3 * kM2) fold[F_W3 + i] = q.w3[i];
  if (i < 4) fold[F_B3 + i] = i < kM3 ? q.b3[i] : 0.0f;
  if (i < kK) {
    const int t = i >> 6;
    const float x = (t == 0 ? in.xa : t == 1 ? in.xb : in.xc)[(i & 63) * (t == 0 ? in.pa : t == 1 ? in.pb : in.pc)];
    const uint32_t word = in.mask ? in.mask[(int64_t)(i >> 5) * in.P] : 0xffffffffu;
    fold[F_X0 + i] = ((word >> (i & 31)) & 1u) ? x * in.scale : 0.0f;
  }
  if (i < kM1) {
    fold[F_G1 + i] = q.g1[i];
    fold[F_BE1 + i] = q.be1[i];
  }
  if (i < kM2) {
    fold[F_G2 + i] = q.g2[i];
    fold[F_BE2 + i] = q.be2[i];
  }
}

// One point per lane through the chain.
//   MODE 1  sum z1c, sum z1c^2 (z1c is z1 about its value at the first point)
//   MODE 2  the shift of z2                                  MODE 3  the same sums of z2
//   MODE 4  the logits                                       MODE 5  backward pass 1: sum da2, sum da2 zhat2, sum g (x) h2d, sum g
// Sums: per trip a wave sum in fp32, added in float64 by the lane that owns the column; the four waves add in a fixed order.
template <int MODE>
__global__ __launch_bounds__(256) void ph_pass(PhIn in, const float* __restrict__ fold, float* __restrict__ shift,
                                               const float* __restrict__ g, float* __restrict__ out, double* __restrict__ partial,
                                               int64_t nchunks) {
  __shared__ double red[4][kColsB1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t P = in.P, N = in.N;
  for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int t = 0; t < kPhChunk / kPhBlock; ++t) {
      const int64_t tile0 = chunk * kPhChunk + t * kPhBlock;
      if (tile0 >= P) break;
      const ChunkPoint pt = chunk_point(MODE == 2 ? 0 : tile0 + tid, P, N);
      float z[kM1];
      ph_z1(in, fold, pt, z);
      if (MODE == 1) {
#pragma unroll
        for (int j = 0; j < kM1; ++j) {
          const float v = pt.live ? z[j] : 0.0f;
          const float s1 = wave_sum(v), s2 = wave_sum(v * v);
          if (j < 64) {
            acc[0] += lane == j ? (double)s1 : 0.0;
            acc[1] += lane == j ? (double)s2 : 0.0;
          } else {
            acc[2] += lane == j - 64 ? (double)s1 : 0.0;
            acc[3] += lane == j - 64 ? (double)s2 : 0.0;
          }
          __builtin_amdgcn_sched_barrier(0);      // one column at a time: interleaving all 96 costs hundreds of registers
        }
      } else {
        ph_zhat1(fold, z);
        float h[kM1];
        ph_h1(fold, z, h);
        uint32_t m0, m1;
        ph_mask2(in, pt, m0, m1);
        float gl[kM3] = {0.f, 0.f, 0.f}, lg[kM3] = {0.f, 0.f, 0.f};
        if (MODE == 5) {
#pragma unroll
          for (int m = 0; m < kM3; ++m) gl[m] = g[(pt.s * kM3 + m) * N + pt.n];
        }
#pragma unroll 2
        for (int j = 0; j < kM2; ++j) {
          const float z2 = ph_z2(fold + F_W2 + j * kM1, h);
          if (MODE == 2) {
            shift[j] = z2;                      // (every lane holds the first point: the same value from all)
          } else if (MODE == 3) {
            const float v = pt.live ? z2 - fold[F_SH2 + j] : 0.0f;
            const float s1 = wave_sum(v), s2 = wave_sum(v * v);
            acc[0] += lane == j ? (double)s1 : 0.0;
            acc[1] += lane == j ? (double)s2 : 0.0;
          } else {
            const float zh = ((z2 - fold[F_MU2H + j]) - fold[F_MU2L + j]) * fold[F_R2 + j];
            const float pre = fmaf(fold[F_G2 + j], zh, fold[F_BE2 + j]);
            const bool keep = ph_keep2(m0, m1, j);
            const float h2d = keep ? fmaxf(pre, 0.0f) * in.scale : 0.0f;
            if (MODE == 4) {
#pragma unroll
              for (int m = 0; m < kM3; ++m) lg[m] = fmaf(fold[F_W3 + m * kM2 + j], h2d, lg[m]);
            } else {
              float dh = 0.0f;
#pragma unroll
              for (int m = 0; m < kM3; ++m) dh = fmaf(fold[F_W3 + m * kM2 + j], gl[m], dh);
              const float da = (pt.live && keep && pre > 0.0f) ? dh * in.scale : 0.0f;
              const float hl = pt.live ? h2d : 0.0f;
              const float s0 = wave_sum(da), s1 = wave_sum(da * zh);
              const float t0 = wave_sum(gl[0] * hl), t1 = wave_sum(gl[1] * hl), t2 = wave_sum(gl[2] * hl);
              acc[0] += lane == j ? (double)s0 : 0.0;
              acc[1] += lane == j ? (double)s1 : 0.0;
              acc[2] += lane == j ? (double)t0 : 0.0;
              acc[3] += lane == j ? (double)t1 : 0.0;
              acc[4] += lane == j ? (double)t2 : 0.0;
            }
          }
        }
        if (MODE == 4) {
          if (pt.live) {
#pragma unroll
            for (int m = 0; m < kM3; ++m) out[(pt.s * kM3 + m) * N + pt.n] = lg[m] + fold[F_B3 + m];
          }
        }
        if (MODE == 5) {
#pragma unroll
          for (int m = 0; m < kM3; ++m) {
            const float s = wave_sum(pt.live ? gl[m] : 0.0f);
            acc[5] += lane == m ? (double)s : 0.0;
          }
        }
      }
      if (MODE == 2) break;
    }
    if (MODE == 1) {
      red[wave][lane] = acc[0];
      red[wave][kM1 + lane] = acc[1];
      if (lane < kM1 - 64) {
        red[wave][64 + lane] = acc[2];
        red[wave][kM1 + 64 + lane] = acc[3];
      }
      block_columns_store<kColsS1>(red, partial, chunk, tid);
    } else if (MODE == 3) {
      red[wave][lane] = acc[0];
      red[wave][kM2 + lane] = acc[1];
      block_columns_store<kColsS2>(red, partial, chunk, tid);
    } else if (MODE == 5) {
#pragma unroll
      for (int i = 0; i < 5; ++i) red[wave][i * 64 + lane] = acc[i];
      if (lane < 4) red[wave][320 + lane] = acc[5];
      block_columns_store<kColsB1>(red, partial, chunk, tid);
    }
  }
}

// BN statistics of layer L (1 or 2): training from the sums about the shift, the running buffers updated; eval from the
// buffers.  The shift of layer 1 is z1 at the first point, W1 xt0, formed here in float64; the chain works on z1 - shift.
__global__ __launch_bounds__(128) void ph_fin_stats(int layer, int training, const double* __restrict__ gsum, int64_t ngroups, int64_t P,
                                                    PhParams q, float* __restrict__ fold, double* __restrict__ dstat) {
  const int j = threadIdx.x, M = layer == 1 ? kM1 : kM2;
  if (j >= M) return;
  float* rm = layer == 1 ? q.rm1 : q.rm2;
  float* rv = layer == 1 ? q.rv1 : q.rv2;
  const double eps = q.eps[layer - 1], mom = q.mom[layer - 1];
  double shift = 0.0;
  if (layer == 1) {
    for (int k = 0; k < kK; ++k) shift += (double)q.w1[j * kK + k] * (double)fold[F_X0 + k];
  } else {
    shift = (double)fold[F_SH2 + j];
  }
  double mu, var;
  if (training) {
    bn_stats_about_shift(gsum, ngroups, M, j, P, &mu, &var);
    mu += shift;
    bn_running_update(rm, rv, j, mom, mu, var, P);
  } else {
    mu = (double)rm[j];
    var = (double)rv[j];
  }
  const double sub = layer == 1 ? mu - shift : mu;       // what the chain subtracts: layer 1 works about the shift
  split_hi_lo(sub, &fold[(layer == 1 ? F_MU1H : F_MU2H) + j], &fold[(layer == 1 ? F_MU1L : F_MU2L) + j]);
  fold[(layer == 1 ? F_R1 : F_R2) + j] = (float)(1.0 / sqrt(var + eps));
  dstat[(layer == 1 ? D_MU1 : D_MU2) + j] = mu;
  dstat[(layer == 1 ? D_VAR1 : D_VAR2) + j] = var;
}

// ---------------------------------------------------------------------------------------------------------------------
// Backward passes 2 and 3.  Both recompute the chain down to da1 = (W2^T dz2) [a1 > 0]: one walk over the 64 output
// channels of layer 2 forms z2[j], dz2[j] and adds dz2[j] W2[j][:] into da1 with the weight row it already holds.
//   PASS 2  sum da1, sum da1 zhat1; dW2 = sum dz2 (x) h1
//   PASS 3  dz1; the input gradients (W1^T dz1) keep1 scale; dW1 = sum dz1 (x) xt
// The sums over points: per round r the wave r stages its 64 points point-major in LDS, then every wave works on the 64
// staged points.  The GEMMs run on v_mfma_f32_32x32x2_f32 with the points on K, the row operand on the accumulator
// registers, the column operand on the lane.  dW2: waves 0..2 own columns [32 w, 32 w + 32) of h1, both row tiles, while wave
// 3 adds up the columns of da1 and da1 zhat1 (a lane per column, points in order).  dW1: wave w owns column tile w of xt,
// waves 0 and 1 also tiles 4 and 5; three row tiles each.
// LDS, pass 2: h1 | da1 | da1 zhat1 of the staged wave, [64][kPH] each, then dz2 [4][64][kPZ] of every wave's points.
// LDS, pass 3: zhat1 of all 256 points [256][kPH], parked there while h1 and da1 need the registers; once every wave has
// taken its zhat1 back the same space stages dz1 [64][kPH] | xt [64][kPX].
template <int PASS>
__global__ __launch_bounds__(256) void ph_bwd(PhIn in, const float* __restrict__ fold, const double* __restrict__ coef,
                                              const float* __restrict__ g, float* __restrict__ partial, float* __restrict__ dxa,
                                              float* __restrict__ dxb, float* __restrict__ dxc, int need_w, int64_t nchunks) {
  extern __shared__ float lds[];
  float* s_row = lds;
  float* s_da = lds + 64 * kPH;                           // pass 2
  float* s_dazh = lds + 2 * 64 * kPH;                     // pass 2
  float* s_dz2 = lds + 3 * 64 * kPH;                      // pass 2
  float* s_x = lds + 64 * kPH;                            // pass 3
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 31, hh = lane >> 5;
  const int64_t P = in.P, N = in.N;
  constexpr int kTiles = PASS == 2 ? 2 : 6;
  for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    f32x16 acc[kTiles];
#pragma unroll
    for (int i = 0; i < kTiles; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
    double sum[4] = {0, 0, 0, 0};       // pass 2, wave 3: columns lane and 64 + (lane & 31) of da1, of da1 zhat1
    for (int t = 0; t < kPhChunk / kPhBlock; ++t) {
      const int64_t tile0 = chunk * kPhChunk + t * kPhBlock;
      if (tile0 >= P) break;
      const ChunkPoint pt = chunk_point(tile0 + tid, P, N);
      float zh[kM1], h[kM1], da1[kM1];
      ph_z1(in, fold, pt, zh);
      ph_zhat1(fold, zh);
      ph_h1(fold, zh, h);
      float* my_zh = lds + tid * kPH;
      if (PASS == 3) {
#pragma unroll
        for (int k = 0; k < kM1; ++k) my_zh[k] = zh[k];
      }
      {
        uint32_t m0, m1;
        ph_mask2(in, pt, m0, m1);
        float gl[kM3];
#pragma unroll
        for (int m = 0; m < kM3; ++m) gl[m] = g[(pt.s * kM3 + m) * N + pt.n];
#pragma unroll
        for (int k = 0; k < kM1; ++k) da1[k] = 0.0f;
        float* my_dz = s_dz2 + (wave * 64 + lane) * kPZ;
#pragma unroll 1
        for (int j = 0; j < kM2; ++j) {
          const float* wr = fold + F_W2 + j * kM1;
          const float z2 = ph_z2(wr, h);
          const float zh2 = ((z2 - fold[F_MU2H + j]) - fold[F_MU2L + j]) * fold[F_R2 + j];
          const float pre = fmaf(fold[F_G2 + j], zh2, fold[F_BE2 + j]);
          float dh = 0.0f;
#pragma unroll
          for (int m = 0; m < kM3; ++m) dh = fmaf(fold[F_W3 + m * kM2 + j], gl[m], dh);
          const float da = (ph_keep2(m0, m1, j) && pre > 0.0f) ? dh * in.scale : 0.0f;
          // (in float64: with few points the three terms cancel to eps / (var + eps) of their size)
          float dz = (float)((double)(fold[F_G2 + j] * fold[F_R2 + j]) * (((double)da - coef[C_B2 + j]) - (double)zh2 * coef[C_G2 + j]));
          dz = pt.live ? dz : 0.0f;
          if (PASS == 2) my_dz[j] = dz;
#pragma unroll
          for (int k = 0; k < kM1; ++k) da1[k] = fmaf(wr[k], dz, da1[k]);
        }
      }
      // a1 > 0 is h1 > 0.  (A point past the end has dz2 = 0, so its da1 is 0.)
#pragma unroll
      for (int k = 0; k < kM1; ++k) da1[k] = h[k] > 0.0f ? da1[k] : 0.0f;
      if (PASS == 2) {
        for (int r = 0; r < 4; ++r) {
          if (wave == r) {
#pragma unroll
            for (int k = 0; k < kM1; ++k) {
              s_row[lane * kPH + k] = h[k];
              s_da[lane * kPH + k] = da1[k];
              s_dazh[lane * kPH + k] = da1[k] * zh[k];
            }
          }
          __syncthreads();
          if (wave < 3) {
            if (need_w) {
              const float* sa = s_dz2 + r * 64 * kPZ;
#pragma unroll 4
              for (int s = 0; s < 32; ++s) {
                const int row = 2 * s + hh;
                const float b = s_row[row * kPH + wave * 32 + col];
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                  acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(sa[row * kPZ + mt * 32 + col], b, acc[mt], 0, 0, 0);
              }
            }
          } else {
            const int c2 = 64 + (lane & 31);
            float a0 = 0.0f, a1 = 0.0f, b0 = 0.0f, b1 = 0.0f;
#pragma unroll 4
            for (int p = 0; p < 64; ++p) {
              a0 += s_da[p * kPH + lane];
              a1 += s_dazh[p * kPH + lane];
              b0 += s_da[p * kPH + c2];
              b1 += s_dazh[p * kPH + c2];
            }
            sum[0] += (double)a0;
            sum[1] += (double)a1;
            sum[2] += (double)b0;
            sum[3] += (double)b1;
          }
          __syncthreads();
        }
      } else {
#pragma unroll
        for (int k = 0; k < kM1; ++k) {
          const float dz = (float)((double)(fold[F_G1 + k] * fold[F_R1 + k]) * (((double)da1[k] - coef[C_B1 + k]) - (double)my_zh[k] * coef[C_G1 + k]));
          da1[k] = pt.live ? dz : 0.0f;          // dz1 from here on
        }
        if (dxa) {
#pragma unroll 1
          for (int gq = 0; gq < kK / 8; ++gq) {
            const int i = gq >> 3;
            float* dst = (i == 0 ? dxa : i == 1 ? dxb : dxc) + (pt.s * 64 + (gq & 7) * 8) * N + pt.n;
            uint32_t word = 0xffffffffu;
            if (in.mask) word = in.mask[(int64_t)(gq >> 2) * P + pt.pc];
            word >>= (gq & 3) * 8;
#pragma unroll 2
            for (int c = 0; c < 8; ++c) {
              const float* wr = fold + F_W1T + (gq * 8 + c) * kM1;
              float v = 0.0f;
#pragma unroll
              for (int j = 0; j < kM1; ++j) v = fmaf(wr[j], da1[j], v);
              v = ((word >> c) & 1u) ? v * in.scale : 0.0f;
              if (pt.live) dst[c * N] = v;
            }
          }
        }
        if (need_w) {
          __syncthreads();            // every wave has its zhat1 back: the space turns into the staging buffers
          for (int r = 0; r < 4; ++r) {
            if (wave == r) {
#pragma unroll
              for (int k = 0; k < kM1; ++k) s_row[lane * kPH + k] = da1[k];
              PhX x;
#pragma unroll 1
              for (int gq = 0; gq < kK / 8; ++gq) {
                ph_load8(in, pt, gq, x);
#pragma unroll
                for (int c = 0; c < 8; ++c) s_x[lane * kPX + gq * 8 + c] = ph_xt(in, x, c);
              }
            }
            __syncthreads();
#pragma unroll 2
            for (int s = 0; s < 32; ++s) {
              const int row = 2 * s + hh;
              float a[3];
#pragma unroll
              for (int mt = 0; mt < 3; ++mt) a[mt] = s_row[row * kPH + mt * 32 + col];
              const float b0 = s_x[row * kPX + wave * 32 + col];
#pragma unroll
              for (int mt = 0; mt < 3; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt], b0, acc[mt], 0, 0, 0);
              if (wave < 2) {
                const float b1 = s_x[row * kPX + (wave + 4) * 32 + col];
#pragma unroll
                for (int mt = 0; mt < 3; ++mt) acc[3 + mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt], b1, acc[3 + mt], 0, 0, 0);
              }
            }
            __syncthreads();
          }
        }
      }
    }
    // the chunk's partial row.  Accumulator register r of lane (col, hh) is row 8 (r >> 2) + 4 hh + (r & 3), column col of its tile.
    float* prow = partial + chunk * (PASS == 2 ? kColsB2 : kColsB3);
    if (PASS == 2) {
      if (wave < 3) {
        int off = 4 * hh * kM1 + wave * 32 + col;
        asm volatile("" : "+v"(off));       // (formed here: hoisted out of the chunk loop, the 32 addresses would live across it)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) prow[off + (mt * 32 + 8 * (r >> 2) + (r & 3)) * kM1] = acc[mt][r];
      } else {
        prow[kM2 * kM1 + lane] = (float)sum[0];
        prow[kM2 * kM1 + kM1 + lane] = (float)sum[1];
        if (lane < kM1 - 64) {
          prow[kM2 * kM1 + 64 + lane] = (float)sum[2];
          prow[kM2 * kM1 + kM1 + 64 + lane] = (float)sum[3];
        }
      }
    } else if (need_w) {
      int off = 4 * hh * kK + wave * 32 + col;
      asm volatile("" : "+v"(off));         // (as above)
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        if (ct == 1 && wave >= 2) break;
#pragma unroll
        for (int mt = 0; mt < 3; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) prow[off + (mt * 32 + 8 * (r >> 2) + (r & 3)) * kK + 4 * ct * 32] = acc[3 * ct + mt][r];
      }
    }
  }
}

struct PhGrads {
  float* w1; float* g1; float* be1; float* w2; float* g2; float* be2; float* w3; float* b3;
};

__global__ __launch_bounds__(256) void ph_fin_b1(int have, int training, const double* __restrict__ gsum, int64_t ngroups, int64_t P,
                                                 PhGrads o, double* __restrict__ coef) {
  const int i = threadIdx.x;
  if (i < kM2) {
    const double db = have ? total(gsum, ngroups, kColsB1, i) : 0.0, dg = have ? total(gsum, ngroups, kColsB1, kM2 + i) : 0.0;
    if (o.be2) o.be2[i] = (float)db;
    if (o.g2) o.g2[i] = (float)dg;
    coef[C_B2 + i] = training ? db / (double)P : 0.0;
    coef[C_G2 + i] = training ? dg / (double)P : 0.0;
  }
  if (have && o.w3 && i < kM3 * kM2) o.w3[i] = (float)total(gsum, ngroups, kColsB1, 2 * kM2 + i);
  if (have && o.b3 && i < kM3) o.b3[i] = (float)total(gsum, ngroups, kColsB1, 2 * kM2 + kM3 * kM2 + i);
}

__global__ __launch_bounds__(256) void ph_fin_b2(int have, int training, const double* __restrict__ gsum, int64_t ngroups, int64_t P,
                                                 PhGrads o, double* __restrict__ coef) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < kM2 * kM1) {
    if (have && o.w2) o.w2[i] = (float)total(gsum, ngroups, kColsB2, i);
  } else if (i < kColsB2) {
    const int k = i - kM2 * kM1;
    const double v = have ? total(gsum, ngroups, kColsB2, i) : 0.0;
    if (k < kM1) {
      if (o.be1) o.be1[k] = (float)v;
      coef[C_B1 + k] = training ? v / (double)P : 0.0;
    } else {
      if (o.g1) o.g1[k - kM1] = (float)v;
      coef[C_G1 + k - kM1] = training ? v / (double)P : 0.0;
    }
  }
}

__global__ __launch_bounds__(256) void ph_fin_b3(const double* __restrict__ gsum, int64_t ngroups, float* __restrict__ d_w1) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < kColsB3) d_w1[i] = (float)total(gsum, ngroups, kColsB3, i);
}

// keep bits: packed from explicit byte masks, or drawn (header)
__global__ __launch_bounds__(256) void ph_masks(const uint8_t* __restrict__ keep1, const uint8_t* __restrict__ keep2,
                                                const int64_t* __restrict__ seed, int64_t P, int64_t N, uint32_t* __restrict__ masks) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= 8 * P) return;
  const int w = (int)(i / P);
  const int64_t p = i - (int64_t)w * P;
  uint32_t bits = 0;
  if (keep1) {
    const int64_t s = p / N, n = p - s * N;
    const uint8_t* src = w < 6 ? keep1 + (s * kK + w * 32) * N + n : keep2 + (s * kM2 + (w - 6) * 32) * N + n;
    for (int c = 0; c < 32; ++c) bits |= (src[c * N] != 0 ? 1u : 0u) << c;
  } else {
    const uint64_t s0 = (uint64_t)seed[0], s1 = (uint64_t)seed[1];
    for (int c = 0; c < 8; ++c) {
      const Philox4 d = philox4x32_10((uint32_t)p, (uint32_t)(w * 8 + c), (uint32_t)s1, (uint32_t)(s1 >> 32), (uint32_t)s0, (uint32_t)(s0 >> 32));
#pragma unroll
      for (int v = 0; v < 4; ++v) bits |= (d.v[v] < kKeepBelow ? 1u : 0u) << (4 * c + v);
    }
  }
  masks[i] = bits;
}

// the widest partial row is pass 3 of the backward
ChunkWork ph_work(void* work, int64_t P) { return chunk_work(work, P, kPhChunk, kColsB3); }

int ph_params(const void* const* p, const double* eps_mom, PhParams* q) {
  for (int i = 0; i < 12; ++i) SMOS_REQUIRE(p[i], "point_head_train: null parameter pointer %d", i);
  q->w1 = (const float*)p[0]; q->g1 = (const float*)p[1]; q->be1 = (const float*)p[2]; q->rm1 = (float*)p[3]; q->rv1 = (float*)p[4];
  q->w2 = (const float*)p[5]; q->g2 = (const float*)p[6]; q->be2 = (const float*)p[7]; q->rm2 = (float*)p[8]; q->rv2 = (float*)p[9];
  q->w3 = (const float*)p[10]; q->b3 = (const float*)p[11];
  for (int i = 0; i < 2; ++i) {
    q->eps[i] = eps_mom[i];
    q->mom[i] = eps_mom[2 + i];
  }
  return SMOS_OK;
}

int ph_inputs(const char* what, const float* a, const float* b, const float* c, const int64_t* pitch, const uint32_t* masks, double scale,
              int64_t B, int64_t N, PhIn* in) {
  SMOS_REQUIRE(a && b && c && pitch, "%s: null input pointer", what);
  SMOS_REQUIRE(B > 0 && N > 0 && pitch[0] >= N && pitch[1] >= N && pitch[2] >= N, "%s: bad sizes", what);
  in->xa = a; in->xb = b; in->xc = c;
  in->pa = pitch[0]; in->pb = pitch[1]; in->pc = pitch[2];
  in->mask = masks;
  in->scale = masks ? (float)scale : 1.0f;
  in->P = B * N;
  in->N = N;
  return SMOS_OK;
}

}  // namespace
}  // namespace smos

using namespace smos;

extern "C" int32_t smos_point_head_train_chunk(void) { return kPhChunk; }
extern "C" int32_t smos_point_head_train_fold_floats(void) { return F_END; }
extern "C" int32_t smos_point_head_train_stat_doubles(void) { return D_END; }

extern "C" int64_t smos_point_head_train_work_bytes(int64_t P) {
  return ph_work(nullptr, P).bytes;
}

extern "C" int64_t smos_point_head_train_mask_words(int64_t P) { return ph_work(nullptr, P).bytes < 0 ? -1 : 8 * P; }

extern "C" int smos_point_head_train_masks(const uint8_t* keep1, const uint8_t* keep2, const int64_t* seed, int64_t B, int64_t N,
                                           uint32_t* masks, smos_stream_t stream) {
  SMOS_REQUIRE(masks && B > 0 && N > 0 && smos_point_head_train_mask_words(B * N) > 0, "point_head_train_masks: null pointer / bad sizes");
  SMOS_REQUIRE((keep1 && keep2) || (!keep1 && !keep2 && seed), "point_head_train_masks: want both byte masks, or none and a seed");
  const int64_t P = B * N;
  hipLaunchKernelGGL(ph_masks, dim3((unsigned)((8 * P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, keep1, keep2, seed, P, N, masks);
  return check_launch("point_head_train_masks");
}

extern "C" int smos_point_head_train_fwd(const float* a, const float* b, const float* c, const int64_t* pitch, const uint32_t* masks,
                                         double scale, int64_t B, int64_t N, int32_t training, const void* const* params,
                                         const double* eps_mom, float* logits, float* fold, double* dstat, void* work,
                                         int64_t work_bytes, smos_stream_t stream) {
  PhIn in;
  if (int rc = ph_inputs("point_head_train_fwd", a, b, c, pitch, masks, scale, B, N, &in)) return rc;
  SMOS_REQUIRE(params && eps_mom && logits && fold && dstat && work, "point_head_train_fwd: null pointer");
  const int64_t P = in.P;
  const ChunkWork w = ph_work(work, P);
  if (int rc = chunk_work_check(w, P, work_bytes, "point_head_train_fwd")) return rc;
  SMOS_REQUIRE(!training || P > 1, "point_head_train_fwd: batch statistics need more than one point");
  PhParams q;
  if (int rc = ph_params(params, eps_mom, &q)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int64_t nchunks = w.nchunks, ngroups = w.ngroups;
  double* partial = reinterpret_cast<double*>(w.part);
  int64_t grid = 1;
  hipLaunchKernelGGL(ph_prep, dim3((kM1 * kK + 255) / 256), dim3(256), 0, s, q, in, fold);
  if (training) {
    if (int rc = chunk_grid(reinterpret_cast<const void*>(&ph_pass<1>), 0, kPhBlock, nchunks, "point_head_train z1 sums", &grid)) return rc;
    hipLaunchKernelGGL((ph_pass<1>), dim3((unsigned)grid), dim3(kPhBlock), 0, s, in, fold, nullptr, nullptr, nullptr, partial, nchunks);
    if (int rc = launch_group_sum(partial, nchunks, kColsS1, w.gsum, s, "point_head_train group sum")) return rc;
  }
  hipLaunchKernelGGL(ph_fin_stats, dim3(1), dim3(128), 0, s, 1, (int)training, w.gsum, ngroups, P, q, fold, dstat);
  if (training) {
    if (int rc = chunk_grid(reinterpret_cast<const void*>(&ph_pass<3>), 0, kPhBlock, nchunks, "point_head_train z2 sums", &grid)) return rc;
    hipLaunchKernelGGL((ph_pass<2>), dim3(1), dim3(64), 0, s, in, fold, fold + F_SH2, nullptr, nullptr, nullptr, (int64_t)1);
    hipLaunchKernelGGL((ph_pass<3>), dim3((unsigned)grid), dim3(kPhBlock), 0, s, in, fold, nullptr, nullptr, nullptr, partial, nchunks);
    if (int rc = launch_group_sum(partial, nchunks, kColsS2, w.gsum, s, "point_head_train group sum")) return rc;
  }
  hipLaunchKernelGGL(ph_fin_stats, dim3(1), dim3(128), 0, s, 2, (int)training, w.gsum, ngroups, P, q, fold, dstat);
  if (int rc = chunk_grid(reinterpret_cast<const void*>(&ph_pass<4>), 0, kPhBlock, nchunks, "point_head_train logits", &grid)) return rc;
  hipLaunchKernelGGL((ph_pass<4>), dim3((unsigned)grid), dim3(kPhBlock), 0, s, in, fold, nullptr, nullptr, logits, nullptr, nchunks);
  return check_launch("point_head_train_fwd");
}

// grads: HOST array of 11 DEVICE pointers (NULL: not wanted): d_a, d_b, d_c [B,64,N] (all three or none), dW1, dgamma1,
// dbeta1, dW2, dgamma2, dbeta2, dW3, db3
extern "C" int smos_point_head_train_bwd(const float* a, const float* b, const float* c, const int64_t* pitch, const uint32_t* masks,
                                         double scale, const float* grad_logits, int64_t B, int64_t N, int32_t training,
                                         const float* fold, void* const* grads, void* work, int64_t work_bytes,
                                         smos_stream_t stream) {
  PhIn in;
  if (int rc = ph_inputs("point_head_train_bwd", a, b, c, pitch, masks, scale, B, N, &in)) return rc;
  SMOS_REQUIRE(grad_logits && fold && grads && work, "point_head_train_bwd: null pointer");
  const int64_t P = in.P;
  const ChunkWork w = ph_work(work, P);
  if (int rc = chunk_work_check(w, P, work_bytes, "point_head_train_bwd")) return rc;
  float* dxa = (float*)grads[0];
  float* dxb = (float*)grads[1];
  float* dxc = (float*)grads[2];
  SMOS_REQUIRE((dxa && dxb && dxc) || (!dxa && !dxb && !dxc), "point_head_train_bwd: input gradients come all three or not at all");
  PhGrads o;
  o.w1 = (float*)grads[3]; o.g1 = (float*)grads[4]; o.be1 = (float*)grads[5]; o.w2 = (float*)grads[6]; o.g2 = (float*)grads[7];
  o.be2 = (float*)grads[8]; o.w3 = (float*)grads[9]; o.b3 = (float*)grads[10];
  const int need_p3 = (dxa || o.w1) ? 1 : 0;
  const int need_p2 = (o.w2 || o.g1 || o.be1 || (training && need_p3)) ? 1 : 0;
  const int need_p1 = (o.w3 || o.b3 || o.g2 || o.be2 || (training && (need_p2 || need_p3))) ? 1 : 0;
  if (!need_p1 && !need_p2 && !need_p3) return SMOS_OK;
  hipStream_t s = (hipStream_t)stream;
  const int64_t nchunks = w.nchunks, ngroups = w.ngroups;
  double* coef = static_cast<double*>(w.coef);
  char* part = w.part;
  int64_t grid = 1;
  if (need_p1) {
    if (int rc = chunk_grid(reinterpret_cast<const void*>(&ph_pass<5>), 0, kPhBlock, nchunks, "point_head_train backward pass 1", &grid)) return rc;
    hipLaunchKernelGGL((ph_pass<5>), dim3((unsigned)grid), dim3(kPhBlock), 0, s, in, fold, nullptr, grad_logits, nullptr,
                       reinterpret_cast<double*>(part), nchunks);
    if (int rc = launch_group_sum(reinterpret_cast<const double*>(part), nchunks, kColsB1, w.gsum, s, "point_head_train group sum")) return rc;
  }
  hipLaunchKernelGGL(ph_fin_b1, dim3(1), dim3(256), 0, s, need_p1, (int)training, w.gsum, ngroups, P, o, coef);
  if (need_p2) {
    if (int rc = chunk_grid(reinterpret_cast<const void*>(&ph_bwd<2>), kLds2, kPhBlock, nchunks, "point_head_train backward pass 2", &grid)) return rc;
    hipLaunchKernelGGL((ph_bwd<2>), dim3((unsigned)grid), dim3(kPhBlock), kLds2, s, in, fold, coef, grad_logits, reinterpret_cast<float*>(part),
                       nullptr, nullptr, nullptr, o.w2 ? 1 : 0, nchunks);
    if (int rc = launch_group_sum(reinterpret_cast<const float*>(part), nchunks, kColsB2, w.gsum, s, "point_head_train group sum")) return rc;
  }
  hipLaunchKernelGGL(ph_fin_b2, dim3((kColsB2 + 255) / 256), dim3(256), 0, s, need_p2, (int)training, w.gsum, ngroups, P, o, coef);
  if (need_p3) {
    if (int rc = chunk_grid(reinterpret_cast<const void*>(&ph_bwd<3>), kLds3, kPhBlock, nchunks, "point_head_train backward pass 3", &grid)) return rc;
    hipLaunchKernelGGL((ph_bwd<3>), dim3((unsigned)grid), dim3(kPhBlock), kLds3, s, in, fold, coef, grad_logits, reinterpret_cast<float*>(part),
                       dxa, dxb, dxc, o.w1 ? 1 : 0, nchunks);
    if (o.w1) {
      if (int rc = launch_group_sum(reinterpret_cast<const float*>(part), nchunks, kColsB3, w.gsum, s, "point_head_train group sum")) return rc;
      hipLaunchKernelGGL(ph_fin_b3, dim3((kColsB3 + 255) / 256), dim3(256), 0, s, w.gsum, ngroups, o.w1);
    }
  }
  return check_launch("point_head_train_bwd");
}
