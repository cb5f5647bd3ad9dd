// Training point MLP: BN0 -> 1x1 conv 7->64 -> BN1 -> ReLU -> 1x1 conv 64->64 -> BN2 -> ReLU of
// PointNetStacker(7, 64, pre_bn=True, stack_num=2) as one forward and one backward entry, batch statistics included.
//
// Nothing but x is kept between the passes: every pass recomputes the chain from x (7 floats per point) with the batch
// statistics folded into a small parameter block ("fold") that the finalize kernels leave on the device.
//
//   forward, training   x sums -> mean0 | centred 7x7 second moments of x -> BN0 and (z1 is linear in x) BN1 statistics |
//                       z2 sums about a shift -> BN2 statistics | y
//   forward, eval       fold the running statistics | y
//   backward            pass 1: dbeta2, dgamma2 | pass 2: dW2 = sum dz2 (x) h1 and M = sum da1 (x) (x - mu0, 1), from which
//                       dbeta1, dgamma1, dW1, dgamma0, dbeta0 follow in closed form (everything is linear in the statistics)
//
// Arithmetic: fp32 FMA chains on the vector unit, one point per lane, the weights wave-uniform (scalar loads).  gfx950's
// fp32-input MFMA runs at the vector rate, so the matrix pipe would buy layout, not throughput; the reductions over points
// are what shapes these kernels.
//
// Reductions: the fixed-order sums of csrc/chunk_sums.h over chunks of kPmChunk = 512 points; the bits of every output
// depend on the data alone.
//
// Accuracy: means are taken about a shift (x: the first point; z2: the mean of the first chunk) and variances about the
// mean (x) or the shift (z2) with the correction done in float64, so a channel with mean 1000 and spread 0.01 keeps its
// variance.  In the chain a mean is subtracted as a float pair (hi, lo) BEFORE scaling: folding it into a bias would round
// at the magnitude of the mean.
#include "chunk_sums.h"

namespace smos {
namespace {

constexpr int kPmChunk = 512;                // points per chunk of partial sums
constexpr int kPmRow = 68;                   // LDS row pitch in floats (16-byte rows, 4-bank skew)
constexpr int kPmCols2 = 64 * 64 + 64 * 8;   // backward pass 2: dW2, then M[j][0..6] and dbeta1 at [j][7]

// the folded parameter block (floats)
enum : int {
  F_MU0H = 0, F_MU0L = 8,          // mean of x as a float pair
  F_Z1 = 16,                       // [64][8]  r1 W1 a0  (zhat1 = Z1 d + ZC1; column 7 is zero)
  F_ZC1 = 528, F_GAM1 = 592, F_BET1 = 656,
  F_W2 = 720,                      // [j][k]
  F_W2T = 4816,                    // [k][j]
  F_MU2H = 8912, F_MU2L = 8976, F_G2 = 9040, F_BET2 = 9104, F_R2 = 9168, F_SH2 = 9232,
  F_END = 9296
};
// the float64 statistics the backward's closed forms need
enum : int { D_MU0 = 0, D_A0 = 8, D_R0 = 16, D_COV = 24, D_R1 = 88, D_R2 = 152, D_MU1 = 216, D_END = 280 };
// work buffer: the coefficients are 128 floats, dbeta2 / P and dgamma2 / P
struct PmPoint {
  bool live;
  int64_t xoff;   // x + xoff: channel 0 of the point; channels are N apart
  int64_t yoff;   // y + yoff likewise
};

__device__ __forceinline__ PmPoint pm_point(int64_t p, int64_t P, int64_t N) {
  const ChunkPoint c = chunk_point(p, P, N);
  return {c.live, c.s * 7 * N + c.n, c.s * 64 * N + c.n};
}

__device__ __forceinline__ void pm_load_d(const float* __restrict__ x, const float* __restrict__ fold, int64_t xoff, int64_t N,
                                          float (&d)[7]) {
#pragma unroll
  for (int c = 0; c < 7; ++c) d[c] = (x[xoff + c * N] - fold[F_MU0H + c]) - fold[F_MU0L + c];
}

__device__ __forceinline__ float pm_zhat1(const float* __restrict__ fold, const float (&d)[7], int j) {
  float z = fold[F_ZC1 + j];
#pragma unroll
  for (int c = 0; c < 7; ++c) z = fmaf(fold[F_Z1 + j * 8 + c], d[c], z);
  return z;
}

__device__ __forceinline__ void pm_h1(const float* __restrict__ fold, const float (&d)[7], float (&h)[64]) {
#pragma unroll
  for (int j = 0; j < 64; ++j) h[j] = fmaxf(fmaf(fold[F_GAM1 + j], pm_zhat1(fold, d, j), fold[F_BET1 + j]), 0.0f);
}

__device__ __forceinline__ float pm_z2(const float* __restrict__ fold, const float (&h)[64], int j) {
  float z = 0.0f;
#pragma unroll
  for (int k = 0; k < 64; ++k) z = fmaf(fold[F_W2 + j * 64 + k], h[k], z);
  return z;
}

// ---------------------------------------------------------------------------------------------------------------------
// statistics of x
__global__ __launch_bounds__(256) void pm_xsum(const float* __restrict__ x, int64_t P, int64_t N, int64_t nchunks,
                                               double* __restrict__ partial) {
  __shared__ double red[4][8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double k0[7];
#pragma unroll
  for (int c = 0; c < 7; ++c) k0[c] = (double)x[c * N];
  for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    double acc[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int t = 0; t < kPmChunk / 256; ++t) {
      const PmPoint pt = pm_point(chunk * kPmChunk + t * 256 + tid, P, N);
#pragma unroll
      for (int c = 0; c < 7; ++c) {
        const double v = (double)x[pt.xoff + c * N] - k0[c];
        acc[c] += pt.live ? v : 0.0;
      }
    }
#pragma unroll
    for (int c = 0; c < 7; ++c) acc[c] = wave_sum(acc[c]);
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < 7; ++c) red[wave][c] = acc[c];
      red[wave][7] = 0.0;
    }
    block_columns_store<8>(red, partial, chunk, tid);
  }
}

__global__ __launch_bounds__(256) void pm_xcov(const float* __restrict__ x, const double* __restrict__ dstat, int64_t P, int64_t N,
                                               int64_t nchunks, double* __restrict__ partial) {
  __shared__ double red[4][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double mu[7];
#pragma unroll
  for (int c = 0; c < 7; ++c) mu[c] = dstat[D_MU0 + c];
  for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    double acc[28];
#pragma unroll
    for (int i = 0; i < 28; ++i) acc[i] = 0.0;
    for (int t = 0; t < kPmChunk / 256; ++t) {
      const PmPoint pt = pm_point(chunk * kPmChunk + t * 256 + tid, P, N);
      double d[7];
#pragma unroll
      for (int c = 0; c < 7; ++c) d[c] = pt.live ? (double)x[pt.xoff + c * N] - mu[c] : 0.0;
      int i = 0;
#pragma unroll
      for (int a = 0; a < 7; ++a)
#pragma unroll
        for (int b = a; b < 7; ++b) acc[i++] += d[a] * d[b];
    }
    red[wave][lane] = 0.0;
    int i = 0;
#pragma unroll
    for (int a = 0; a < 7; ++a)
#pragma unroll
      for (int b = a; b < 7; ++b) {
        const double s = wave_sum(acc[i++]);
        if (lane == 0) {
          red[wave][a * 8 + b] = s;
          red[wave][b * 8 + a] = s;
        }
      }
    block_columns_store<64>(red, partial, chunk, tid);
  }
}

__global__ void pm_fin_mean0(const double* __restrict__ gsum, int64_t ngroups, const float* __restrict__ x, int64_t N, int64_t P,
                             double* __restrict__ dstat) {
  const int c = threadIdx.x;
  if (c < 8) dstat[D_MU0 + c] = c < 7 ? (double)x[c * N] + total(gsum, ngroups, 8, c) / (double)P : 0.0;
}

struct PmParams {
  const float* g0; const float* b0; float* rm0; float* rv0;
  const float* w1; const float* g1; const float* b1; float* rm1; float* rv1;
  const float* w2; const float* g2; const float* b2; float* rm2; float* rv2;
  double eps[3], mom[3];
};

// BN0 and BN1 statistics (training: from the centred second moments of x; eval: the running buffers), layer 1 folded
__global__ __launch_bounds__(256) void pm_fin_l1(int training, const double* __restrict__ gsum, int64_t ngroups, int64_t P, PmParams q,
                                                 float* __restrict__ fold, double* __restrict__ dstat) {
  __shared__ double cov[64], a0[8];
  const int tid = threadIdx.x;
  if (tid < 64) cov[tid] = training ? total(gsum, ngroups, 64, tid) / (double)P : 0.0;
  __syncthreads();
  if (tid < 8) {
    const int c = tid;
    double mu = 0.0, a = 0.0, r = 0.0;
    if (c < 7) {
      double var;
      if (training) {
        mu = dstat[D_MU0 + c];
        var = cov[c * 8 + c];
        bn_running_update(q.rm0, q.rv0, c, q.mom[0], mu, var, P);
      } else {
        mu = (double)q.rm0[c];
        var = (double)q.rv0[c];
        dstat[D_MU0 + c] = mu;
      }
      r = 1.0 / sqrt(var + q.eps[0]);
      a = (double)q.g0[c] * r;
    }
    split_hi_lo(mu, &fold[F_MU0H + c], &fold[F_MU0L + c]);
    a0[c] = a;
    dstat[D_A0 + c] = a;
    dstat[D_R0 + c] = r;
  }
  __syncthreads();
  if (tid < 64) {
    const int j = tid;
    double u[7], m1 = 0.0;
#pragma unroll
    for (int c = 0; c < 7; ++c) {
      u[c] = (double)q.w1[j * 7 + c] * a0[c];
      m1 += (double)q.w1[j * 7 + c] * (double)q.b0[c];
    }
    double mu1, var1;
    if (training) {
      mu1 = m1;           // the mean of xhat0 is beta0 exactly
      var1 = 0.0;
      for (int a = 0; a < 7; ++a)
        for (int b = 0; b < 7; ++b) var1 += u[a] * cov[a * 8 + b] * u[b];
      var1 = var1 > 0.0 ? var1 : 0.0;
      bn_running_update(q.rm1, q.rv1, j, q.mom[1], mu1, var1, P);
    } else {
      mu1 = (double)q.rm1[j];
      var1 = (double)q.rv1[j];
    }
    const double r1 = 1.0 / sqrt(var1 + q.eps[1]);
#pragma unroll
    for (int c = 0; c < 7; ++c) fold[F_Z1 + j * 8 + c] = (float)(r1 * u[c]);
    fold[F_Z1 + j * 8 + 7] = 0.0f;
    fold[F_ZC1 + j] = (float)(r1 * (m1 - mu1));
    fold[F_GAM1 + j] = q.g1[j];
    fold[F_BET1 + j] = q.b1[j];
    fold[F_SH2 + j] = 0.0f;
    dstat[D_R1 + j] = r1;
    dstat[D_MU1 + j] = mu1;
    dstat[D_COV + j] = cov[j];
  }
  for (int i = tid; i < 4096; i += 256) {
    const float w = q.w2[i];
    fold[F_W2 + i] = w;
    fold[F_W2T + (i & 63) * 64 + (i >> 6)] = w;
  }
}

__global__ void pm_fin_shift(const double* __restrict__ partial, int64_t nfirst, float* __restrict__ fold) {
  const int j = threadIdx.x;
  if (j < 64) fold[F_SH2 + j] = (float)(partial[j] / (double)nfirst);
}

__global__ void pm_fin_l2(int training, const double* __restrict__ gsum, int64_t ngroups, int64_t P, PmParams q,
                          float* __restrict__ fold, double* __restrict__ dstat) {
  const int j = threadIdx.x;
  if (j >= 64) return;
  double mu, var;
  if (training) {
    bn_stats_about_shift(gsum, ngroups, 64, j, P, &mu, &var);
    mu += (double)fold[F_SH2 + j];
    bn_running_update(q.rm2, q.rv2, j, q.mom[2], mu, var, P);
  } else {
    mu = (double)q.rm2[j];
    var = (double)q.rv2[j];
  }
  const double r2 = 1.0 / sqrt(var + q.eps[2]);
  split_hi_lo(mu, &fold[F_MU2H + j], &fold[F_MU2L + j]);
  fold[F_G2 + j] = (float)((double)q.g2[j] * r2);
  fold[F_BET2 + j] = q.b2[j];
  fold[F_R2 + j] = (float)r2;
  dstat[D_R2 + j] = r2;
}

// ---------------------------------------------------------------------------------------------------------------------
// One point per lane through the chain; per output channel j either two sums over the points (lane j of every wave keeps
// channel j's float64 accumulators for the chunk) or the store of y.
//   MODE 0  sum (z2 - shift), sum (z2 - shift)^2          MODE 1  y          MODE 2  sum da2, sum da2 zhat2
template <int MODE>
__global__ __launch_bounds__(256) void pm_pass(const float* __restrict__ x, const float* __restrict__ fold, const float* __restrict__ g,
                                               float* __restrict__ y, double* __restrict__ partial, int64_t P, int64_t N, int64_t nchunks) {
  __shared__ double red[4][128];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    double acc1 = 0.0, acc2 = 0.0;
    for (int t = 0; t < kPmChunk / 256; ++t) {
      const int64_t tile0 = chunk * kPmChunk + t * 256;
      if (tile0 >= P) break;
      const PmPoint pt = pm_point(tile0 + tid, P, N);
      float d[7], h[64];
      pm_load_d(x, fold, pt.xoff, N, d);
      pm_h1(fold, d, h);
#pragma unroll 2
      for (int j = 0; j < 64; ++j) {
        const float z = pm_z2(fold, h, j);
        if (MODE == 0) {
          const float v = pt.live ? z - fold[F_SH2 + j] : 0.0f;
          const float s1 = wave_sum(v), s2 = wave_sum(v * v);
          acc1 += lane == j ? (double)s1 : 0.0;
          acc2 += lane == j ? (double)s2 : 0.0;
        } else {
          const float c = (z - fold[F_MU2H + j]) - fold[F_MU2L + j];
          const float pre = fmaf(fold[F_G2 + j], c, fold[F_BET2 + j]);
          if (MODE == 1) {
            if (pt.live) y[pt.yoff + j * N] = fmaxf(pre, 0.0f);
          } else {
            const float gv = g[pt.yoff + j * N];
            const float da = (pt.live && pre > 0.0f) ? gv : 0.0f;
            const float s1 = wave_sum(da), s2 = wave_sum(da * (c * fold[F_R2 + j]));
            acc1 += lane == j ? (double)s1 : 0.0;
            acc2 += lane == j ? (double)s2 : 0.0;
          }
        }
      }
    }
    if (MODE != 1) {
      red[wave][lane] = acc1;
      red[wave][64 + lane] = acc2;
      block_columns_store<128>(red, partial, chunk, tid);
    }
  }
}

__global__ void pm_fin_bwd1(int have, int training, const double* __restrict__ gsum, int64_t ngroups, int64_t P, float* __restrict__ d_g2,
                            float* __restrict__ d_b2, float* __restrict__ coef) {
  const int j = threadIdx.x;
  if (j >= 64) return;
  const double db = have ? total(gsum, ngroups, 128, j) : 0.0, dg = have ? total(gsum, ngroups, 128, 64 + j) : 0.0;
  if (d_b2) d_b2[j] = (float)db;
  if (d_g2) d_g2[j] = (float)dg;
  coef[j] = training ? (float)(db / (double)P) : 0.0f;
  coef[64 + j] = training ? (float)(dg / (double)P) : 0.0f;
}

// Backward pass 2, one wave per block, 64 points per trip, 8 trips per chunk.  dz2 and h1 of the trip go to LDS point-major;
// the 64x64 sum dz2 (x) h1 is an 8x8 register tile per lane over the 64 points; each lane then takes its own dz2 row back,
// forms da1 = (W2^T dz2) [h1 > 0] into the dz2 buffer, and lane j sums da1[j] (x) (d, 1).  Sums run in fp32 over a trip
// and the trips add in fp32 into the chunk's partial (512 points), stored as float and summed in float64 from there on.
__global__ __launch_bounds__(64) void pm_bwd2(const float* __restrict__ x, const float* __restrict__ fold, const float* __restrict__ coef,
                                              const float* __restrict__ g, int64_t P, int64_t N, int64_t nchunks,
                                              float* __restrict__ partial, int need_w2, int need_low) {
  __shared__ __attribute__((aligned(16))) float s_dz[64 * kPmRow];
  __shared__ __attribute__((aligned(16))) float s_h[64 * kPmRow];
  __shared__ __attribute__((aligned(16))) float s_dx[64 * 8];
  const int lane = threadIdx.x, jb = lane >> 3, kb = lane & 7;
  for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    float cw[8][8], cm[8];
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      cm[a] = 0.0f;
#pragma unroll
      for (int b = 0; b < 8; ++b) cw[a][b] = 0.0f;
    }
    for (int t = 0; t < kPmChunk / 64; ++t) {
      const int64_t tile0 = chunk * kPmChunk + t * 64;
      if (tile0 >= P) break;
      const PmPoint pt = pm_point(tile0 + lane, P, N);
      {
        float d[7], h[64];
        pm_load_d(x, fold, pt.xoff, N, d);
        *reinterpret_cast<float4*>(&s_dx[lane * 8]) = make_float4(d[0], d[1], d[2], d[3]);
        *reinterpret_cast<float4*>(&s_dx[lane * 8 + 4]) = make_float4(d[4], d[5], d[6], 1.0f);
        pm_h1(fold, d, h);
#pragma unroll
        for (int k = 0; k < 64; k += 4)
          *reinterpret_cast<float4*>(&s_h[lane * kPmRow + k]) = make_float4(h[k], h[k + 1], h[k + 2], h[k + 3]);
#pragma unroll 2
        for (int j = 0; j < 64; ++j) {
          const float z = pm_z2(fold, h, j);
          const float c = (z - fold[F_MU2H + j]) - fold[F_MU2L + j];
          const float pre = fmaf(fold[F_G2 + j], c, fold[F_BET2 + j]);
          const float gv = g[pt.yoff + j * N];
          const float da = pre > 0.0f ? gv : 0.0f;
          const float dz = fold[F_G2 + j] * ((da - coef[j]) - (c * fold[F_R2 + j]) * coef[64 + j]);
          s_dz[lane * kPmRow + j] = pt.live ? dz : 0.0f;
        }
      }
      __syncthreads();
      if (need_w2) {
        float tw[8][8];
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
          for (int b = 0; b < 8; ++b) tw[a][b] = 0.0f;
#pragma unroll 2
        for (int p = 0; p < 64; ++p) {
          const float4 a0 = *reinterpret_cast<const float4*>(&s_dz[p * kPmRow + jb * 8]);
          const float4 a1 = *reinterpret_cast<const float4*>(&s_dz[p * kPmRow + jb * 8 + 4]);
          const float4 b0 = *reinterpret_cast<const float4*>(&s_h[p * kPmRow + kb * 8]);
          const float4 b1 = *reinterpret_cast<const float4*>(&s_h[p * kPmRow + kb * 8 + 4]);
          const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
          const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
          for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int b = 0; b < 8; ++b) tw[a][b] = fmaf(av[a], bv[b], tw[a][b]);
        }
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
          for (int b = 0; b < 8; ++b) cw[a][b] += tw[a][b];
      }
      if (need_low) {
        float dzr[64];
#pragma unroll
        for (int k = 0; k < 64; k += 4) {
          const float4 v = *reinterpret_cast<const float4*>(&s_dz[lane * kPmRow + k]);
          dzr[k] = v.x; dzr[k + 1] = v.y; dzr[k + 2] = v.z; dzr[k + 3] = v.w;
        }
        __syncthreads();      // every row is in registers and the dW2 tile is done: the buffer now takes da1
#pragma unroll 2
        for (int k = 0; k < 64; ++k) {
          float dh = 0.0f;
#pragma unroll
          for (int j = 0; j < 64; ++j) dh = fmaf(fold[F_W2T + k * 64 + j], dzr[j], dh);
          const float hk = s_h[lane * kPmRow + k];
          s_dz[lane * kPmRow + k] = hk > 0.0f ? dh : 0.0f;
        }
        __syncthreads();
        float tm[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int p = 0; p < 64; ++p) {
          const float a = s_dz[p * kPmRow + lane];
          const float4 b0 = *reinterpret_cast<const float4*>(&s_dx[p * 8]);
          const float4 b1 = *reinterpret_cast<const float4*>(&s_dx[p * 8 + 4]);
          const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
          for (int c = 0; c < 8; ++c) tm[c] = fmaf(a, bv[c], tm[c]);
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) cm[c] += tm[c];
      }
      __syncthreads();
    }
    float* out = partial + chunk * kPmCols2;
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      float* row = out + (jb * 8 + a) * 64 + kb * 8;
      *reinterpret_cast<float4*>(row) = make_float4(cw[a][0], cw[a][1], cw[a][2], cw[a][3]);
      *reinterpret_cast<float4*>(row + 4) = make_float4(cw[a][4], cw[a][5], cw[a][6], cw[a][7]);
    }
    *reinterpret_cast<float4*>(out + 4096 + lane * 8) = make_float4(cm[0], cm[1], cm[2], cm[3]);
    *reinterpret_cast<float4*>(out + 4096 + lane * 8 + 4) = make_float4(cm[4], cm[5], cm[6], cm[7]);
  }
}

struct PmGrads {
  float* g0; float* b0; float* w1; float* g1; float* b1; float* w2;
};

// The closed forms of the header, in float64.  M[j][c] = sum_p da1[j] d[c], dbeta1 = M[j][7];
//   dgamma1[j] = sum_c Z1[j][c] M[j][c] + ZC1[j] dbeta1[j]
//   D[j][c] = sum_p dz1[j] d[c] = gamma1 r1 (M[j][c] - t dgamma1[j] r1[j] sum_c' W1[j][c'] a0[c'] cov[c'][c])
//   sum_p dz1[j] = (1 - t) gamma1 r1 dbeta1          (t = 1 in training, 0 in eval)
//   dW1[j][c] = a0[c] D[j][c] + beta0[c] sum_p dz1[j];  dgamma0[c] = r0[c] sum_j W1[j][c] D[j][c];  dbeta0[c] = sum_j W1[j][c] sum_p dz1[j]
__global__ __launch_bounds__(256) void pm_fin_bwd2(int training, const double* __restrict__ gsum, int64_t ngroups, PmParams q,
                                                   const double* __restrict__ dstat, PmGrads o, int need_low) {
  __shared__ double Dm[64 * 8], sdz1[64];
  const int tid = threadIdx.x;
  if (o.w2)
    for (int i = tid; i < 4096; i += 256) o.w2[i] = (float)total(gsum, ngroups, kPmCols2, i);
  if (!need_low) return;
  if (tid < 64) {
    const int j = tid;
    double M[8], u[7], m1 = 0.0;
    for (int c = 0; c < 8; ++c) M[c] = total(gsum, ngroups, kPmCols2, 4096 + j * 8 + c);
    for (int c = 0; c < 7; ++c) {
      u[c] = (double)q.w1[j * 7 + c] * dstat[D_A0 + c];
      m1 += (double)q.w1[j * 7 + c] * (double)q.b0[c];
    }
    const double r1 = dstat[D_R1 + j], db1 = M[7];
    double dg1 = r1 * (m1 - dstat[D_MU1 + j]) * db1;
    for (int c = 0; c < 7; ++c) dg1 += r1 * u[c] * M[c];
    const double gr = (double)q.g1[j] * r1;
    for (int c = 0; c < 7; ++c) {
      double corr = 0.0;
      if (training) {
        double s = 0.0;
        for (int e = 0; e < 7; ++e) s += u[e] * dstat[D_COV + e * 8 + c];
        corr = dg1 * r1 * s;
      }
      Dm[j * 8 + c] = gr * (M[c] - corr);
    }
    sdz1[j] = training ? 0.0 : gr * db1;
    if (o.b1) o.b1[j] = (float)db1;
    if (o.g1) o.g1[j] = (float)dg1;
    if (o.w1)
      for (int c = 0; c < 7; ++c) o.w1[j * 7 + c] = (float)(dstat[D_A0 + c] * Dm[j * 8 + c] + (double)q.b0[c] * sdz1[j]);
  }
  __syncthreads();
  if (tid < 7) {
    const int c = tid;
    double dg0 = 0.0, db0 = 0.0;
    for (int j = 0; j < 64; ++j) {
      dg0 += (double)q.w1[j * 7 + c] * Dm[j * 8 + c];
      db0 += (double)q.w1[j * 7 + c] * sdz1[j];
    }
    if (o.g0) o.g0[c] = (float)(dstat[D_R0 + c] * dg0);
    if (o.b0) o.b0[c] = (float)db0;
  }
}

// the widest partial row is pass 2 of the backward
ChunkWork pm_work(void* work, int64_t P) { return chunk_work(work, P, kPmChunk, kPmCols2); }

int pm_params(const void* const* p, const double* eps_mom, PmParams* q) {
  for (int i = 0; i < 14; ++i) SMOS_REQUIRE(p[i], "point_mlp: null parameter pointer %d", i);
  q->g0 = (const float*)p[0]; q->b0 = (const float*)p[1]; q->rm0 = (float*)p[2]; q->rv0 = (float*)p[3];
  q->w1 = (const float*)p[4]; q->g1 = (const float*)p[5]; q->b1 = (const float*)p[6]; q->rm1 = (float*)p[7]; q->rv1 = (float*)p[8];
  q->w2 = (const float*)p[9]; q->g2 = (const float*)p[10]; q->b2 = (const float*)p[11]; q->rm2 = (float*)p[12]; q->rv2 = (float*)p[13];
  for (int i = 0; i < 3; ++i) {
    q->eps[i] = eps_mom[i];
    q->mom[i] = eps_mom[3 + i];
  }
  return SMOS_OK;
}

}  // namespace
}  // namespace smos

using namespace smos;

extern "C" int32_t smos_point_mlp_chunk(void) { return kPmChunk; }
extern "C" int32_t smos_point_mlp_fold_floats(void) { return F_END; }
extern "C" int32_t smos_point_mlp_stat_doubles(void) { return D_END; }

extern "C" int64_t smos_point_mlp_work_bytes(int64_t P) {
  return pm_work(nullptr, P).bytes;
}

extern "C" int smos_point_mlp_fwd(const float* x, int64_t S, int64_t N, int32_t training, const void* const* params,
                                  const double* eps_mom, float* y, float* fold, double* dstat, void* work, int64_t work_bytes,
                                  smos_stream_t stream) {
  SMOS_REQUIRE(x && params && eps_mom && y && fold && dstat && work, "point_mlp_fwd: null pointer");
  SMOS_REQUIRE(S > 0 && N > 0, "point_mlp_fwd: bad sizes");
  const int64_t P = S * N;
  const ChunkWork w = pm_work(work, P);
  if (int rc = chunk_work_check(w, P, work_bytes, "point_mlp_fwd")) return rc;
  SMOS_REQUIRE(!training || P > 1, "point_mlp_fwd: batch statistics need more than one point");
  PmParams q;
  if (int rc = pm_params(params, eps_mom, &q)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int64_t nchunks = w.nchunks, ngroups = w.ngroups;
  double* partial = reinterpret_cast<double*>(w.part);
  int64_t grid = 1;
  if (training) {
    if (int rc = chunk_grid(reinterpret_cast<const void*>(&pm_xsum), 0, 256, nchunks, "point_mlp x sums", &grid)) return rc;
    hipLaunchKernelGGL(pm_xsum, dim3((unsigned)grid), dim3(256), 0, s, x, P, N, nchunks, partial);
    if (int rc = launch_group_sum(partial, nchunks, 8, w.gsum, s, "point_mlp group sum")) return rc;
    hipLaunchKernelGGL(pm_fin_mean0, dim3(1), dim3(64), 0, s, w.gsum, ngroups, x, N, P, dstat);
    if (int rc = chunk_grid(reinterpret_cast<const void*>(&pm_xcov), 0, 256, nchunks, "point_mlp x moments", &grid)) return rc;
    hipLaunchKernelGGL(pm_xcov, dim3((unsigned)grid), dim3(256), 0, s, x, dstat, P, N, nchunks, partial);
    if (int rc = launch_group_sum(partial, nchunks, 64, w.gsum, s, "point_mlp group sum")) return rc;
  }
  hipLaunchKernelGGL(pm_fin_l1, dim3(1), dim3(256), 0, s, (int)training, w.gsum, ngroups, P, q, fold, dstat);
  if (training) {
    if (int rc = chunk_grid(reinterpret_cast<const void*>(&pm_pass<0>), 0, 256, nchunks, "point_mlp z2 sums", &grid)) return rc;
    // the shift: the mean of z2 over the first chunk
    hipLaunchKernelGGL((pm_pass<0>), dim3(1), dim3(256), 0, s, x, fold, nullptr, nullptr, partial, P, N, (int64_t)1);
    hipLaunchKernelGGL(pm_fin_shift, dim3(1), dim3(64), 0, s, partial, P < kPmChunk ? P : (int64_t)kPmChunk, fold);
    hipLaunchKernelGGL((pm_pass<0>), dim3((unsigned)grid), dim3(256), 0, s, x, fold, nullptr, nullptr, partial, P, N, nchunks);
    if (int rc = launch_group_sum(partial, nchunks, 128, w.gsum, s, "point_mlp group sum")) return rc;
  }
  hipLaunchKernelGGL(pm_fin_l2, dim3(1), dim3(64), 0, s, (int)training, w.gsum, ngroups, P, q, fold, dstat);
  if (int rc = chunk_grid(reinterpret_cast<const void*>(&pm_pass<1>), 0, 256, nchunks, "point_mlp y", &grid)) return rc;
  hipLaunchKernelGGL((pm_pass<1>), dim3((unsigned)grid), dim3(256), 0, s, x, fold, nullptr, y, nullptr, P, N, nchunks);
  return check_launch("point_mlp_fwd");
}

extern "C" int smos_point_mlp_bwd(const float* x, const float* grad_y, int64_t S, int64_t N, int32_t training,
                                  const void* const* params, const double* eps_mom, const float* fold, const double* dstat,
                                  void* const* grads, void* work, int64_t work_bytes, smos_stream_t stream) {
  SMOS_REQUIRE(x && grad_y && params && eps_mom && fold && dstat && grads && work, "point_mlp_bwd: null pointer");
  SMOS_REQUIRE(S > 0 && N > 0, "point_mlp_bwd: bad sizes");
  const int64_t P = S * N;
  const ChunkWork w = pm_work(work, P);
  if (int rc = chunk_work_check(w, P, work_bytes, "point_mlp_bwd")) return rc;
  PmParams q;
  if (int rc = pm_params(params, eps_mom, &q)) return rc;
  // grads: gamma0, beta0, W1, gamma1, beta1, W2, gamma2, beta2 (NULL: not wanted)
  PmGrads o;
  o.g0 = (float*)grads[0]; o.b0 = (float*)grads[1]; o.w1 = (float*)grads[2]; o.g1 = (float*)grads[3]; o.b1 = (float*)grads[4];
  o.w2 = (float*)grads[5];
  float* d_g2 = (float*)grads[6];
  float* d_b2 = (float*)grads[7];
  const int need_low = (o.g0 || o.b0 || o.w1 || o.g1 || o.b1) ? 1 : 0, need_w2 = o.w2 ? 1 : 0;
  const int need_p2 = need_low || need_w2, need_p1 = (d_g2 || d_b2 || (training && need_p2)) ? 1 : 0;
  if (!need_p1 && !need_p2) return SMOS_OK;
  hipStream_t s = (hipStream_t)stream;
  const int64_t nchunks = w.nchunks, ngroups = w.ngroups;
  float* coef = static_cast<float*>(w.coef);
  char* part = w.part;
  int64_t grid = 1;
  if (need_p1) {
    if (int rc = chunk_grid(reinterpret_cast<const void*>(&pm_pass<2>), 0, 256, nchunks, "point_mlp backward pass 1", &grid)) return rc;
    hipLaunchKernelGGL((pm_pass<2>), dim3((unsigned)grid), dim3(256), 0, s, x, fold, grad_y, nullptr, reinterpret_cast<double*>(part), P, N,
                       nchunks);
    if (int rc = launch_group_sum(reinterpret_cast<const double*>(part), nchunks, 128, w.gsum, s, "point_mlp group sum")) return rc;
  }
  hipLaunchKernelGGL(pm_fin_bwd1, dim3(1), dim3(64), 0, s, need_p1, (int)training, w.gsum, ngroups, P, d_g2, d_b2, coef);
  if (need_p2) {
    if (int rc = chunk_grid(reinterpret_cast<const void*>(&pm_bwd2), 0, 64, nchunks, "point_mlp backward pass 2", &grid)) return rc;
    hipLaunchKernelGGL(pm_bwd2, dim3((unsigned)grid), dim3(64), 0, s, x, fold, coef, grad_y, P, N, nchunks, reinterpret_cast<float*>(part),
                       need_w2, need_low);
    if (int rc = launch_group_sum(reinterpret_cast<const float*>(part), nchunks, kPmCols2, w.gsum, s, "point_mlp group sum")) return rc;
    hipLaunchKernelGGL(pm_fin_bwd2, dim3(1), dim3(256), 0, s, (int)training, w.gsum, ngroups, q, dstat, o, need_low);
  }
  return check_launch("point_mlp_bwd");
}
