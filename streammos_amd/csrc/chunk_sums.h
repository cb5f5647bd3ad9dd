// Fixed-order sums over points: the reduction layer of the fused training ops (csrc/point_mlp_train.hip,
// csrc/point_head_train.hip).  One definition: a new fused training block gets the guarantee by including
// this header.
//
// The scheme.  No float atomics anywhere.  The P points are cut into chunks of a per-op constant size (never a function
// of the grid).  Whichever block walks a chunk forms the chunk's partial sums in a fixed lane / wave / trip order and stores
// them as the chunk's row of `partial` (block_columns_store for the kernels whose four waves each hold the columns in LDS).
// group_sum then adds the rows per group of kSumGroup chunks, in chunk order, in float64, and `total` adds the groups, in
// group order, in float64.
//
// What it guarantees.  Which block walks which chunk, and how many blocks there are, decides nothing: the bits of every
// sum depend on the data alone, so two runs, two grids (chunk_grid honours the grid cap of the tests) and two devices
// of one architecture give the same bits.
//
// The work buffer (chunk_work): 4096 bytes of coefficients the backward passes hand each other | the partial rows, sized
// for the op's widest row | the group sums, sized likewise.
#pragma once
#include "smos_common.h"

namespace smos {

constexpr int kSumGroup = 64;                // chunks per first-level float64 sum
constexpr int64_t kWorkCoefBytes = 4096;     // the coefficient block in front of the partials

// xor butterfly 32 ... 1: every lane ends with the sum, formed in the same order
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// sum over the groups, in group order
__device__ __forceinline__ double total(const double* __restrict__ gsum, int64_t ngroups, int cols, int col) {
  double s = 0.0;
  for (int64_t g = 0; g < ngroups; ++g) s += gsum[g * cols + col];
  return s;
}

// A point past the end is clamped onto the last one: its loads are valid, its contributions are selected away.
struct ChunkPoint {
  bool live;
  int64_t pc;     // the point, clamped
  int64_t s, n;   // its sample and its index in the sample
};

__device__ __forceinline__ ChunkPoint chunk_point(int64_t p, int64_t P, int64_t N) {
  ChunkPoint r;
  r.live = p < P;
  r.pc = r.live ? p : P - 1;
  r.s = (int64_t)((uint32_t)r.pc / (uint32_t)N);      // P < 2^31
  r.n = r.pc - r.s * N;
  return r;
}

// The block step of a 256-thread kernel: every wave has written its columns of the chunk to red[wave]; the waves add as
// (r0 + r1) + (r2 + r3) into the chunk's partial row (up to 256 columns the loop is one guarded store; a wider row strides).
template <int COLS, int W>
__device__ __forceinline__ void block_columns_store(const double (&red)[4][W], double* __restrict__ partial, int64_t chunk, int tid) {
  static_assert(COLS <= W, "more columns than the waves hold");
  __syncthreads();
  for (int i = tid; i < COLS; i += 256) partial[chunk * COLS + i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
  __syncthreads();
}

// running_mean / running_var as nn.BatchNorm updates them: the biased variance in, the unbiased one stored
__device__ __forceinline__ void bn_running_update(float* rm, float* rv, int i, double mom, double mean, double var, int64_t P) {
  rm[i] = (float)((1.0 - mom) * (double)rm[i] + mom * mean);
  rv[i] = (float)((1.0 - mom) * (double)rv[i] + mom * (var * ((double)P / (double)(P - 1))));
}

// a float64 mean as the float pair the chain subtracts before scaling
__device__ __forceinline__ void split_hi_lo(double v, float* hi, float* lo) {
  const float h = (float)v;
  *hi = h;
  *lo = (float)(v - (double)h);
}

// Channel j of M from the group sums of [sum (v - shift) | sum (v - shift)^2]: the mean less the shift (the caller adds
// the shift) and the biased variance.
__device__ __forceinline__ void bn_stats_about_shift(const double* __restrict__ gsum, int64_t ngroups, int M, int j, int64_t P,
                                                     double* mean_less_shift, double* var) {
  const double s1 = total(gsum, ngroups, 2 * M, j) / (double)P, s2 = total(gsum, ngroups, 2 * M, M + j) / (double)P;
  const double v = s2 - s1 * s1;
  *mean_less_shift = s1;
  *var = v > 0.0 ? v : 0.0;
}

inline int64_t chunk_count(int64_t P, int chunk) { return (P + chunk - 1) / chunk; }
inline int64_t group_count(int64_t P, int chunk) { return (chunk_count(P, chunk) + kSumGroup - 1) / kSumGroup; }

// The work buffer of P points in chunks of `chunk` with partial rows of up to `row` floats; bytes < 0: P is out of range.
struct ChunkWork {
  int64_t nchunks, ngroups, bytes;
  void* coef;
  char* part;
  double* gsum;
};

inline ChunkWork chunk_work(void* work, int64_t P, int chunk, int row) {
  ChunkWork w = {0, 0, -1, nullptr, nullptr, nullptr};
  if (P < 1 || P >= (1LL << 31) - chunk) return w;
  w.nchunks = chunk_count(P, chunk);
  w.ngroups = group_count(P, chunk);
  const int64_t part_bytes = w.nchunks * row * 4;
  w.bytes = kWorkCoefBytes + part_bytes + w.ngroups * row * 8;
  w.coef = work;
  w.part = static_cast<char*>(work) + kWorkCoefBytes;
  w.gsum = reinterpret_cast<double*>(w.part + part_bytes);
  return w;
}

inline int chunk_work_check(const ChunkWork& w, int64_t P, int64_t work_bytes, const char* what) {
  SMOS_REQUIRE(w.bytes > 0 && work_bytes >= w.bytes, "%s: %lld points need %lld bytes of work space, got %lld", what, (long long)P,
               (long long)w.bytes, (long long)work_bytes);
  return SMOS_OK;
}

// grid of a kernel whose blocks stride over the chunks: the resident blocks, the chunks at most (and the test hook's cap,
// which makes a block walk several chunks)
inline int chunk_grid(const void* fn, size_t dyn_lds_bytes, int block, int64_t nchunks, const char* what, int64_t* grid) {
  KernelSetup ks;
  if (int rc = kernel_setup(fn, dyn_lds_bytes, block, &ks, what)) return rc;
  const int64_t resident = conv_grid_cap((int64_t)(ks.per_cu > 0 ? ks.per_cu : 1) * (ks.cus > 0 ? ks.cus : 1));
  *grid = nchunks < resident ? nchunks : resident;
  return SMOS_OK;
}

namespace {

// first-level sums: one thread per (group of kSumGroup chunks, column), chunks in order
template <typename T>
__global__ __launch_bounds__(256) void group_sum(const T* __restrict__ partial, int64_t nchunks, int cols, double* __restrict__ gsum) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t ngroups = (nchunks + kSumGroup - 1) / kSumGroup;
  if (i >= ngroups * cols) return;
  const int64_t grp = i / cols;
  const int col = (int)(i - grp * cols);
  const int64_t c0 = grp * kSumGroup, c1 = c0 + kSumGroup < nchunks ? c0 + kSumGroup : nchunks;
  double s = 0.0;
  for (int64_t c = c0; c < c1; ++c) s += (double)partial[c * cols + col];
  gsum[i] = s;
}

template <typename T>
int launch_group_sum(const T* partial, int64_t nchunks, int cols, double* gsum, hipStream_t s, const char* what) {
  const int64_t items = ((nchunks + kSumGroup - 1) / kSumGroup) * cols;
  hipLaunchKernelGGL((group_sum<T>), dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, partial, nchunks, cols, gsum);
  return check_launch(what);
}

}  // namespace
}  // namespace smos
