// Device-side training sample builder for gfx950.
//
// Restates what DataloadTrain.__getitem__ does per sample on the host with numpy (datasets/data_StreamMOS.py:292-364,
// datasets/utils.py:116-126,280-343): 5 scans -> 3 chained windows x 3 frames, each (window, frame) pair a *job*:
//   job = 3 w + t uses scan k = w + t
//   first alignment  inv(P_0) P_k in float64 -> float32 (Trans, always applied: the reference multiplies frame 0 by
//                    inv(P_0) P_0 as well), for w > 0 a second one, inv(P_w) P_0, on that float32 result
//   range filter     lo <= p < hi on the re-posed point, kept points compacted in order
//   resampling       slot j of the job takes kept point (r * n_valid) >> 32 of a 32-bit draw r
//   augmentation     noise (float64 add, rounded once), shift (float32), scale (float32), flips, rotation (float64 products
//                    and sum, rounded once); the five scalars are shared by the three windows, the noise is per slot
//   quantisation, point feature: emit_point of prep_point.h, the arithmetic of the validation path
//   targets          lut[word & 0xFFFF] of frame 0, one per label map; BEV label grid = integer max over the cells of
//                    frame 0 (the max-pool scatter's cell rule, smos_voxel_maxpool_fwd)
// Four launches per sample whatever the number of jobs:
//   count   (job, chunk of 1024 points) -> in-range points of the chunk; the same launch zero-fills the BEV grids
//   scan    one block per job: exclusive prefix of the chunk counts, n_valid of the job
//   compact (job, chunk) -> kept[job][base + rank] = point index, ranks from wave ballots (order preserving)
//   emit    one thread per output slot (job, j), the job uniform over a block: one 16-byte row load, one label word,
//           plane stores coalesced along N
// No load sits under a lane-dependent branch: indices are clamped and the value is selected afterwards.
// The draws are either read (words [3,T,N] uint32, noise [3,T*N,3] float64) or generated in the kernel with
// Philox4x32-10 (layout: include/smos.h); smos_train_prep_draws writes what the kernel would generate.
#include "philox.h"
#include "prep_point.h"

namespace smos {

constexpr int kTpFrames = 5;     // scans of a sample
constexpr int kTpT = 3;          // frames of a window
constexpr int kTpWindows = 3;
constexpr int kTpJobs = kTpWindows * kTpT;
constexpr int kTpChunk = 4 * kBlock;   // points of one (job, chunk) unit: four rounds of a block
constexpr int kTpMaxMaps = 4;

struct TrainArgs {
  const float* scan[kTpFrames];        // [n_k, 4]
  const uint32_t* word[kTpFrames];     // [n_k] label words
  int64_t n[kTpFrames];
  double first[kTpFrames][12];         // inv(P_0) P_k, rows 0..2
  double second[kTpWindows][12];       // inv(P_w) P_0 (w = 0 unused)
  PrepGeom g;
  int64_t n_max, nchunks, N;
  int32_t* kept;                       // [jobs, n_max]
  int32_t* chunk_count;                // [jobs, nchunks]
  int32_t* chunk_base;                 // [jobs, nchunks]
  int32_t* counts;                     // [jobs] n_valid
  // draws
  const uint32_t* words;               // [3, T, N] or null: Philox
  const double* noise;                 // [3, T*N, 3] or null
  uint32_t key[2], sample[2];
  float noise_mean, noise_std;
  // augmentation scalars of the sample
  float shift[3], scale;
  int v_flip, h_flip;
  double rot_c, rot_s;
  // labels
  const int32_t* lut;                  // [n_maps, lut_len]
  int32_t n_maps, lut_len;
  // outputs of window w
  float* xyzi[kTpWindows];             // [T, 7, N]
  float* coord[kTpWindows];            // [T, N, 3]
  float* sphere[kTpWindows];           // [T, N, 2]
  int64_t* target[kTpMaxMaps][kTpWindows];   // [N]
  int64_t* bev[kTpWindows];            // [256, 256]
  int bev_size[2];
};

struct SlotDraw {
  uint32_t r;
  double noise[3];
};

// The draws of slot j of frame t of window w (counter layout: include/smos.h).
__device__ __forceinline__ SlotDraw seeded_draw(const uint32_t (&key)[2], const uint32_t (&sample)[2], int w, int t, uint32_t j,
                                                float mean, float std) {
  const uint32_t c1 = ((uint32_t)w << 8) | (uint32_t)t;
  const Philox4 a = philox4x32_10(j, c1, sample[0], sample[1], key[0], key[1]);
  const Philox4 b = philox4x32_10(j, c1 | (1u << 16), sample[0], sample[1], key[0], key[1]);
  SlotDraw d;
  d.r = a.v[0];
  d.noise[0] = (double)__fadd_rn(__fmul_rn(box_muller_f32(a.v[2], a.v[3]), std), mean);
  d.noise[1] = (double)__fadd_rn(__fmul_rn(box_muller_f32(b.v[0], b.v[1]), std), mean);
  d.noise[2] = (double)__fadd_rn(__fmul_rn(box_muller_f32(b.v[2], b.v[3]), std), mean);
  return d;
}

// Scan row -> the point of window w in float32: one rounding per alignment.
__device__ __forceinline__ void train_align(const TrainArgs& a, int w, int k, const float4& p, float& x, float& y, float& z) {
  const double dx = p.x, dy = p.y, dz = p.z;
  x = (float)pose_row_f64(a.first[k] + 0, dx, dy, dz);
  y = (float)pose_row_f64(a.first[k] + 4, dx, dy, dz);
  z = (float)pose_row_f64(a.first[k] + 8, dx, dy, dz);
  if (w > 0) {
    const double ex = x, ey = y, ez = z;
    x = (float)pose_row_f64(a.second[w] + 0, ex, ey, ez);
    y = (float)pose_row_f64(a.second[w] + 4, ex, ey, ez);
    z = (float)pose_row_f64(a.second[w] + 8, ex, ey, ez);
  }
}

__device__ __forceinline__ bool train_in_range(const PrepGeom& g, float x, float y, float z) {
  return x >= g.lo[0] && x < g.hi[0] && y >= g.lo[1] && y < g.hi[1] && z >= g.lo[2] && z < g.hi[2];
}

// One (job, chunk) unit per trip: kWrite = false counts the in-range points of the chunk, kWrite = true writes their
// indices behind the chunk's base.  Four rounds of kBlock consecutive points; inside a round a point's rank is the number
// of kept points in front of it: lanes below it in its wave (ballot) plus the waves below (LDS).
template <bool kWrite>
__global__ __launch_bounds__(kBlock) void train_prep_compact(TrainArgs a) {
  __shared__ int wave_total[kBlock / kWave];
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  if (!kWrite) {
    // the BEV label grids start at 0 (empty cell = 0, deep_point/__init__.py:26)
    const int64_t cells = (int64_t)a.bev_size[0] * a.bev_size[1];
    for (int w = 0; w < kTpWindows; ++w)
      for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (int64_t)gridDim.x * blockDim.x) a.bev[w][i] = 0;
  }
  const int64_t units = (int64_t)kTpJobs * a.nchunks;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int job = (int)(u / a.nchunks);
    const int64_t chunk = u - (int64_t)job * a.nchunks;
    const int w = job / kTpT, k = w + job % kTpT;
    const int64_t n = a.n[k];
    const float4* __restrict__ rows = reinterpret_cast<const float4*>(a.scan[k]);
    int32_t* __restrict__ kept = a.kept + (int64_t)job * a.n_max;
    int running = kWrite ? a.chunk_base[u] : 0;
#pragma unroll 1
    for (int r = 0; r < kTpChunk / kBlock; ++r) {
      const int64_t i = chunk * kTpChunk + r * kBlock + threadIdx.x;
      const float4 p = rows[min(i, n - 1)];
      float x, y, z;
      train_align(a, w, k, p, x, y, z);
      const bool m = i < n && train_in_range(a.g, x, y, z);
      const unsigned long long b = __ballot(m);
      if (lane == 0) wave_total[wave] = __popcll(b);
      __syncthreads();
      int below = 0, total = 0;
#pragma unroll
      for (int v = 0; v < kBlock / kWave; ++v) {
        const int c = wave_total[v];
        below += v < wave ? c : 0;
        total += c;
      }
      if (kWrite && m) kept[running + below + __popcll(b & ((1ull << lane) - 1ull))] = (int32_t)i;
      running += total;
      __syncthreads();
    }
    if (!kWrite && threadIdx.x == 0) a.chunk_count[u] = running;
  }
}

// One block per job: chunk_base = exclusive prefix of chunk_count, counts[job] = their sum.
__global__ __launch_bounds__(kBlock) void train_prep_scan(TrainArgs a) {
  __shared__ int buf[2][kBlock];
  const int job = blockIdx.x;
  const int32_t* __restrict__ cnt = a.chunk_count + (int64_t)job * a.nchunks;
  int32_t* __restrict__ base = a.chunk_base + (int64_t)job * a.nchunks;
  int carry = 0;
  for (int64_t c0 = 0; c0 < a.nchunks; c0 += kBlock) {
    const int64_t c = c0 + threadIdx.x;
    const int v = cnt[min(c, a.nchunks - 1)];
    int cur = 0;
    buf[0][threadIdx.x] = c < a.nchunks ? v : 0;
    __syncthreads();
    for (int d = 1; d < kBlock; d <<= 1) {
      const int s = buf[cur][threadIdx.x] + ((int)threadIdx.x >= d ? buf[cur][threadIdx.x - d] : 0);
      buf[cur ^ 1][threadIdx.x] = s;
      cur ^= 1;
      __syncthreads();
    }
    const int incl = buf[cur][threadIdx.x];
    if (c < a.nchunks) base[c] = carry + incl - v;
    carry += buf[cur][kBlock - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) a.counts[job] = carry;
}

// One (job, block of kBlock slots) unit per trip, so that the job -- and with it the scan, the poses and the output planes -- is
// uniform over the block; a slot past N computes on slot N - 1 and stores nothing.
__global__ __launch_bounds__(kBlock) void train_prep_emit(TrainArgs a) {
  const int64_t nblk = (a.N + kBlock - 1) / kBlock;
  for (int64_t u = blockIdx.x; u < kTpJobs * nblk; u += gridDim.x) {
    const int job = (int)(u / nblk);
    const int64_t slot = (u - (int64_t)job * nblk) * kBlock + threadIdx.x;
    const bool live = slot < a.N;
    const int64_t j = min(slot, a.N - 1);
    const int64_t idx = (int64_t)job * a.N + j;
    const int w = job / kTpT, t = job - w * kTpT, k = w + t;
    const int64_t n = a.n[k];
    const uint32_t nv = (uint32_t)a.counts[job];
    SlotDraw d;
    if (a.words) {      // uniform: the whole launch reads its draws or generates them
      d.r = a.words[idx];
      d.noise[0] = a.noise[idx * 3 + 0];
      d.noise[1] = a.noise[idx * 3 + 1];
      d.noise[2] = a.noise[idx * 3 + 2];
    } else {
      d = seeded_draw(a.key, a.sample, w, t, (uint32_t)j, a.noise_mean, a.noise_std);
    }
    // choice < n_valid for every 32-bit draw; n_valid = 0 gives 0, whose entry of `kept` was never written: the row index is
    // clamped into the scan and the values are replaced below
    const int64_t choice = (int64_t)(((uint64_t)d.r * (uint64_t)nv) >> 32);
    const int64_t src = min(max((int64_t)a.kept[(int64_t)job * a.n_max + choice], (int64_t)0), n - 1);
    const float4 p = reinterpret_cast<const float4*>(a.scan[k])[src];
    const uint32_t word = a.word[k][src];
    float x, y, z;
    train_align(a, w, k, p, x, y, z);
    // DataAugmentTemp.__call__ (datasets/utils.py:280-343)
    x = (float)__dadd_rn((double)x, d.noise[0]);
    y = (float)__dadd_rn((double)y, d.noise[1]);
    z = (float)__dadd_rn((double)z, d.noise[2]);
    x = __fadd_rn(x, a.shift[0]);
    y = __fadd_rn(y, a.shift[1]);
    z = __fadd_rn(z, a.shift[2]);
    x = __fmul_rn(x, a.scale);
    y = __fmul_rn(y, a.scale);
    z = __fmul_rn(z, a.scale);
    x = a.v_flip ? -x : x;
    y = a.h_flip ? -y : y;
    const double rx = x, ry = y;
    x = (float)__dadd_rn(__dmul_rn(rx, a.rot_c), __dmul_rn(ry, a.rot_s));
    y = (float)__dsub_rn(__dmul_rn(ry, a.rot_c), __dmul_rn(rx, a.rot_s));
    float inten = p.w;
    const bool empty = nv == 0;     // the reference raises; here the frame is the validation padding point, label 0
    x = empty ? -1000.0f : x;
    y = empty ? -1000.0f : y;
    z = empty ? -4000.0f : z;
    inten = empty ? -1000.0f : inten;

    EmitArgs e;
    e.xyzi = a.xyzi[w];
    e.coord = a.coord[w];
    e.sphere = a.sphere[w];
    e.N = a.N;
    e.t = t;
    e.T = kTpT;
    e.V = 1;
    e.sx[0] = 1.0f;
    e.sy[0] = 1.0f;
    e.g = a.g;
    if (live) emit_point(e, j, x, y, z, inten);

    // labels: lut[word & 0xFFFF] (utils.relabel: an id the map does not name is 0), frame 0 of the window only
    const int sem = (int)(word & 0xFFFFu);
    const bool known = sem < a.lut_len && !empty;
    const int at = min(sem, a.lut_len - 1);
    int first = 0;
#pragma unroll
    for (int m = 0; m < kTpMaxMaps; ++m) {
      if (m < a.n_maps) {
        const int raw = a.lut[(int64_t)m * a.lut_len + at];
        const int lab = known ? raw : 0;
        if (t == 0 && live) a.target[m][w][j] = (int64_t)lab;
        if (m == 0) first = lab;
      }
    }
    // BEV label grid: the max-pool scatter's cell rule on (x_quan, y_quan) * 0.5 (csrc/voxel_maxpool.hip cell_offset);
    // labels are >= 0 and the grid starts at 0, so an integer max equals the float max of the reference
    const float qx = __fdiv_rn(__fsub_rn(x, a.g.lo[0]), a.g.cell[0]);
    const float qy = __fdiv_rn(__fsub_rn(y, a.g.lo[1]), a.g.cell[1]);
    const float px = __fmul_rn(qx, 0.5f), py = __fmul_rn(qy, 0.5f);
    const bool in = px > -1.0f && px < (float)a.bev_size[0] && py > -1.0f && py < (float)a.bev_size[1];
    if (t == 0 && live && in && first > 0)
      atomicMax(reinterpret_cast<long long*>(a.bev[w]) + (int64_t)(int)px * a.bev_size[1] + (int)py, (long long)first);
  }
}

__global__ __launch_bounds__(kBlock) void train_prep_draws(uint32_t k0, uint32_t k1, uint32_t s0, uint32_t s1, int64_t N, float mean,
                                                           float std, uint32_t* __restrict__ words, double* __restrict__ noise) {
  const uint32_t key[2] = {k0, k1}, sample[2] = {s0, s1};
  const int64_t total = (int64_t)kTpJobs * N;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int job = (int)(idx / N);
    const int64_t j = idx - (int64_t)job * N;
    const SlotDraw d = seeded_draw(key, sample, job / kTpT, job % kTpT, (uint32_t)j, mean, std);
    words[idx] = d.r;
    noise[idx * 3 + 0] = d.noise[0];
    noise[idx * 3 + 1] = d.noise[1];
    noise[idx * 3 + 2] = d.noise[2];
  }
}

static int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }
static int64_t tp_chunks(int64_t n_max) { return (n_max + kTpChunk - 1) / kTpChunk; }
constexpr int64_t kTpMaxPoints = 1LL << 30;      // per scan and per frame: every index fits an int32

}  // namespace smos

using namespace smos;

extern "C" int64_t smos_train_prep_work_bytes(int64_t n_max) {
  if (n_max < 1 || n_max > kTpMaxPoints) return -1;
  return align256(kTpJobs * n_max * 4) + 2 * align256(kTpJobs * tp_chunks(n_max) * 4);
}

extern "C" int smos_train_prep_build(const void* const* scans, const void* const* label_words, const int64_t* n, const double* first_pose,
                                     const double* second_pose, const double* range6, const int64_t* bev_size3, const double* rv4,
                                     int64_t N, const uint32_t* words, const double* noise, uint64_t seed, uint64_t sample_index,
                                     double noise_mean, double noise_std, const double* shift3, double scale, int32_t v_flip,
                                     int32_t h_flip, double rot_cos, double rot_sin, const int32_t* lut, int32_t n_maps,
                                     int32_t lut_len, void* const* xyzi, void* const* coord, void* const* sphere,
                                     void* const* targets, void* const* bev, int32_t* counts, void* work, int64_t work_bytes,
                                     smos_stream_t stream) {
  SMOS_REQUIRE(scans && label_words && n && first_pose && second_pose && range6 && bev_size3 && rv4 && shift3 && lut && xyzi &&
                   coord && sphere && targets && bev && counts && work,
               "train_prep_build: null pointer");
  SMOS_REQUIRE(N > 0 && N <= kTpMaxPoints, "train_prep_build: frame_point_num=%lld outside 1..2^30", (long long)N);
  SMOS_REQUIRE(n_maps >= 1 && n_maps <= kTpMaxMaps && lut_len >= 1, "train_prep_build: %d label maps of %d entries (1..%d maps)",
               (int)n_maps, (int)lut_len, kTpMaxMaps);
  SMOS_REQUIRE((words == nullptr) == (noise == nullptr), "train_prep_build: words and noise come together or not at all");
  SMOS_REQUIRE(bev_size3[0] > 0 && bev_size3[1] > 0 && bev_size3[0] % 2 == 0 && bev_size3[1] % 2 == 0 && bev_size3[0] < (1 << 16) &&
                   bev_size3[1] < (1 << 16),
               "train_prep_build: bad BEV shape");
  TrainArgs a;
  a.n_max = 0;
  for (int k = 0; k < kTpFrames; ++k) {
    SMOS_REQUIRE(n[k] >= 1 && n[k] <= kTpMaxPoints, "train_prep_build: scan %d has %lld points (1..2^30)", k, (long long)n[k]);
    SMOS_REQUIRE(scans[k] && label_words[k], "train_prep_build: null scan pointer");
    a.scan[k] = (const float*)scans[k];
    a.word[k] = (const uint32_t*)label_words[k];
    a.n[k] = n[k];
    if (n[k] > a.n_max) a.n_max = n[k];
    for (int i = 0; i < 12; ++i) a.first[k][i] = first_pose[16 * k + i];
  }
  for (int w = 0; w < kTpWindows; ++w)
    for (int i = 0; i < 12; ++i) a.second[w][i] = second_pose[16 * w + i];
  SMOS_REQUIRE(work_bytes >= smos_train_prep_work_bytes(a.n_max), "train_prep_build: work buffer of %lld bytes, %lld needed",
               (long long)work_bytes, (long long)smos_train_prep_work_bytes(a.n_max));
  fill_geom(a.g, range6, bev_size3, rv4);
  a.nchunks = tp_chunks(a.n_max);
  a.N = N;
  char* wp = (char*)work;
  a.kept = (int32_t*)wp;
  wp += align256(kTpJobs * a.n_max * 4);
  a.chunk_count = (int32_t*)wp;
  wp += align256(kTpJobs * a.nchunks * 4);
  a.chunk_base = (int32_t*)wp;
  a.counts = counts;
  a.words = words;
  a.noise = noise;
  a.key[0] = (uint32_t)seed;
  a.key[1] = (uint32_t)(seed >> 32);
  a.sample[0] = (uint32_t)sample_index;
  a.sample[1] = (uint32_t)(sample_index >> 32);
  a.noise_mean = (float)noise_mean;
  a.noise_std = (float)noise_std;
  for (int d = 0; d < 3; ++d) a.shift[d] = (float)shift3[d];
  a.scale = (float)scale;
  a.v_flip = v_flip ? 1 : 0;
  a.h_flip = h_flip ? 1 : 0;
  a.rot_c = rot_cos;
  a.rot_s = rot_sin;
  a.lut = lut;
  a.n_maps = n_maps;
  a.lut_len = lut_len;
  a.bev_size[0] = (int)(bev_size3[0] / 2);
  a.bev_size[1] = (int)(bev_size3[1] / 2);
  for (int w = 0; w < kTpWindows; ++w) {
    SMOS_REQUIRE(xyzi[w] && coord[w] && sphere[w] && bev[w], "train_prep_build: null output pointer");
    a.xyzi[w] = (float*)xyzi[w];
    a.coord[w] = (float*)coord[w];
    a.sphere[w] = (float*)sphere[w];
    a.bev[w] = (int64_t*)bev[w];
    for (int m = 0; m < kTpMaxMaps; ++m) {
      a.target[m][w] = m < n_maps ? (int64_t*)targets[m * kTpWindows + w] : nullptr;
      SMOS_REQUIRE(m >= n_maps || a.target[m][w], "train_prep_build: null target pointer");
    }
  }
  hipStream_t s = (hipStream_t)stream;
  const dim3 cgrid((unsigned)conv_grid_cap(grid_for(kTpJobs * a.nchunks, 1, kMaxGrid)));
  hipLaunchKernelGGL((train_prep_compact<false>), cgrid, dim3(kBlock), 0, s, a);
  hipLaunchKernelGGL(train_prep_scan, dim3(kTpJobs), dim3(kBlock), 0, s, a);
  hipLaunchKernelGGL((train_prep_compact<true>), cgrid, dim3(kBlock), 0, s, a);
  hipLaunchKernelGGL(train_prep_emit, dim3((unsigned)conv_grid_cap(grid_for(kTpJobs * ((N + kBlock - 1) / kBlock), 1, kMaxGrid))), dim3(kBlock), 0, s, a);
  return check_launch("train_prep_build");
}

extern "C" int smos_train_prep_draws(uint64_t seed, uint64_t sample_index, int64_t N, double noise_mean, double noise_std,
                                     uint32_t* words, double* noise, smos_stream_t stream) {
  SMOS_REQUIRE(N > 0 && N <= kTpMaxPoints, "train_prep_draws: frame_point_num=%lld outside 1..2^30", (long long)N);
  SMOS_REQUIRE(words && noise, "train_prep_draws: null device pointer");
  hipLaunchKernelGGL(train_prep_draws, dim3((unsigned)conv_grid_cap(grid_for(kTpJobs * N, kBlock, kMaxGrid))), dim3(kBlock), 0,
                     (hipStream_t)stream, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)sample_index,
                     (uint32_t)(sample_index >> 32), N, (float)noise_mean, (float)noise_std, words, noise);
  return check_launch("train_prep_draws");
}
