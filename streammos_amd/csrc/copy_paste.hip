// Copy-paste augmentation on the device for gfx950: SequenceCutPaste of datasets/copy_paste.py /
// copy_paste_seg.py on the five first-aligned scans of a training sample.  Host restatement: preprocess.copy_paste_sample.
//
// State of a sample (one flat array each, frame k owns rows off[k] .. off[k] + n_k + M, M = the points of all objects):
//   pts [rows, 4] float32, word [rows] uint32, ang [rows, 2] = (phi, theta) float32, flag [rows] uint8 (bit 0 alive, bit 1
//   object class: raw id in [10, 33) or [252, 260), or a pasted point, raw id 30).
// Frame k's rows are its n_k scan points in their order, then one slot range per object in paste order.  A removed point and a
// slot nothing was pasted into hold the validation padding point: the half-open range filter of train_prep_compact drops it,
// and its order-preserving compaction then yields the array the reference resamples from.
//
// Launches: one per sample (init: first alignment, angles, flags, padded slots), four per object whatever its size:
//   road   (chunk of 1024 points of scan 0) x 20 candidates -> count and float64 sum of the road heights under the footprint
//   prep   one block per candidate j = trial j: road mean of trials 0..j, the z chain over the road-passing trials before it,
//          the j + 1 accumulated rotations of every point, the five view boxes
//   count  (frame, chunk of rows) x 20 boxes of that frame -> object-class points inside, integer atomics
//   apply  every block picks the first valid candidate; rows inside its boxes are removed, the object's rows written
// A candidate replays its own chain, so no launch waits on another block and nothing is read back.  Every partial result
// belongs to a fixed chunk, so the bits do not depend on the grid.  Road points come from the raw scan 0 (re-aligned: same
// bits), which no paste edits: the reference takes its road list once, before any paste.
// No load sits under a lane-dependent branch: indices are clamped and values selected afterwards; a frame, a candidate and
// with them the boxes are uniform over a block.
#include "philox.h"

namespace smos {

constexpr int kCpFrames = 5;
constexpr int kCpTrials = 20;
constexpr int kCpChunk = 4 * kBlock;
constexpr int kCpWaves = kBlock / kWave;
constexpr int64_t kCpMaxPoints = 1LL << 30;
constexpr int kCpMaxObjPoints = 1 << 20;
constexpr float kCpNoiseStd = 0.001f;      // copy_paste.py:140

struct CpCand {                  // what trial j found (written by prep, read by count and apply)
  int32_t road_ok;               // more than 5 road points under the footprint
  uint32_t lifted;               // bit i: trial i <= j passed the road test (its lift is part of this trial's z)
  int32_t fits[kCpFrames];       // the three spans below their limits
  float box[kCpFrames][4];       // phi_min, phi_max, theta_min, theta_max
  float lift[kCpFrames][kCpTrials];   // the float32 addend of trial i in frame t
};

struct CpState {
  float4* pts;
  uint32_t* word;
  float2* ang;
  uint8_t* flag;
  int32_t* status;
  int64_t off[kCpFrames], n[kCpFrames];
  int64_t slots;                 // M
};

struct CpInit {
  CpState s;
  const float* scan[kCpFrames];
  const uint32_t* label[kCpFrames];
  double first[kCpFrames][12];
  int32_t count;
};

struct CpObject {
  CpState s;
  const float* scan0;
  const uint32_t* label0;
  double first0[12];
  int64_t nchunks0;
  const float4* obj;             // [m, 4] of the bank
  const double* quad;            // [4, 2] footprint of the scaled box, frame 0
  int32_t m, number;
  int64_t slot;                  // first row of the object's slot range behind a frame's scan points
  double shift_x[kCpFrames], shift_y[kCpFrames];      // velo * t * 0.1
  double rot_c[kCpTrials], rot_s[kCpTrials];          // of trial i, in trial order
  const double* noise;           // [5, m, 3] or null: Philox
  uint32_t key[2], sample[2];
  uint32_t paste_word;
  int32_t* road_cnt;             // [20, nchunks0]
  double* road_sum;              // [20, nchunks0]
  CpCand* cand;                  // [20]
  int32_t* blockers;             // [20, 5]
};

__device__ __forceinline__ float sqrt_rn(float v) { return (float)sqrt((double)v); }      // correctly rounded, like numpy's

// get_fov / occlusion_process (copy_paste.py:93-115) in float32, sums left to right
__device__ __forceinline__ void view_angles(float x, float y, float z, float& u, float& phi, float& theta) {
  const float xy = __fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y));
  const float d = __fadd_rn(sqrt_rn(__fadd_rn(xy, __fmul_rn(z, z))), 1e-12f);
  u = __fadd_rn(sqrt_rn(xy), 1e-12f);
  phi = atan2f(x, y);
  theta = asinf(__fdiv_rn(z, d));
}

__device__ __forceinline__ bool object_class(uint32_t word) {
  const uint32_t sem = word & 0xFFFFu;
  return (sem >= 10u && sem < 33u) || (sem >= 252u && sem < 260u);
}

__device__ __forceinline__ float4 pad_point() { return make_float4(-1000.0f, -1000.0f, -4000.0f, -1000.0f); }

// rotate_along_z: [x y] . M in float64 (the caller rounds)
__device__ __forceinline__ void rotate_f64(double x, double y, double c, double s, double& ox, double& oy) {
  ox = __dadd_rn(__dmul_rn(x, c), __dmul_rn(y, s));
  oy = __dsub_rn(__dmul_rn(y, c), __dmul_rn(x, s));
}

// The noise of point p of frame t of object `number` (counter layout: include/smos.h).
__device__ __forceinline__ void seeded_paste_noise(const uint32_t (&key)[2], const uint32_t (&sample)[2], int number, int t, uint32_t p,
                                                   double (&out)[3]) {
  const uint32_t c1 = (1u << 24) | ((uint32_t)number << 8) | (uint32_t)t;
  const Philox4 a = philox4x32_10(p, c1, sample[0], sample[1], key[0], key[1]);
  const Philox4 b = philox4x32_10(p, c1 | (1u << 16), sample[0], sample[1], key[0], key[1]);
  out[0] = (double)__fadd_rn(__fmul_rn(box_muller_f32(a.v[2], a.v[3]), kCpNoiseStd), 0.0f);
  out[1] = (double)__fadd_rn(__fmul_rn(box_muller_f32(b.v[0], b.v[1]), kCpNoiseStd), 0.0f);
  out[2] = (double)__fadd_rn(__fmul_rn(box_muller_f32(b.v[2], b.v[3]), kCpNoiseStd), 0.0f);
}

// make_sequential_obj (copy_paste.py:135-140) for point p (inside the object) of frame t: the shift and the noise are float64
// sums, each rounded once to float32.
__device__ __forceinline__ float4 object_point(const CpObject& a, int t, int p) {
  const float4 b = a.obj[p];
  double nz[3];
  if (a.noise) {        // uniform: a launch reads its noise or generates it
    const double* q = a.noise + ((int64_t)t * a.m + p) * 3;
    nz[0] = q[0];
    nz[1] = q[1];
    nz[2] = q[2];
  } else {
    seeded_paste_noise(a.key, a.sample, a.number, t, (uint32_t)p, nz);
  }
  const float x = (float)__dsub_rn((double)b.x, a.shift_x[t]), y = (float)__dsub_rn((double)b.y, a.shift_y[t]);
  return make_float4((float)__dadd_rn((double)x, nz[0]), (float)__dadd_rn((double)y, nz[1]), (float)__dadd_rn((double)b.z, nz[2]), b.w);
}

// Trials 0..j on a point: every rotation rounds x, y to float32; the lifts of the road-passing trials add up in float32.
__device__ __forceinline__ void replay(const CpObject& a, int j, uint32_t lifted, const float* lift, float4& p) {
  for (int i = 0; i <= j; ++i) {
    double x, y;
    rotate_f64((double)p.x, (double)p.y, a.rot_c[i], a.rot_s[i], x, y);
    p.x = (float)x;
    p.y = (float)y;
    if ((lifted >> i) & 1u) p.z = __fadd_rn(p.z, lift[i]);
  }
}

template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
  return v;
}

// All threads get op over the block; `lds` holds kCpWaves values and is free again after the call.
template <typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, Op op, T* lds) {
  v = wave_reduce(v, op);
  if (threadIdx.x % kWave == 0) lds[threadIdx.x / kWave] = v;
  __syncthreads();
  T r = lds[0];
#pragma unroll
  for (int w = 1; w < kCpWaves; ++w) r = op(r, lds[w]);
  __syncthreads();
  return r;
}

struct MinF { __device__ float operator()(float a, float b) const { return fminf(a, b); } };
struct MaxF { __device__ float operator()(float a, float b) const { return fmaxf(a, b); } };
struct AddI { __device__ int operator()(int a, int b) const { return a + b; } };
struct AddD { __device__ double operator()(double a, double b) const { return __dadd_rn(a, b); } };

__device__ __forceinline__ void frame_of_unit(const int64_t (&blocks)[kCpFrames], int64_t u, int& t, int64_t& b) {
  t = 0;
#pragma unroll
  for (int k = 0; k < kCpFrames - 1; ++k) {
    const bool next = t == k && u >= blocks[k];
    u -= next ? blocks[k] : 0;
    t += next ? 1 : 0;
  }
  b = u;
}

// ---- init: one thread per row ----
__global__ __launch_bounds__(kBlock) void copy_paste_init(CpInit a) {
  int64_t blocks[kCpFrames], total = 0;
  for (int k = 0; k < kCpFrames; ++k) {
    blocks[k] = (a.s.n[k] + a.s.slots + kBlock - 1) / kBlock;
    total += blocks[k];
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < a.count) a.s.status[threadIdx.x] = -1;
  for (int64_t u = blockIdx.x; u < total; u += gridDim.x) {
    int t;
    int64_t b;
    frame_of_unit(blocks, u, t, b);
    const int64_t n = a.s.n[t], r = b * kBlock + threadIdx.x;
    const int64_t src = min(r, n - 1);
    const float4 p = reinterpret_cast<const float4*>(a.scan[t])[src];
    const uint32_t w = a.label[t][src];
    const double dx = p.x, dy = p.y, dz = p.z;
    float4 q;
    q.x = (float)pose_row_f64(a.first[t] + 0, dx, dy, dz);
    q.y = (float)pose_row_f64(a.first[t] + 4, dx, dy, dz);
    q.z = (float)pose_row_f64(a.first[t] + 8, dx, dy, dz);
    q.w = p.w;
    float uu, phi, theta;
    view_angles(q.x, q.y, q.z, uu, phi, theta);
    const bool scan_row = r < n;
    if (r < n + a.s.slots) {
      const int64_t at = a.s.off[t] + r;
      a.s.pts[at] = scan_row ? q : pad_point();
      a.s.word[at] = scan_row ? w : 0u;
      a.s.ang[at] = make_float2(scan_row ? phi : 0.0f, scan_row ? theta : 0.0f);
      a.s.flag[at] = scan_row ? (uint8_t)(1u | (object_class(w) ? 2u : 0u)) : (uint8_t)0;
    }
  }
}

// ---- road: scan 0's road points against the 20 footprints ----
__global__ __launch_bounds__(kBlock) void copy_paste_road(CpObject a) {
  __shared__ double quad[kCpTrials][4][2];
  __shared__ int w_cnt[kCpWaves][kCpTrials];
  __shared__ double w_sum[kCpWaves][kCpTrials];
  // candidate c = the footprint after trials 0..c; the first kCpTrials threads replay one chain each, all the same number of
  // steps (a step past the own trial leaves the value alone)
  {
    const int c = min((int)threadIdx.x, kCpTrials - 1);
    double q[4][2];
    for (int v = 0; v < 4; ++v) {
      q[v][0] = a.quad[2 * v];
      q[v][1] = a.quad[2 * v + 1];
    }
    for (int i = 0; i < kCpTrials; ++i)
      for (int v = 0; v < 4; ++v) {
        double x, y;
        rotate_f64(q[v][0], q[v][1], a.rot_c[i], a.rot_s[i], x, y);
        q[v][0] = i <= c ? x : q[v][0];
        q[v][1] = i <= c ? y : q[v][1];
      }
    if ((int)threadIdx.x < kCpTrials)
      for (int v = 0; v < 4; ++v) {
        quad[c][v][0] = q[v][0];
        quad[c][v][1] = q[v][1];
      }
  }
  __syncthreads();
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int64_t n = a.s.n[0];
  for (int64_t chunk = blockIdx.x; chunk < a.nchunks0; chunk += gridDim.x) {
    // the chunk's four points of this thread stay in registers; the candidates are walked one after the other
    constexpr int kRounds = kCpChunk / kBlock;
    double px[kRounds], py[kRounds];
    float z[kRounds];
    bool road[kRounds], any_road = false;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
      const int64_t i = chunk * kCpChunk + r * kBlock + threadIdx.x;
      const int64_t src = min(i, n - 1);
      const float4 p = reinterpret_cast<const float4*>(a.scan0)[src];
      road[r] = i < n && (a.label0[src] & 0xFFFFu) == 40u;
      any_road = any_road || road[r];
      const double dx = p.x, dy = p.y, dz = p.z;
      px[r] = (double)(float)pose_row_f64(a.first0 + 0, dx, dy, dz);
      py[r] = (double)(float)pose_row_f64(a.first0 + 4, dx, dy, dz);
      z[r] = (float)pose_row_f64(a.first0 + 8, dx, dy, dz);
    }
    const bool wave_has_road = __any(any_road);       // wave-uniform
#pragma unroll 1
    for (int c = 0; c < kCpTrials; ++c) {
      int cnt = 0;
      double sum = 0.0;
      if (wave_has_road) {
        double ax[4], ay[4], ex[4], ey[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          ax[v] = quad[c][v][0];
          ay[v] = quad[c][v][1];
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          ex[v] = __dsub_rn(ax[(v + 1) & 3], ax[v]);
          ey[v] = __dsub_rn(ay[(v + 1) & 3], ay[v]);
        }
#pragma unroll
        for (int r = 0; r < kRounds; ++r) {
          bool pos = true, neg = true;
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const double cr = __dsub_rn(__dmul_rn(ex[v], __dsub_rn(py[r], ay[v])), __dmul_rn(ey[v], __dsub_rn(px[r], ax[v])));
            pos = pos && cr >= 0.0;
            neg = neg && cr <= 0.0;
          }
          const bool in = road[r] && (pos || neg);
          cnt += in ? 1 : 0;
          sum = __dadd_rn(sum, in ? (double)z[r] : 0.0);
        }
        cnt = wave_reduce(cnt, AddI());
        sum = wave_reduce(sum, AddD());
      }
      if (lane == 0) {
        w_cnt[wave][c] = cnt;
        w_sum[wave][c] = sum;
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < kCpTrials) {
      int tc = 0;
      double ts = 0.0;
      for (int w = 0; w < kCpWaves; ++w) {
        tc += w_cnt[w][threadIdx.x];
        ts = __dadd_rn(ts, w_sum[w][threadIdx.x]);
      }
      a.road_cnt[(int64_t)threadIdx.x * a.nchunks0 + chunk] = tc;
      a.road_sum[(int64_t)threadIdx.x * a.nchunks0 + chunk] = ts;
    }
    __syncthreads();
  }
}

// ---- prep: candidate j ----
__global__ __launch_bounds__(kBlock) void copy_paste_prep(CpObject a) {
  __shared__ int pass[kCpTrials];
  __shared__ float mean[kCpTrials];
  __shared__ float lift[kCpFrames][kCpTrials];
  __shared__ float redf[kCpWaves];
  for (int j = blockIdx.x; j < kCpTrials; j += gridDim.x) {
    // road count and mean of every trial: thread c < 20 adds the chunks of candidate c in chunk order (the others repeat 19)
    {
      const int c = min((int)threadIdx.x, kCpTrials - 1);
      int cnt = 0;
      double sum = 0.0;
      for (int64_t ch = 0; ch < a.nchunks0; ++ch) {
        cnt += a.road_cnt[(int64_t)c * a.nchunks0 + ch];
        sum = __dadd_rn(sum, a.road_sum[(int64_t)c * a.nchunks0 + ch]);
      }
      if ((int)threadIdx.x < kCpTrials) {
        pass[c] = cnt > 5 ? 1 : 0;                                  // copy_paste.py:209
        mean[c] = cnt > 0 ? (float)(sum / (double)cnt) : 0.0f;      // the float64 sum rounded once (numpy: pairwise float32)
      }
    }
    __syncthreads();
    // z.min() of every frame before any lift; a lift moves every z of a frame by the same float32 addend, which keeps the
    // minimum where it is (rounding is monotone), so the chain of minima is the chain of that one value
    float zmin[kCpFrames];
    for (int t = 0; t < kCpFrames; ++t) {
      float v = INFINITY;
      for (int p0 = 0; p0 < a.m; p0 += kBlock) {
        const int p = p0 + threadIdx.x;
        const float4 q = object_point(a, t, min(p, a.m - 1));
        v = fminf(v, p < a.m ? q.z : INFINITY);
      }
      zmin[t] = block_reduce(v, MinF(), redf);
    }
    uint32_t lifted = 0;
    for (int i = 0; i <= j; ++i) lifted |= pass[i] ? (1u << i) : 0u;
    if ((int)threadIdx.x < kCpFrames) {
      float zm = INFINITY;
      for (int t = 0; t < kCpFrames; ++t) zm = (int)threadIdx.x == t ? zmin[t] : zm;
      for (int i = 0; i < kCpTrials; ++i) {
        const float d = __fsub_rn(mean[i], zm);                     // road_mean_height - z.min(), float32
        const bool on = i <= j && pass[i];
        lift[threadIdx.x][i] = on ? d : 0.0f;
        zm = on ? __fadd_rn(zm, d) : zm;
      }
    }
    __syncthreads();
    CpCand* out = a.cand + j;
    const int ok = pass[j];
    for (int t = 0; t < kCpFrames; ++t) {
      float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
      if (ok) {       // uniform
        for (int p0 = 0; p0 < a.m; p0 += kBlock) {
          const int p = p0 + threadIdx.x;
          float4 q = object_point(a, t, min(p, a.m - 1));
          replay(a, j, lifted, lift[t], q);
          float v[3];
          view_angles(q.x, q.y, q.z, v[0], v[1], v[2]);
          for (int d = 0; d < 3; ++d) {
            lo[d] = fminf(lo[d], p < a.m ? v[d] : INFINITY);
            hi[d] = fmaxf(hi[d], p < a.m ? v[d] : -INFINITY);
          }
        }
        for (int d = 0; d < 3; ++d) {
          lo[d] = block_reduce(lo[d], MinF(), redf);
          hi[d] = block_reduce(hi[d], MaxF(), redf);
        }
      }
      if (threadIdx.x == 0) {
        // copy_paste.py:160
        out->fits[t] = ok && fabsf(__fsub_rn(hi[0], lo[0])) < 8.0f && fabsf(__fsub_rn(hi[1], lo[1])) < 1.0f && fabsf(__fsub_rn(hi[2], lo[2])) < 1.0f;
        out->box[t][0] = lo[1];
        out->box[t][1] = hi[1];
        out->box[t][2] = lo[2];
        out->box[t][3] = hi[2];
        a.blockers[j * kCpFrames + t] = 0;
      }
    }
    if (threadIdx.x == 0) {
      out->road_ok = ok;
      out->lifted = lifted;
    }
    if ((int)threadIdx.x < kCpFrames * kCpTrials) out->lift[threadIdx.x / kCpTrials][threadIdx.x % kCpTrials] = lift[threadIdx.x / kCpTrials][threadIdx.x % kCpTrials];
    __syncthreads();
  }
}

// rows of frame t a launch of object `a` looks at: the scan points and the slots of the objects before it
__device__ __forceinline__ int64_t live_rows(const CpObject& a, int t) { return a.s.n[t] + a.slot; }

// ---- count: object-class points inside the boxes ----
__global__ __launch_bounds__(kBlock) void copy_paste_count(CpObject a) {
  int64_t blocks[kCpFrames], total = 0;
  for (int k = 0; k < kCpFrames; ++k) {
    blocks[k] = (live_rows(a, k) + kBlock - 1) / kBlock;
    total += blocks[k];
  }
  const int lane = threadIdx.x % kWave;
  for (int64_t u = blockIdx.x; u < total; u += gridDim.x) {
    int t;
    int64_t b;
    frame_of_unit(blocks, u, t, b);
    const int64_t rows = live_rows(a, t), r = b * kBlock + threadIdx.x;
    const int64_t at = a.s.off[t] + min(r, rows - 1);
    const float2 g = a.s.ang[at];
    const bool blocker = r < rows && (a.s.flag[at] & 3u) == 3u;
    if (!__any(blocker)) continue;        // wave-uniform
    for (int c = 0; c < kCpTrials; ++c) {
      const CpCand* cd = a.cand + c;
      if (!(cd->road_ok && cd->fits[t])) continue;      // block-uniform
      const float* bx = cd->box[t];
      // in_range: half-open (copy_paste.py:11-12,114)
      const bool in = blocker && g.x >= bx[0] && g.x < bx[1] && g.y >= bx[2] && g.y < bx[3];
      const int k = __popcll(__ballot(in));
      if (lane == 0 && k > 0) atomicAdd(a.blockers + c * kCpFrames + t, k);
    }
  }
}

// ---- apply ----
__global__ __launch_bounds__(kBlock) void copy_paste_apply(CpObject a) {
  int chosen = -1;
  for (int c = kCpTrials - 1; c >= 0; --c) {
    const CpCand* cd = a.cand + c;
    bool ok = cd->road_ok != 0;
    for (int t = 0; t < kCpFrames; ++t) ok = ok && cd->fits[t] && a.blockers[c * kCpFrames + t] < 3;      // copy_paste.py:164,218-223
    chosen = ok ? c : chosen;
  }
  if (chosen < 0) return;       // uniform over the launch; the status stays -1
  const CpCand* cd = a.cand + chosen;
  if (blockIdx.x == 0 && threadIdx.x == 0) a.s.status[a.number] = chosen;
  int64_t blocks[kCpFrames], total = 0;
  for (int k = 0; k < kCpFrames; ++k) {
    blocks[k] = (live_rows(a, k) + kBlock - 1) / kBlock;
    total += blocks[k];
  }
  const int64_t oblocks = (a.m + kBlock - 1) / kBlock;
  for (int64_t u = blockIdx.x; u < total + kCpFrames * oblocks; u += gridDim.x) {
    if (u < total) {            // block-uniform: the rows inside the frame's box go
      int t;
      int64_t b;
      frame_of_unit(blocks, u, t, b);
      const int64_t rows = live_rows(a, t), r = b * kBlock + threadIdx.x;
      const int64_t at = a.s.off[t] + min(r, rows - 1);
      const float2 g = a.s.ang[at];
      const uint8_t f = a.s.flag[at];
      const float* bx = cd->box[t];
      if (r < rows && (f & 1u) && g.x >= bx[0] && g.x < bx[1] && g.y >= bx[2] && g.y < bx[3]) {
        a.s.pts[at] = pad_point();
        a.s.flag[at] = (uint8_t)(f & 2u);
      }
    } else {                    // the object's rows of frame t
      const int64_t v = u - total;
      const int t = (int)(v / oblocks);
      const int p = (int)(v - (int64_t)t * oblocks) * kBlock + threadIdx.x;
      float4 q = object_point(a, t, min(p, a.m - 1));
      replay(a, chosen, cd->lifted, cd->lift[t], q);
      float uu, phi, theta;
      view_angles(q.x, q.y, q.z, uu, phi, theta);
      if (p < a.m) {
        const int64_t at = a.s.off[t] + a.s.n[t] + a.slot + p;
        a.s.pts[at] = q;
        a.s.word[at] = a.paste_word;
        a.s.ang[at] = make_float2(phi, theta);
        a.s.flag[at] = (uint8_t)3;
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void copy_paste_draws(uint32_t k0, uint32_t k1, uint32_t s0, uint32_t s1, int number, int m,
                                                           double* __restrict__ noise) {
  const uint32_t key[2] = {k0, k1}, sample[2] = {s0, s1};
  const int64_t total = (int64_t)kCpFrames * m;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int t = (int)(idx / m);
    double nz[3];
    seeded_paste_noise(key, sample, number, t, (uint32_t)(idx - (int64_t)t * m), nz);
    noise[idx * 3 + 0] = nz[0];
    noise[idx * 3 + 1] = nz[1];
    noise[idx * 3 + 2] = nz[2];
  }
}

static int64_t cp_align256(int64_t b) { return (b + 255) / 256 * 256; }
static int64_t cp_chunks(int64_t n0) { return (n0 + kCpChunk - 1) / kCpChunk; }

static int fill_state(CpState& s, const int64_t* n, int64_t slots, void* pts, void* words, void* ang, void* flags, int32_t* status) {
  SMOS_REQUIRE(n && pts && words && ang && flags && status, "copy_paste: null pointer");
  SMOS_REQUIRE(slots >= 0 && slots <= kCpMaxPoints, "copy_paste: %lld object points outside 0..2^30", (long long)slots);
  int64_t off = 0;
  for (int k = 0; k < kCpFrames; ++k) {
    SMOS_REQUIRE(n[k] >= 1 && n[k] <= kCpMaxPoints, "copy_paste: scan %d has %lld points (1..2^30)", k, (long long)n[k]);
    s.n[k] = n[k];
    s.off[k] = off;
    off += n[k] + slots;
  }
  s.slots = slots;
  s.pts = (float4*)pts;
  s.word = (uint32_t*)words;
  s.ang = (float2*)ang;
  s.flag = (uint8_t*)flags;
  s.status = status;
  return SMOS_OK;
}

}  // namespace smos

using namespace smos;

extern "C" int64_t smos_copy_paste_work_bytes(int64_t n0) {
  if (n0 < 1 || n0 > kCpMaxPoints) return -1;
  return cp_align256(kCpTrials * cp_chunks(n0) * 4) + cp_align256(kCpTrials * cp_chunks(n0) * 8) + cp_align256(kCpTrials * sizeof(CpCand)) +
         cp_align256(kCpTrials * kCpFrames * 4);
}

extern "C" int smos_copy_paste_begin(const void* const* scans, const void* const* label_words, const int64_t* n, const double* first_pose,
                                     int64_t slots, int32_t count, void* pts, void* words, void* angles, void* flags, int32_t* status,
                                     smos_stream_t stream) {
  SMOS_REQUIRE(scans && label_words && first_pose, "copy_paste_begin: null pointer");
  SMOS_REQUIRE(count >= 0 && count <= kBlock, "copy_paste_begin: %d objects outside 0..%d", (int)count, kBlock);
  CpInit a;
  const int rc = fill_state(a.s, n, slots, pts, words, angles, flags, status);
  if (rc != SMOS_OK) return rc;
  int64_t units = 0;
  for (int k = 0; k < kCpFrames; ++k) {
    SMOS_REQUIRE(scans[k] && label_words[k], "copy_paste_begin: null scan pointer");
    a.scan[k] = (const float*)scans[k];
    a.label[k] = (const uint32_t*)label_words[k];
    for (int i = 0; i < 12; ++i) a.first[k][i] = first_pose[16 * k + i];
    units += (n[k] + slots + kBlock - 1) / kBlock;
  }
  a.count = count;
  hipLaunchKernelGGL(copy_paste_init, dim3((unsigned)conv_grid_cap(grid_for(units, 1, kMaxGrid))), dim3(kBlock), 0, (hipStream_t)stream, a);
  return check_launch("copy_paste_begin");
}

extern "C" int smos_copy_paste_object(const void* scan0, const void* label_words0, const double* first_pose0, const int64_t* n, int64_t slots,
                                      void* pts, void* words, void* angles, void* flags, int32_t* status, int32_t count, int32_t number,
                                      const void* object_points, int32_t m, int64_t slot, const double* footprint,
                                      const double* shift_x5, const double* shift_y5, const uint8_t* order20, const double* cos20,
                                      const double* sin20, const double* noise, uint64_t seed, uint64_t sample_index, uint32_t paste_word,
                                      void* work, int64_t work_bytes, smos_stream_t stream) {
  SMOS_REQUIRE(scan0 && label_words0 && first_pose0 && object_points && footprint && shift_x5 && shift_y5 && order20 && cos20 && sin20 && work,
               "copy_paste_object: null pointer");
  CpObject a;
  const int rc = fill_state(a.s, n, slots, pts, words, angles, flags, status);
  if (rc != SMOS_OK) return rc;
  SMOS_REQUIRE(m >= 10 && m <= kCpMaxObjPoints, "copy_paste_object: an object of %d points (10..2^20; smaller ones are skipped by the caller)", (int)m);
  SMOS_REQUIRE(slot >= 0 && slot + m <= slots, "copy_paste_object: slot %lld + %d points past the %lld reserved", (long long)slot, (int)m,
               (long long)slots);
  SMOS_REQUIRE(count >= 1 && count <= kBlock && number >= 0 && number < count, "copy_paste_object: object number %d of %d (at most %d)",
               (int)number, (int)count, kBlock);
  SMOS_REQUIRE(paste_word <= 0xFFFFu, "copy_paste_object: label id %u does not fit the low half of a label word", (unsigned)paste_word);
  SMOS_REQUIRE(work_bytes >= smos_copy_paste_work_bytes(n[0]), "copy_paste_object: work buffer of %lld bytes, %lld needed", (long long)work_bytes,
               (long long)smos_copy_paste_work_bytes(n[0]));
  bool seen[kCpTrials] = {};
  for (int i = 0; i < kCpTrials; ++i) {
    SMOS_REQUIRE(order20[i] < kCpTrials && !seen[order20[i]], "copy_paste_object: the trial order is not a permutation of 0..19");
    seen[order20[i]] = true;
    a.rot_c[i] = cos20[order20[i]];
    a.rot_s[i] = sin20[order20[i]];
  }
  a.scan0 = (const float*)scan0;
  a.label0 = (const uint32_t*)label_words0;
  for (int i = 0; i < 12; ++i) a.first0[i] = first_pose0[i];
  a.nchunks0 = cp_chunks(n[0]);
  a.obj = (const float4*)object_points;
  a.quad = footprint;
  a.m = m;
  a.number = number;
  a.slot = slot;
  for (int t = 0; t < kCpFrames; ++t) {
    a.shift_x[t] = shift_x5[t];
    a.shift_y[t] = shift_y5[t];
  }
  a.noise = noise;
  a.key[0] = (uint32_t)seed;
  a.key[1] = (uint32_t)(seed >> 32);
  a.sample[0] = (uint32_t)sample_index;
  a.sample[1] = (uint32_t)(sample_index >> 32);
  a.paste_word = paste_word;
  char* wp = (char*)work;
  a.road_cnt = (int32_t*)wp;
  wp += cp_align256(kCpTrials * a.nchunks0 * 4);
  a.road_sum = (double*)wp;
  wp += cp_align256(kCpTrials * a.nchunks0 * 8);
  a.cand = (CpCand*)wp;
  wp += cp_align256(kCpTrials * sizeof(CpCand));
  a.blockers = (int32_t*)wp;
  int64_t row_units = 0;
  for (int k = 0; k < kCpFrames; ++k) row_units += (n[k] + slot + kBlock - 1) / kBlock;
  const int64_t obj_units = (int64_t)kCpFrames * ((m + kBlock - 1) / kBlock);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(copy_paste_road, dim3((unsigned)conv_grid_cap(grid_for(a.nchunks0, 1, kMaxGrid))), dim3(kBlock), 0, s, a);
  hipLaunchKernelGGL(copy_paste_prep, dim3((unsigned)conv_grid_cap(kCpTrials)), dim3(kBlock), 0, s, a);
  hipLaunchKernelGGL(copy_paste_count, dim3((unsigned)conv_grid_cap(grid_for(row_units, 1, kMaxGrid))), dim3(kBlock), 0, s, a);
  hipLaunchKernelGGL(copy_paste_apply, dim3((unsigned)conv_grid_cap(grid_for(row_units + obj_units, 1, kMaxGrid))), dim3(kBlock), 0, s, a);
  return check_launch("copy_paste_object");
}

extern "C" int smos_copy_paste_draws(uint64_t seed, uint64_t sample_index, int32_t number, int32_t m, double* noise, smos_stream_t stream) {
  SMOS_REQUIRE(m >= 1 && m <= kCpMaxObjPoints, "copy_paste_draws: an object of %d points (1..2^20)", (int)m);
  SMOS_REQUIRE(number >= 0 && number < kBlock, "copy_paste_draws: object number %d outside 0..%d", (int)number, kBlock - 1);
  SMOS_REQUIRE(noise, "copy_paste_draws: null device pointer");
  hipLaunchKernelGGL(copy_paste_draws, dim3((unsigned)conv_grid_cap(grid_for((int64_t)kCpFrames * m, kBlock, kMaxGrid))), dim3(kBlock), 0,
                     (hipStream_t)stream, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)sample_index, (uint32_t)(sample_index >> 32),
                     (int)number, (int)m, noise);
  return check_launch("copy_paste_draws");
}
