// Instance-level voting for gfx950: the two heavy parts of cluster()
// (voxel_instance_voting.py:144-193) as device kernels.
//
//   dbscan     : DBSCAN(eps, min_samples).fit_predict of the scan's foreground points (:150-153).  scikit-learn's
//                result is a pure function of the eps-neighbourhood graph: core = at least min_samples points within
//                eps (the point itself included); clusters = connected components of the core points; a border point
//                takes the cluster that is expanded first among those it touches; clusters are numbered in the order
//                of their lowest-index core point.  Here every cluster is NAMED by the index of its lowest core point
//                (so "expanded first" = smallest name): a neighbour count, min-label propagation with pointer jumping
//                until nothing changes, and one pass for the border points -- each a banded pair test over the
//                x-sorted points.  Distances are taken the
//                way scikit-learn's KD-tree takes them: float32 coordinates widened to float64, squared differences
//                summed x, y, z without contraction, compared with eps*eps by <=.
//   box_vote   : for every kept cluster, the number of local-map points of class 1 / 2 inside its axis-aligned box
//                (:170-187) -- the local map is never materialised: history frames are pose-aligned (float64 matmul,
//                float32 result, datasets/utils.py:116-126) and cropped (utils/transforms.py:151-161) on the fly, as
//                in vote.hip.  in_hull() of the reference triangulates the 8 box corners and asks find_simplex >= 0;
//                for float32 points and float32 corners that is the closed interval test used here.
#include "smos_common.h"
#include <hipcub/hipcub.hpp>

namespace smos {

constexpr int kTile = kBlock;   // points staged per LDS tile

__device__ __forceinline__ bool within(double xi, double yi, double zi, float qx, float qy, float qz, double eps2) {
  const double dx = __dsub_rn(xi, (double)qx), dy = __dsub_rn(yi, (double)qy), dz = __dsub_rn(zi, (double)qz);
  const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
  return d2 <= eps2;
}

// The points are processed in x-sorted order (hipCUB radix sort of the x coordinate): a block of 256 consecutive sorted
// points only has to look at the sorted range whose x lies within eps of the block's own x interval, which turns the
// all-pairs test into a narrow band.  Cluster names stay ORIGINAL indices (orig[] maps sorted position -> original index,
// pos[] back), so the result does not depend on the sort.
__global__ __launch_bounds__(kBlock) void dbscan_keys(const float* __restrict__ pts, int n, int64_t stride, float* __restrict__ keys,
                                                      int* __restrict__ iota) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) {
    keys[i] = pts[(int64_t)i * stride];
    iota[i] = i;
  }
}

__global__ __launch_bounds__(kBlock) void dbscan_gather(const float* __restrict__ pts, int n, int64_t stride, const int* __restrict__ orig,
                                                        const float* __restrict__ keys_sorted, double eps, float4* __restrict__ sp,
                                                        int* __restrict__ pos, int2* __restrict__ band) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) {
    const int o = orig[i];
    const float* p = pts + (int64_t)o * stride;
    sp[i] = make_float4(p[0], p[1], p[2], 0.0f);
    pos[o] = i;
  }
  if (threadIdx.x == 0) {
    // band of this block: sorted positions whose x is in [x_first - eps, x_last + eps] (float64 bounds: a superset of
    // the exact neighbourhood, the exact test happens per pair)
    const int first = blockIdx.x * kBlock, last = min(n, first + kBlock) - 1;
    const double lo = (double)keys_sorted[first] - eps, hi = (double)keys_sorted[last] + eps;
    int a = 0, b = first;                       // lowest position with key >= lo
    while (a < b) {
      const int m = (a + b) >> 1;
      if ((double)keys_sorted[m] < lo) a = m + 1; else b = m;
    }
    int c = last + 1, d = n;                    // lowest position with key > hi
    while (c < d) {
      const int m = (c + d) >> 1;
      if ((double)keys_sorted[m] <= hi) c = m + 1; else d = m;
    }
    band[blockIdx.x] = make_int2(a, c);
  }
}

// mode 0: label[i] = orig[i] if sorted point i is a core point, else -1
// mode 1: one propagation sweep over the core points (label[] in place; *changed set when a label dropped)
// mode 2: out[orig[i]] = cluster name (core: its label; border: smallest label among its core neighbours; else -1)
template <int kMode>
__global__ __launch_bounds__(kBlock) void dbscan_pass(const float4* __restrict__ sp, int n, const int2* __restrict__ band,
                                                      const int* __restrict__ orig, const int* __restrict__ pos, double eps2,
                                                      int min_samples, int* label, int* __restrict__ out, int* changed) {
  __shared__ float tx[kTile], ty[kTile], tz[kTile];
  __shared__ int tl[kTile];
  const int i = blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < n;
  double xi = 0, yi = 0, zi = 0;
  int mine = -1;
  if (live) {
    const float4 p = sp[i];
    xi = p.x; yi = p.y; zi = p.z;
    if (kMode != 0) {
      mine = label[i];
      if (kMode == 1 && mine >= 0) mine = label[pos[mine]];   // pointer jumping: adopt the label of my representative
    }
  }
  int count = 0;
  int best = (kMode == 2 && mine < 0) ? 0x7fffffff : mine;
  const bool active = live && (kMode == 0 || (kMode == 1 && mine >= 0) || (kMode == 2 && mine < 0));
  const int2 range = band[blockIdx.x];
  for (int j0 = range.x; j0 < range.y; j0 += kTile) {
    const int j = j0 + threadIdx.x;
    __syncthreads();
    if (j < range.y) {
      const float4 q = sp[j];
      tx[threadIdx.x] = q.x; ty[threadIdx.x] = q.y; tz[threadIdx.x] = q.z;
      if (kMode != 0) tl[threadIdx.x] = label[j];
    }
    __syncthreads();
    if (!active) continue;
    const int m = min(kTile, range.y - j0);
    for (int t = 0; t < m; ++t) {
      if (kMode != 0 && tl[t] < 0) continue;   // only core points carry labels
      if (!within(xi, yi, zi, tx[t], ty[t], tz[t], eps2)) continue;
      if (kMode == 0) ++count;
      else best = min(best, tl[t]);
    }
  }
  if (!live) return;
  if (kMode == 0) {
    label[i] = count >= min_samples ? orig[i] : -1;
  } else if (kMode == 1) {
    if (mine >= 0 && best < label[i]) {
      label[i] = best;
      *changed = 1;
    }
  } else {
    out[orig[i]] = mine >= 0 ? mine : (best == 0x7fffffff ? -1 : best);
  }
}

struct BoxPose {
  double m[12];
  int identity;
};

// counts[k*3 + c] += 1 for every kept point of class c inside box k.  boxes: [K, 6] float32 (lo xyz, hi xyz).
__global__ __launch_bounds__(kBlock) void box_vote(const float* __restrict__ pts, int64_t n, int64_t stride,
                                                   const uint8_t* __restrict__ labels, BoxPose pose, float clo0, float clo1,
                                                   float clo2, float chi0, float chi1, float chi2,
                                                   const float* __restrict__ boxes, int K, unsigned* __restrict__ counts) {
  extern __shared__ float lds_box[];
  for (int t = threadIdx.x; t < K * 6; t += blockDim.x) lds_box[t] = boxes[t];
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const unsigned lab = labels[i];
    if (lab == 0 || lab > 2) continue;          // only classes 1 and 2 are ever read back (:178-179)
    const float* row = pts + i * stride;
    float x = row[0], y = row[1], z = row[2];
    if (!pose.identity) {
      const double dx = x, dy = y, dz = z;
      x = (float)pose_row_f64(pose.m + 0, dx, dy, dz);
      y = (float)pose_row_f64(pose.m + 4, dx, dy, dz);
      z = (float)pose_row_f64(pose.m + 8, dx, dy, dz);
    }
    if (!((x > clo0) && (x < chi0) && (y > clo1) && (y < chi1) && (z > clo2) && (z < chi2))) continue;
    for (int k = 0; k < K; ++k) {
      const float* b = lds_box + k * 6;
      if (x >= b[0] && x <= b[3] && y >= b[1] && y <= b[4] && z >= b[2] && z <= b[5]) atomicAdd(counts + k * 3 + lab, 1u);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The device-resident form (smos_instance_cluster / smos_box_vote_dev / smos_instance_apply): the same clustering, boxes
// and vote as a FIXED sequence of launches whose grids come from the scan's point count n alone.  The kernels take the
// whole scan and its `_bf` labels; the foreground count n_fg, the cluster count K and everything derived from them stay
// in device memory, and every kernel reads them from there.  Foreground points sort to the front (key = x), so a block
// whose first sorted position is >= n_fg has nothing to do and returns.
//
// Components of the core points: a union-find over ORIGINAL (scan) indices in which a root is always the lowest index
// of its set -- the cluster's name.  Every core-core edge of the band links the two roots by an atomic min that hooks
// the larger root under the smaller one; when the atomic finds the larger root already re-hooked, the link carries on
// with the value it found and the smaller root.  Both indices only decrease, so every loop ends by its own progress:
// nothing waits for another thread.  parent[] is read with agent-scope atomic loads inside the linking launch (another
// XCD's atomic is not visible to a plain load); flattening is the next launch.

constexpr unsigned kKeyBehind = 0xFFFFFFFFu;   // sort key of a non-foreground point (foreground keys stay below it)

// order-preserving image of a float's bits (unsigned compare == float compare; -0 is folded into +0 first)
__device__ __forceinline__ unsigned float_image(float v) {
  const unsigned b = __float_as_uint(v + 0.0f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float image_float(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

struct ClusterStats {   // per name (= scan index of the cluster's lowest core point)
  unsigned* count;      // [n]
  unsigned* lo;         // [3n] images of the minima, x | y | z planes
  unsigned* hi;         // [3n]
};

__global__ void instance_reset(int* __restrict__ n_fg, int* __restrict__ k_raw, int* __restrict__ k_dev, int* __restrict__ status) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    *n_fg = 0;
    *k_raw = 0;
    *k_dev = 0;
    *status = 0;
  }
}

// keys[i] = image of x for a foreground point, kKeyBehind otherwise; n_fg += foreground points of the block; and the
// per-scan-index words the later kernels accumulate into or only partly overwrite get their start values here.
__global__ __launch_bounds__(kBlock) void instance_keys(const float* __restrict__ pts, int n, int64_t stride,
                                                        const uint8_t* __restrict__ bf, unsigned* __restrict__ keys,
                                                        int* __restrict__ iota, int* __restrict__ n_fg, ClusterStats st,
                                                        int* __restrict__ names, int* __restrict__ slot_of) {
  __shared__ int block_fg;
  if (threadIdx.x == 0) block_fg = 0;
  __syncthreads();
  const int i = blockIdx.x * kBlock + threadIdx.x;
  bool fg = false;
  if (i < n) {
    fg = bf[i] == 2;
    unsigned key = kKeyBehind;
    if (fg) key = min(float_image(pts[(int64_t)i * stride]), kKeyBehind - 1u);   // (a NaN x must not pass for "behind")
    keys[i] = key;
    iota[i] = i;
    names[i] = -1;
    slot_of[i] = -1;
    st.count[i] = 0u;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      st.lo[(int64_t)d * n + i] = 0xFFFFFFFFu;
      st.hi[(int64_t)d * n + i] = 0u;
    }
  }
  const int wave_fg = __popcll(__ballot(fg));
  if ((threadIdx.x & (kWave - 1)) == 0 && wave_fg) atomicAdd(&block_fg, wave_fg);
  __syncthreads();
  if (threadIdx.x == 0 && block_fg) atomicAdd(n_fg, block_fg);
}

// dbscan_gather for the first n_fg sorted positions: x-sorted copy of the foreground points and each block's band, the
// search bounded by n_fg (a non-foreground point is in no band, whatever its coordinates).
__global__ __launch_bounds__(kBlock) void instance_gather(const float* __restrict__ pts, const int* __restrict__ n_fg_ptr, int64_t stride,
                                                          const int* __restrict__ orig, const unsigned* __restrict__ keys_sorted,
                                                          double eps, float4* __restrict__ sp, int2* __restrict__ band) {
  const int n = *n_fg_ptr;
  const int first = blockIdx.x * kBlock;
  if (first >= n) return;
  const int i = first + threadIdx.x;
  if (i < n) {
    const float* p = pts + (int64_t)orig[i] * stride;
    sp[i] = make_float4(p[0], p[1], p[2], 0.0f);
  }
  if (threadIdx.x == 0) {
    const int last = min(n, first + kBlock) - 1;
    const double lo = (double)image_float(keys_sorted[first]) - eps, hi = (double)image_float(keys_sorted[last]) + eps;
    int a = 0, b = first;                       // lowest position with key >= lo
    while (a < b) {
      const int m = (a + b) >> 1;
      if ((double)image_float(keys_sorted[m]) < lo) a = m + 1; else b = m;
    }
    int c = last + 1, d = n;                    // lowest position with key > hi
    while (c < d) {
      const int m = (c + d) >> 1;
      if ((double)image_float(keys_sorted[m]) <= hi) c = m + 1; else d = m;
    }
    band[blockIdx.x] = make_int2(a, c);
  }
}

__device__ __forceinline__ int uf_load(const int* parent, int x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Root of x: walks strictly decreasing parents.  On the way a node whose parent is no root is re-hooked to its grandparent
// (an atomic min: a parent only ever moves down, and stays inside its set).
__device__ __forceinline__ int uf_find(int* parent, int x) {
  int p = uf_load(parent, x);
  while (p != x) {
    const int g = uf_load(parent, p);
    if (g != p) __hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p;
    p = g;
  }
  return x;
}

// Joins the sets of a and b; returns a root-or-ancestor estimate of the joined set (the smaller root seen last).
__device__ __forceinline__ int uf_unite(int* parent, int a, int b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return a;
    const int hi = max(a, b), lo = min(a, b);
    const int was = __hip_atomic_fetch_min(parent + hi, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (was == hi) return lo;                  // hi was still a root and now hangs under lo
    a = was;                                   // hi had been re-hooked to `was` (< hi) meanwhile: its set and lo's remain to be joined
    b = lo;
  }
}

// mode 0: core test (dbscan_pass<0>): core[i] = orig[i] and parent[orig[i]] = orig[i] for a core point, core[i] = -1 otherwise
// mode 1: every core-core edge (i, j) of the band with j > i links the two sets in parent[]
// mode 2: core[i] = root of orig[i] (flatten; no pair test)
// mode 3: border pass (dbscan_pass<2>) into names[] in scan-index space, and the cluster's statistics
template <int kMode>
__global__ __launch_bounds__(kBlock) void instance_pass(const float4* __restrict__ sp, const int* __restrict__ n_fg_ptr,
                                                        const int2* __restrict__ band, const int* __restrict__ orig, double eps2,
                                                        int min_samples, int* core, int* parent, int* __restrict__ names,
                                                        ClusterStats st, int n_scan) {
  __shared__ float tx[kTile], ty[kTile], tz[kTile];
  __shared__ int tl[kTile];
  const int n = *n_fg_ptr;
  if ((int)(blockIdx.x * kBlock) >= n) return;
  const int i = blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < n;
  if (kMode == 2) {
    if (live && core[i] >= 0) core[i] = uf_find(parent, core[i]);
    return;
  }
  double xi = 0, yi = 0, zi = 0;
  float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
  int mine = -1;
  if (live) {
    p = sp[i];
    xi = p.x; yi = p.y; zi = p.z;
    if (kMode != 0) mine = core[i];
  }
  int count = 0;
  int best = (kMode == 3 && mine < 0) ? 0x7fffffff : mine;
  const bool active = live && (kMode == 0 || (kMode == 1 && mine >= 0) || (kMode == 3 && mine < 0));
  const int2 range = band[blockIdx.x];
  for (int j0 = range.x; j0 < range.y; j0 += kTile) {
    const int j = j0 + threadIdx.x;
    __syncthreads();
    if (j < range.y) {
      const float4 q = sp[j];
      tx[threadIdx.x] = q.x; ty[threadIdx.x] = q.y; tz[threadIdx.x] = q.z;
      if (kMode != 0) tl[threadIdx.x] = core[j];
    }
    __syncthreads();
    if (!active) continue;
    const int m = min(kTile, range.y - j0);
    for (int t = (kMode == 1) ? max(0, i + 1 - j0) : 0; t < m; ++t) {
      if (kMode != 0 && tl[t] < 0) continue;   // only core points carry names
      if (!within(xi, yi, zi, tx[t], ty[t], tz[t], eps2)) continue;
      if (kMode == 0) ++count;
      else if (kMode == 1) best = uf_unite(parent, best, tl[t]);
      else best = min(best, tl[t]);
    }
  }
  if (!live) return;
  if (kMode == 0) {
    const int o = orig[i];
    const bool is_core = count >= min_samples;
    core[i] = is_core ? o : -1;
    if (is_core) parent[o] = o;
  } else if (kMode == 3) {
    const int name = mine >= 0 ? mine : (best == 0x7fffffff ? -1 : best);
    names[orig[i]] = name;
    if (name >= 0) {
      atomicAdd(st.count + name, 1u);
      const float v[3] = {p.x, p.y, p.z};
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const unsigned im = float_image(v[d]);
        atomicMin(st.lo + (int64_t)d * n_scan + name, im);
        atomicMax(st.hi + (int64_t)d * n_scan + name, im);
      }
    }
  }
}

// InstanceVoter.cluster_boxes for every name: kept (more than min_points points) clusters get a slot and a box.
__global__ __launch_bounds__(kBlock) void instance_boxes(int n, ClusterStats st, int min_points, float floor_lift, int max_boxes,
                                                         float* __restrict__ boxes, int* __restrict__ slot_of, int* __restrict__ k_raw,
                                                         int* __restrict__ k_dev, int* __restrict__ status) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  if (st.count[i] <= (unsigned)min_points) return;
  const int slot = atomicAdd(k_raw, 1);
  if (slot >= max_boxes) {
    atomicOr(status, 1);
    return;
  }
  atomicMax(k_dev, slot + 1);
  float lo[3], hi[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    lo[d] = image_float(st.lo[(int64_t)d * n + i]);
    hi[d] = image_float(st.hi[(int64_t)d * n + i]);
  }
  const float lifted = __fadd_rn(lo[2], floor_lift);     // the corners at z_min move up, in float32
  const bool flat = hi[2] == lo[2];
  const float z0 = fminf(lifted, hi[2]), z1 = fmaxf(lifted, hi[2]);
  const bool degenerate = flat || hi[0] == lo[0] || hi[1] == lo[1] || z1 == z0;
  float* b = boxes + (int64_t)slot * 6;
  b[0] = degenerate ? INFINITY : lo[0];
  b[1] = degenerate ? INFINITY : lo[1];
  b[2] = degenerate ? INFINITY : z0;
  b[3] = hi[0];
  b[4] = hi[1];
  b[5] = z1;
  slot_of[i] = slot;
}

constexpr int kMaxBoxFrames = 9;   // a voting window and the current frame

struct BoxFrames {
  const float* pts[kMaxBoxFrames];
  const uint8_t* labels[kMaxBoxFrames];
  int64_t n[kMaxBoxFrames];
  int64_t stride[kMaxBoxFrames];
  BoxPose pose[kMaxBoxFrames];
};

// box_vote with the box count read from device memory; blockIdx.y = frame of the window.
__global__ __launch_bounds__(kBlock) void box_vote_dev(BoxFrames fs, float clo0, float clo1, float clo2, float chi0, float chi1,
                                                       float chi2, const float* __restrict__ boxes, const int* __restrict__ k_dev,
                                                       int max_boxes, unsigned* __restrict__ counts) {
  extern __shared__ float lds_box[];
  const int K = min(*k_dev, max_boxes);
  if (K <= 0) return;
  for (int t = threadIdx.x; t < K * 6; t += blockDim.x) lds_box[t] = boxes[t];
  __syncthreads();
  const int f = blockIdx.y;
  const float* pts = fs.pts[f];
  const uint8_t* labels = fs.labels[f];
  const int64_t n = fs.n[f], stride = fs.stride[f];
  const bool identity = fs.pose[f].identity != 0;
  double m[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) m[k] = fs.pose[f].m[k];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const unsigned lab = labels[i];
    if (lab == 0 || lab > 2) continue;
    const float* row = pts + i * stride;
    float x = row[0], y = row[1], z = row[2];
    if (!identity) {
      const double dx = x, dy = y, dz = z;
      x = (float)pose_row_f64(m + 0, dx, dy, dz);
      y = (float)pose_row_f64(m + 4, dx, dy, dz);
      z = (float)pose_row_f64(m + 8, dx, dy, dz);
    }
    if (!((x > clo0) && (x < chi0) && (y > clo1) && (y < chi1) && (z > clo2) && (z < chi2))) continue;
    for (int k = 0; k < K; ++k) {
      const float* b = lds_box + k * 6;
      if (x >= b[0] && x <= b[3] && y >= b[1] && y <= b[4] && z >= b[2] && z <= b[5]) atomicAdd(counts + k * 3 + lab, 1u);
    }
  }
}

// labels[i] = 2 if 2 * n2 > n1 else 1 for every point whose cluster has a slot (the reference sums label VALUES)
__global__ __launch_bounds__(kBlock) void instance_apply(const int* __restrict__ names, const int* __restrict__ slot_of,
                                                         const unsigned* __restrict__ counts, const int* __restrict__ k_dev,
                                                         int max_boxes, int32_t* __restrict__ labels, int n) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int name = names[i];
  if (name < 0 || name >= n) return;
  const int slot = slot_of[name];
  if (slot < 0 || slot >= min(*k_dev, max_boxes)) return;
  const int c1 = (int)counts[slot * 3 + 1], c2 = (int)counts[slot * 3 + 2];
  labels[i] = 2 * c2 > c1 ? 2 : 1;
}

}  // namespace smos

using namespace smos;

namespace {
struct DbscanWork {
  size_t keys_in, keys_out, iota, orig, pos, sp, label, band, flag, cub, cub_bytes, total;
};

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

bool dbscan_layout(int64_t n, DbscanWork& w) {
  const size_t nn = (size_t)n, blocks = (nn + kBlock - 1) / kBlock;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off += up256(bytes); return at; };
  w.keys_in = take(nn * 4); w.keys_out = take(nn * 4); w.iota = take(nn * 4); w.orig = take(nn * 4); w.pos = take(nn * 4);
  w.sp = take(nn * 16); w.label = take(nn * 4); w.band = take(blocks * 8); w.flag = take(4);
  w.cub_bytes = 0;
  if (hipcub::DeviceRadixSort::SortPairs(nullptr, w.cub_bytes, (const float*)nullptr, (float*)nullptr, (const int*)nullptr,
                                         (int*)nullptr, (int)n) != hipSuccess)
    return false;
  w.cub = take(w.cub_bytes);
  w.total = off;
  return true;
}
}  // namespace

extern "C" int64_t smos_dbscan_work_bytes(int64_t n) {
  if (n <= 0 || n >= (1LL << 31)) return 0;
  DbscanWork w;
  return dbscan_layout(n, w) ? (int64_t)w.total : -1;
}

extern "C" int smos_dbscan(const float* pts, int64_t n, int64_t pt_stride, double eps, int32_t min_samples, int32_t* labels,
                           void* work, int64_t work_bytes, int32_t max_sweeps, smos_stream_t stream) {
  SMOS_REQUIRE(n >= 0 && n < (1LL << 31) && pt_stride >= 3 && eps > 0 && min_samples >= 1 && max_sweeps >= 1,
               "dbscan: bad arguments");
  if (n == 0) return SMOS_OK;
  SMOS_REQUIRE(pts && labels && work, "dbscan: null device pointer");
  DbscanWork w;
  SMOS_REQUIRE(dbscan_layout(n, w), "dbscan: sort workspace query failed");
  SMOS_REQUIRE(work_bytes >= (int64_t)w.total && (reinterpret_cast<uintptr_t>(work) & 255) == 0,
               "dbscan: workspace too small or not 256-byte aligned (%lld bytes needed)", (long long)w.total);
  hipStream_t s = (hipStream_t)stream;
  char* base = static_cast<char*>(work);
  float* keys_in = (float*)(base + w.keys_in);
  float* keys_out = (float*)(base + w.keys_out);
  int* iota = (int*)(base + w.iota);
  int* orig = (int*)(base + w.orig);
  int* pos = (int*)(base + w.pos);
  float4* sp = (float4*)(base + w.sp);
  int* core = (int*)(base + w.label);
  int2* band = (int2*)(base + w.band);
  int* flag = (int*)(base + w.flag);
  const double eps2 = eps * eps;
  const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
  hipLaunchKernelGGL(dbscan_keys, grid, block, 0, s, pts, (int)n, pt_stride, keys_in, iota);
  size_t cub_bytes = w.cub_bytes;
  if (hipcub::DeviceRadixSort::SortPairs(base + w.cub, cub_bytes, (const float*)keys_in, keys_out, (const int*)iota, orig, (int)n, 0,
                                         32, s) != hipSuccess) {
    set_error("dbscan: radix sort failed");
    return SMOS_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(dbscan_gather, grid, block, 0, s, pts, (int)n, pt_stride, (const int*)orig, (const float*)keys_out, eps, sp, pos, band);
  hipLaunchKernelGGL(dbscan_pass<0>, grid, block, 0, s, (const float4*)sp, (int)n, (const int2*)band, (const int*)orig, (const int*)pos,
                     eps2, (int)min_samples, core, (int*)nullptr, (int*)nullptr);
  // propagation sweeps; the "changed" flag is read back every kBatch sweeps (small inputs are latency-bound on that sync)
  constexpr int kBatch = 4;
  int sweeps = 0;
  for (;;) {
    if (hipMemsetAsync(flag, 0, sizeof(int), s) != hipSuccess) break;
    for (int k = 0; k < kBatch; ++k)
      hipLaunchKernelGGL(dbscan_pass<1>, grid, block, 0, s, (const float4*)sp, (int)n, (const int2*)band, (const int*)orig,
                         (const int*)pos, eps2, (int)min_samples, core, (int*)nullptr, flag);
    int host_flag = 0;
    if (hipMemcpyAsync(&host_flag, flag, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess) break;
    if (hipStreamSynchronize(s) != hipSuccess) break;
    if (!host_flag) {
      hipLaunchKernelGGL(dbscan_pass<2>, grid, block, 0, s, (const float4*)sp, (int)n, (const int2*)band, (const int*)orig,
                         (const int*)pos, eps2, (int)min_samples, core, labels, (int*)nullptr);
      return check_launch("dbscan");
    }
    sweeps += kBatch;
    if (sweeps >= max_sweeps) {
      set_error("dbscan: labels did not settle within %d sweeps", (int)max_sweeps);
      return SMOS_ERR_LAUNCH;
    }
  }
  return check_launch("dbscan");
}

extern "C" int smos_box_vote(const float* pts, int64_t n, int64_t pt_stride, const uint8_t* labels, const double* pose_diff,
                             const float* boxes, int32_t K, uint32_t* counts, smos_stream_t stream) {
  SMOS_REQUIRE(n >= 0 && pt_stride >= 3 && K >= 0 && K <= 2048, "box_vote: bad arguments (at most 2048 boxes)");
  if (n == 0 || K == 0) return SMOS_OK;
  SMOS_REQUIRE(pts && labels && boxes && counts, "box_vote: null device pointer");
  BoxPose p;
  p.identity = pose_diff ? 0 : 1;
  for (int i = 0; i < 12; ++i) p.m[i] = pose_diff ? pose_diff[i] : 0.0;
  // open crop interval with eps = 1e-4, bounds rounded to float32 as torch does (utils/transforms.py:155-157)
  const float clo[3] = {(float)(-50.0 + 1e-4), (float)(-50.0 + 1e-4), (float)(-4.0 + 1e-4)};
  const float chi[3] = {(float)(50.0 - 1e-4), (float)(50.0 - 1e-4), (float)(2.0 - 1e-4)};
  hipLaunchKernelGGL(box_vote, dim3(grid_for(n)), dim3(kBlock), (size_t)K * 6 * sizeof(float), (hipStream_t)stream, pts, n,
                     pt_stride, labels, p, clo[0], clo[1], clo[2], chi[0], chi[1], chi[2], boxes, (int)K, counts);
  return check_launch("box_vote");
}

namespace {
struct InstanceWork {
  size_t keys_in, keys_out, iota, orig, sp, core, parent, band, count, lo, hi, head, cub, cub_bytes, total;
};

bool instance_layout(int64_t n, InstanceWork& w) {
  const size_t nn = (size_t)n, blocks = (nn + kBlock - 1) / kBlock;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off += up256(bytes); return at; };
  w.keys_in = take(nn * 4); w.keys_out = take(nn * 4); w.iota = take(nn * 4); w.orig = take(nn * 4);
  w.sp = take(nn * 16); w.core = take(nn * 4); w.parent = take(nn * 4); w.band = take(blocks * 8);
  w.count = take(nn * 4); w.lo = take(nn * 12); w.hi = take(nn * 12);
  w.head = take(2 * sizeof(int));               // n_fg, clusters kept before the clamp
  // hipCUB's own query needs a device for all but the smallest inputs, and the size must be known without one: reserve
  // a bound (the alternate key / value buffers, per-block digit counters, histograms) and hold the library to it at
  // launch time (smos_instance_cluster).
  w.cub_bytes = nn * 24 + ((size_t)4 << 20);
  w.cub = take(w.cub_bytes);
  w.total = off;
  return true;
}
}  // namespace

extern "C" int64_t smos_instance_work_bytes(int64_t n) {
  if (n <= 0 || n >= (1LL << 31)) return 0;
  InstanceWork w;
  return instance_layout(n, w) ? (int64_t)w.total : -1;
}

extern "C" int smos_instance_cluster(const float* pts, int64_t n, int64_t pt_stride, const uint8_t* bf, double eps,
                                     int32_t min_samples, int32_t min_points, float floor_lift, int32_t max_boxes, int32_t* names,
                                     float* boxes, int32_t* slot_of, int32_t* k_dev, int32_t* status, void* work,
                                     int64_t work_bytes, smos_stream_t stream) {
  SMOS_REQUIRE(n >= 0 && n < (1LL << 31) && pt_stride >= 3 && eps > 0 && min_samples >= 1 && min_points >= 0,
               "instance_cluster: bad arguments");
  SMOS_REQUIRE(max_boxes >= 1 && max_boxes <= 2048, "instance_cluster: max_boxes must be in 1..2048, got %d", (int)max_boxes);
  SMOS_REQUIRE(k_dev && status, "instance_cluster: null device pointer");
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {                                  // no point, no cluster: the two result words, nothing else
    if (hipMemsetAsync(k_dev, 0, sizeof(int32_t), s) != hipSuccess || hipMemsetAsync(status, 0, sizeof(int32_t), s) != hipSuccess)
      return check_launch("instance_cluster");
    return SMOS_OK;
  }
  SMOS_REQUIRE(pts && bf && names && boxes && slot_of && work, "instance_cluster: null device pointer");
  InstanceWork w;
  SMOS_REQUIRE(instance_layout(n, w), "instance_cluster: sort workspace query failed");
  SMOS_REQUIRE(work_bytes >= (int64_t)w.total && (reinterpret_cast<uintptr_t>(work) & 255) == 0,
               "instance_cluster: workspace too small or not 256-byte aligned (%lld bytes needed)", (long long)w.total);
  char* base = static_cast<char*>(work);
  unsigned* keys_in = (unsigned*)(base + w.keys_in);
  unsigned* keys_out = (unsigned*)(base + w.keys_out);
  int* iota = (int*)(base + w.iota);
  int* orig = (int*)(base + w.orig);
  float4* sp = (float4*)(base + w.sp);
  int* core = (int*)(base + w.core);
  int* parent = (int*)(base + w.parent);
  int2* band = (int2*)(base + w.band);
  ClusterStats st;
  st.count = (unsigned*)(base + w.count);
  st.lo = (unsigned*)(base + w.lo);
  st.hi = (unsigned*)(base + w.hi);
  int* n_fg = (int*)(base + w.head);
  int* k_raw = n_fg + 1;
  const double eps2 = eps * eps;
  const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
  hipLaunchKernelGGL(instance_reset, dim3(1), dim3(kWave), 0, s, n_fg, k_raw, (int*)k_dev, (int*)status);
  hipLaunchKernelGGL(instance_keys, grid, block, 0, s, pts, (int)n, pt_stride, bf, keys_in, iota, n_fg, st, (int*)names, (int*)slot_of);
  size_t cub_bytes = 0;
  SMOS_REQUIRE(hipcub::DeviceRadixSort::SortPairs(nullptr, cub_bytes, (const unsigned*)keys_in, keys_out, (const int*)iota, orig,
                                                  (int)n, 0, 32, s) == hipSuccess && cub_bytes <= w.cub_bytes,
               "instance_cluster: the radix sort wants %lld bytes of scratch, %lld are reserved", (long long)cub_bytes,
               (long long)w.cub_bytes);
  if (hipcub::DeviceRadixSort::SortPairs(base + w.cub, cub_bytes, (const unsigned*)keys_in, keys_out, (const int*)iota, orig, (int)n,
                                         0, 32, s) != hipSuccess) {
    set_error("instance_cluster: radix sort failed");
    return SMOS_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(instance_gather, grid, block, 0, s, pts, (const int*)n_fg, pt_stride, (const int*)orig, (const unsigned*)keys_out,
                     eps, sp, band);
#define SMOS_INSTANCE_PASS(mode)                                                                                              \
  hipLaunchKernelGGL(instance_pass<mode>, grid, block, 0, s, (const float4*)sp, (const int*)n_fg, (const int2*)band,          \
                     (const int*)orig, eps2, (int)min_samples, core, parent, (int*)names, st, (int)n)
  SMOS_INSTANCE_PASS(0);
  SMOS_INSTANCE_PASS(1);
  SMOS_INSTANCE_PASS(2);
  SMOS_INSTANCE_PASS(3);
#undef SMOS_INSTANCE_PASS
  hipLaunchKernelGGL(instance_boxes, grid, block, 0, s, (int)n, st, (int)min_points, floor_lift, (int)max_boxes, boxes, (int*)slot_of,
                     k_raw, (int*)k_dev, (int*)status);
  return check_launch("instance_cluster");
}

extern "C" int smos_box_vote_dev(int32_t count, const float* const* pts, const int64_t* n, const int64_t* pt_stride,
                                 const uint8_t* const* labels, const double* const* pose_diff, const float* boxes,
                                 const int32_t* k_dev, int32_t max_boxes, uint32_t* counts, smos_stream_t stream) {
  SMOS_REQUIRE(count >= 0 && (count == 0 || (pts && n && pt_stride && labels && pose_diff)), "box_vote_dev: null array");
  SMOS_REQUIRE(max_boxes >= 1 && max_boxes <= 2048, "box_vote_dev: max_boxes must be in 1..2048, got %d", (int)max_boxes);
  int64_t total = 0;
  for (int f = 0; f < count; ++f) {
    SMOS_REQUIRE(n[f] >= 0 && pt_stride[f] >= 3, "box_vote_dev: bad sizes in frame %d (n=%lld stride=%lld)", f, (long long)n[f],
                 (long long)pt_stride[f]);
    SMOS_REQUIRE(n[f] == 0 || (pts[f] && labels[f]), "box_vote_dev: null device pointer in frame %d", f);
    total += n[f];
  }
  if (total == 0) return SMOS_OK;
  SMOS_REQUIRE(boxes && k_dev && counts, "box_vote_dev: null device pointer");
  const float clo[3] = {(float)(-50.0 + 1e-4), (float)(-50.0 + 1e-4), (float)(-4.0 + 1e-4)};   // as smos_box_vote
  const float chi[3] = {(float)(50.0 - 1e-4), (float)(50.0 - 1e-4), (float)(2.0 - 1e-4)};
  for (int f = 0; f < count;) {
    BoxFrames fs;
    int m = 0;
    int64_t longest = 0;
    for (; f < count && m < kMaxBoxFrames; ++f) {
      if (n[f] == 0) continue;
      fs.pts[m] = pts[f];
      fs.labels[m] = labels[f];
      fs.n[m] = n[f];
      fs.stride[m] = pt_stride[f];
      fs.pose[m].identity = pose_diff[f] ? 0 : 1;
      for (int i = 0; i < 12; ++i) fs.pose[m].m[i] = pose_diff[f] ? pose_diff[f][i] : 0.0;
      longest = n[f] > longest ? n[f] : longest;
      ++m;
    }
    if (m == 0) continue;
    for (int k = m; k < kMaxBoxFrames; ++k) {    // unused entries: defined, never indexed (gridDim.y = m)
      fs.pts[k] = nullptr; fs.labels[k] = nullptr; fs.n[k] = 0; fs.stride[k] = 0; fs.pose[k] = fs.pose[0];
    }
    hipLaunchKernelGGL(box_vote_dev, dim3(grid_for(longest), m), dim3(kBlock), (size_t)max_boxes * 6 * sizeof(float),
                       (hipStream_t)stream, fs, clo[0], clo[1], clo[2], chi[0], chi[1], chi[2], boxes, (const int*)k_dev,
                       (int)max_boxes, counts);
    if (int rc = check_launch("box_vote_dev")) return rc;
  }
  return SMOS_OK;
}

extern "C" int smos_instance_apply(const int32_t* names, const int32_t* slot_of, const uint32_t* counts, const int32_t* k_dev,
                                   int32_t max_boxes, int32_t* labels, int64_t n, smos_stream_t stream) {
  SMOS_REQUIRE(n >= 0 && n < (1LL << 31), "instance_apply: bad point count %lld", (long long)n);
  SMOS_REQUIRE(max_boxes >= 1 && max_boxes <= 2048, "instance_apply: max_boxes must be in 1..2048, got %d", (int)max_boxes);
  if (n == 0) return SMOS_OK;
  SMOS_REQUIRE(names && slot_of && counts && k_dev && labels, "instance_apply: null device pointer");
  hipLaunchKernelGGL(instance_apply, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                     (const int*)names, (const int*)slot_of, (const unsigned*)counts, (const int*)k_dev, (int)max_boxes, labels, (int)n);
  return check_launch("instance_apply");
}
