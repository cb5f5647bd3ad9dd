// Training loss of AttNet on the device for gfx950: OHEM cross-entropy + lovasz_weight * Lovasz-softmax as one
// differentiable value.  Replaces the chain of refapi/models/losses.py (utils/criterion.py:10-28 and
// utils/lovasz_losses.py:147-222 of the reference): softmax, mask compaction, a sort per class, two cumulative sums, a
// top-k -- and up to five host reads of device values -- by
//
//   seg_prep      one pass over logits and labels: log-softmax, CE, err_c = |[y == c] - p_c|, one 33-bit sort key per
//                 (segment, position) and the position as payload; C class segments + the CE segment
//   radix sort    ONE hipcub::DeviceRadixSort::SortPairs over all segments, bits [0, 33) (stable: ties by position)
//   seg_count     foreground count of every 2048-element tile of the sorted class segments
//   seg_tilescan  exclusive scan of the tile counts (one block per class) + the foreground total G
//   seg_apply     per tile: the prefix counts F_i, from them the Lovasz coefficient d_i in closed form
//                     foreground  d_i = 1 / U_i                      I_i = G - F_i, U_i = G + (i + 1 - F_i)
//                     background  d_i = I_i / ((U_i - 1) * U_i)      (= jac_i - jac_{i-1} of _lovasz_grad, i = 0 included)
//                 written to coef[c, position]; the tile's sum of err_i * d_i; in the CE segment the top-k flag and the
//                 tile's share of the top-k sum
//   seg_finish    the scalar: mean over the present classes (G > 0), mean CE, top_weight * top-k mean
//
// and one backward launch (seg_bwd) that recomputes the softmax.  No block waits for another (the scan is three launches),
// no float atomics (tile partials are float64, summed in a fixed order), nothing is read back.  The counts are integers and
// d_i is formed in float64 from them and rounded once, so the cancellation of `jac[1:] - jac[:-1]` in float32 is gone.
//
// Key: (segment << 31) | (MAX - bits(v)) with MAX = bits(1.0f) in a class segment (err <= 1) and bits(+inf) in the CE
// segment: larger values first.  bits(v) is clamped to [0, MAX] first, so whatever the logits hold (NaN, Inf) the key stays
// inside its segment and each segment of the sorted array holds exactly n entries; a class key of an ignored position is
// MAX + 1, behind every real one.  The sorted values are recovered from the keys; a NaN reaches the result through the CE
// mean, which seg_prep sums from the unclamped values.
#include "smos_common.h"
#include <hipcub/hipcub.hpp>

namespace smos {

constexpr int kSegItems = 8;                    // elements per thread of a scan tile
constexpr int kSegTile = kBlock * kSegItems;    // 2048
constexpr int kSegWaves = kBlock / kWave;
constexpr uint32_t kOneBits = 0x3F800000u;      // bits(1.0f)
constexpr uint32_t kInfBits = 0x7F800000u;      // bits(+inf)
constexpr int kSegKeyBits = 33;                 // 31 value bits + 2 segment bits
constexpr int kPrepGrid = 1024;                 // fixed: the order of the CE partial sums does not depend on the device

struct SegGeom {
  int64_t sb, sc, sp;   // element strides of pred / grad [B, C, P]
  int64_t P;
  int n;                // B * P
};

struct SegWork {
  size_t keys_in, keys_out, vals_in, vals_out, lab, tile_cnt, tile_off, fg_total, part, ce_part, cub, cub_bytes, total;
  int tiles;
};

static bool seg_layout(int64_t n, int C, SegWork& w) {
  const size_t S = (size_t)C + 1, nn = (size_t)n;
  w.tiles = (int)((n + kSegTile - 1) / kSegTile);
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) & ~(size_t)255; return at; };
  w.keys_in = take(S * nn * 8); w.keys_out = take(S * nn * 8); w.vals_in = take(S * nn * 4); w.vals_out = take(S * nn * 4);
  w.lab = take(nn);
  w.tile_cnt = take((size_t)C * w.tiles * 4); w.tile_off = take((size_t)C * w.tiles * 4); w.fg_total = take(4 * 4);
  w.part = take(S * w.tiles * 8); w.ce_part = take((size_t)kPrepGrid * 8);
  w.cub_bytes = 0;
  if (hipcub::DeviceRadixSort::SortPairs(nullptr, w.cub_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr,
                                         (uint32_t*)nullptr, (int)(S * nn), 0, kSegKeyBits) != hipSuccess)
    return false;
  w.cub = take(w.cub_bytes);
  w.total = off;
  return true;
}

// sum over the block in a fixed order; every thread gets it
__device__ __forceinline__ double seg_block_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// softmax of one position in float32; forward and backward share it, so the backward sees the forward's p to the bit
template <int C>
__device__ __forceinline__ void seg_softmax(const float (&x)[C], float (&p)[C], float& lse) {
  float m = x[0];
#pragma unroll
  for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
  float e[C], s = 0.0f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    e[c] = expf(x[c] - m);
    s += e[c];
  }
  const float inv = 1.0f / s;
#pragma unroll
  for (int c = 0; c < C; ++c) p[c] = e[c] * inv;
  lse = m + logf(s);
}

__device__ __forceinline__ uint32_t seg_key(float v, uint32_t top) {
  uint32_t u = __float_as_uint(v) & 0x7FFFFFFFu;
  u = u > top ? top : u;
  return top - u;
}

template <int C>
__global__ __launch_bounds__(kBlock) void seg_prep(const float* __restrict__ pred, const int64_t* __restrict__ target, SegGeom g,
                                                   int64_t ignore, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                   uint8_t* __restrict__ lab, double* __restrict__ ce_part) {
  __shared__ double sh[kBlock];
  double ce_sum = 0.0;
  for (int q = blockIdx.x * kBlock + threadIdx.x; q < g.n; q += gridDim.x * kBlock) {
    const int64_t b = q / g.P, p = q - b * g.P;
    const float* __restrict__ src = pred + b * g.sb + p * g.sp;
    float x[C], pr[C], lse;
#pragma unroll
    for (int c = 0; c < C; ++c) x[c] = src[c * g.sc];
    const int64_t t = target[q];
    const bool ign = t == ignore || t < 0 || t >= C;
    const int y = ign ? 0 : (int)t;
    seg_softmax<C>(x, pr, lse);
    float xy = x[0];
#pragma unroll
    for (int c = 1; c < C; ++c) xy = y == c ? x[c] : xy;
    const float ce = ign ? 0.0f : lse - xy;
    ce_sum += (double)ce;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float err = fabsf((y == c ? 1.0f : 0.0f) - pr[c]);
      const uint32_t k = ign ? kOneBits + 1u : seg_key(err, kOneBits);
      keys[(size_t)c * g.n + q] = ((uint64_t)c << 31) | k;
      vals[(size_t)c * g.n + q] = (uint32_t)q;
    }
    keys[(size_t)C * g.n + q] = ((uint64_t)C << 31) | seg_key(ce, kInfBits);
    vals[(size_t)C * g.n + q] = (uint32_t)q;
    lab[q] = ign ? (uint8_t)255 : (uint8_t)y;
  }
  const double total = seg_block_sum(ce_sum, sh);
  if (threadIdx.x == 0) ce_part[blockIdx.x] = total;
}

// One tile element: its sorted key and position (index clamped, loaded unconditionally), the label of the position.
struct SegItem {
  uint32_t low;   // key without the segment field
  uint32_t pos;
  bool in, fg;
};

__device__ __forceinline__ SegItem seg_item(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                            const uint8_t* __restrict__ lab, int n, int seg, int i, bool class_seg) {
  SegItem it;
  it.in = i < n;
  const size_t at = (size_t)seg * n + (it.in ? i : n - 1);
  it.low = (uint32_t)keys[at] & 0x7FFFFFFFu;
  const uint32_t pos = vals[at];
  it.pos = pos < (uint32_t)n ? pos : (uint32_t)(n - 1);
  const int l = lab[it.pos];
  it.fg = it.in && class_seg && it.low <= kOneBits && l == seg;
  return it;
}

// grid (tiles, C): foreground count of each tile of the sorted class segments
__global__ __launch_bounds__(kBlock) void seg_count(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                    const uint8_t* __restrict__ lab, int n, int tiles, int* __restrict__ tile_cnt) {
  __shared__ int wave_cnt[kSegWaves];
  const int seg = blockIdx.y, wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < kSegItems; ++j) {
    const SegItem it = seg_item(keys, vals, lab, n, seg, blockIdx.x * kSegTile + j * kBlock + (int)threadIdx.x, true);
    cnt += __popcll(__ballot(it.fg));
  }
  if (lane == 0) wave_cnt[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int w = 0; w < kSegWaves; ++w) total += wave_cnt[w];
    tile_cnt[seg * tiles + blockIdx.x] = total;
  }
}

// grid (C): exclusive scan of a class's tile counts, 256 tiles per round; fg_total[c] = G
__global__ __launch_bounds__(kBlock) void seg_tilescan(const int* __restrict__ tile_cnt, int tiles, int* __restrict__ tile_off,
                                                       int* __restrict__ fg_total) {
  __shared__ int wave_sum[kSegWaves];
  const int seg = blockIdx.x, wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  int carry = 0;
  for (int base = 0; base < tiles; base += kBlock) {
    const int t = base + threadIdx.x;
    const int v = t < tiles ? tile_cnt[seg * tiles + t] : 0;
    int incl = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int up = __shfl_up(incl, o, kWave);
      incl += lane >= o ? up : 0;
    }
    if (lane == kWave - 1) wave_sum[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < kSegWaves; ++w) {
      before += w < wave ? wave_sum[w] : 0;
      all += wave_sum[w];
    }
    if (t < tiles) tile_off[seg * tiles + t] = carry + before + incl - v;
    carry += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) fg_total[seg] = carry;
}

// grid (tiles, C + 1): coefficients, top-k flags and the tile partial sums
__global__ __launch_bounds__(kBlock) void seg_apply(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                    const uint8_t* __restrict__ lab, int n, int tiles, int C, int64_t k,
                                                    const int* __restrict__ tile_off, const int* __restrict__ fg_total,
                                                    float* __restrict__ coef, double* __restrict__ part) {
  __shared__ int cnt[kSegItems * kSegWaves];
  __shared__ double sh[kBlock];
  const int seg = blockIdx.y, wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const bool class_seg = seg < C;
  SegItem it[kSegItems];
  int in_wave[kSegItems];
#pragma unroll
  for (int j = 0; j < kSegItems; ++j) {
    it[j] = seg_item(keys, vals, lab, n, seg, blockIdx.x * kSegTile + j * kBlock + (int)threadIdx.x, class_seg);
    const unsigned long long mask = __ballot(it[j].fg);
    in_wave[j] = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) cnt[j * kSegWaves + wave] = __popcll(mask);
  }
  __syncthreads();
  const int G = class_seg ? fg_total[seg] : 0;
  int before = class_seg ? tile_off[seg * tiles + blockIdx.x] : 0;   // foreground elements in front of the tile
  double sum = 0.0;
  float* __restrict__ dst = coef + (size_t)seg * n;
#pragma unroll
  for (int j = 0; j < kSegItems; ++j) {
    int row = 0;                                                      // ... and in front of this wave's row j of the tile
    for (int w = 0; w < kSegItems * kSegWaves; ++w) row += w < j * kSegWaves + wave ? cnt[w] : 0;
    const int i = blockIdx.x * kSegTile + j * kBlock + (int)threadIdx.x;
    float d, v;
    if (class_seg) {
      const bool valid = it[j].in && it[j].low <= kOneBits;           // an ignored position: behind every real one
      const int F = before + row + in_wave[j] + (it[j].fg ? 1 : 0);   // foreground among the sorted elements 0..i
      const double U = (double)G + (double)(i + 1 - F);
      const double I = (double)(G - F);
      const double dd = it[j].fg ? 1.0 / U : I / ((U - 1.0) * U);
      d = valid && G > 0 ? (float)dd : 0.0f;
      v = __uint_as_float(kOneBits - (valid ? it[j].low : kOneBits));
      sum += (double)v * (double)d;
    } else {
      const bool top = i < k;
      d = top ? 1.0f : 0.0f;
      v = __uint_as_float(kInfBits - it[j].low);
      sum += top ? (double)v : 0.0;
    }
    if (it[j].in) dst[it[j].pos] = d;
  }
  const double total = seg_block_sum(sum, sh);
  if (threadIdx.x == 0) part[seg * tiles + blockIdx.x] = total;
}

// one block: stats[0] = 1 / present classes (0 when none), loss
__global__ __launch_bounds__(kBlock) void seg_finish(const double* __restrict__ part, const double* __restrict__ ce_part,
                                                     const int* __restrict__ fg_total, int tiles, int C, int n, int64_t k,
                                                     float top_weight, float lovasz_weight, float* __restrict__ loss,
                                                     float* __restrict__ stats) {
  __shared__ double sh[kBlock];
  double seg_sum[4];
  for (int s = 0; s <= C; ++s) {
    double v = 0.0;
    for (int t = threadIdx.x; t < tiles; t += kBlock) v += part[s * tiles + t];
    seg_sum[s] = seg_block_sum(v, sh);
  }
  double v = 0.0;
  for (int t = threadIdx.x; t < kPrepGrid; t += kBlock) v += ce_part[t];
  const double ce_total = seg_block_sum(v, sh);
  if (threadIdx.x == 0) {
    int present = 0;
    double lov = 0.0;
    for (int c = 0; c < C; ++c) {
      const bool has = fg_total[c] > 0;
      present += has ? 1 : 0;
      lov += has ? seg_sum[c] : 0.0;
    }
    const double inv_present = present > 0 ? 1.0 / (double)present : 0.0;
    const double ohem = ce_total / (double)n + (double)top_weight * seg_sum[C] / (double)k;
    loss[0] = (float)(ohem + (double)lovasz_weight * lov * inv_present);
    stats[0] = (float)inv_present;
    stats[1] = (float)present;
  }
}

template <int C>
__global__ __launch_bounds__(kBlock) void seg_bwd(const float* __restrict__ pred, const int64_t* __restrict__ target, SegGeom g,
                                                  SegGeom gg, int64_t ignore, const float* __restrict__ coef,
                                                  const float* __restrict__ stats, const float* __restrict__ grad_out, float w_mean,
                                                  float w_top, float lovasz_weight, float* __restrict__ grad) {
  const float go = grad_out[0];
  const float w_lov = go * lovasz_weight * stats[0];
  for (int q = blockIdx.x * kBlock + threadIdx.x; q < g.n; q += gridDim.x * kBlock) {
    const int64_t b = q / g.P, p = q - b * g.P;
    const float* __restrict__ src = pred + b * g.sb + p * g.sp;
    float x[C], pr[C], cf[C], lse;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      x[c] = src[c * g.sc];
      cf[c] = coef[(size_t)c * g.n + q];
    }
    const float top = coef[(size_t)C * g.n + q];
    const int64_t t = target[q];
    const bool ign = t == ignore || t < 0 || t >= C;
    const int y = ign ? 0 : (int)t;
    seg_softmax<C>(x, pr, lse);
    const float w_ce = go * (w_mean + w_top * top);
    float tc[C], tsum = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      tc[c] = (y == c ? -cf[c] : cf[c]) * pr[c];
      tsum += tc[c];
    }
    float* __restrict__ dst = grad + b * gg.sb + p * gg.sp;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float v = w_ce * (pr[c] - (y == c ? 1.0f : 0.0f)) + w_lov * (tc[c] - pr[c] * tsum);
      dst[c * gg.sc] = ign ? 0.0f : v;
    }
  }
}

}  // namespace smos

using namespace smos;

extern "C" int32_t smos_seg_loss_tile(void) { return kSegTile; }

extern "C" int64_t smos_seg_loss_work_bytes(int64_t n, int32_t C) {
  if (n <= 0 || (C != 2 && C != 3) || n * (C + 1) >= (1LL << 30)) return 0;
  SegWork w;
  return seg_layout(n, C, w) ? (int64_t)w.total : 0;
}

extern "C" int smos_seg_loss_fwd(const float* pred, const int64_t* pred_stride, const int64_t* target, int64_t B, int32_t C,
                                 int64_t P, int64_t k, float top_weight, float lovasz_weight, int64_t ignore_index, float* coef,
                                 float* loss, float* stats, void* work, int64_t work_bytes, smos_stream_t stream) {
  SMOS_REQUIRE(C == 2 || C == 3, "seg_loss: %d classes; the kernels are built for 2 and 3", (int)C);
  SMOS_REQUIRE(B > 0 && P > 0 && B * P * (C + 1) < (1LL << 30), "seg_loss: bad sizes B=%lld P=%lld", (long long)B, (long long)P);
  SMOS_REQUIRE(k >= 1 && k <= B * P, "seg_loss: top-k size %lld outside [1, %lld]", (long long)k, (long long)(B * P));
  SMOS_REQUIRE(pred && pred_stride && target && coef && loss && stats && work, "seg_loss: null pointer");
  SegWork w;
  const int n = (int)(B * P);
  SMOS_REQUIRE(seg_layout(n, C, w) && (int64_t)w.total <= work_bytes, "seg_loss: the workspace holds %lld bytes, %lld are needed",
               (long long)work_bytes, (long long)w.total);
  SegGeom g;
  g.sb = pred_stride[0]; g.sc = pred_stride[1]; g.sp = pred_stride[2]; g.P = P; g.n = n;
  hipStream_t s = (hipStream_t)stream;
  char* base = (char*)work;
  uint64_t* keys_in = (uint64_t*)(base + w.keys_in);
  uint64_t* keys_out = (uint64_t*)(base + w.keys_out);
  uint32_t* vals_in = (uint32_t*)(base + w.vals_in);
  uint32_t* vals_out = (uint32_t*)(base + w.vals_out);
  uint8_t* lab = (uint8_t*)(base + w.lab);
  int* tile_cnt = (int*)(base + w.tile_cnt);
  int* tile_off = (int*)(base + w.tile_off);
  int* fg_total = (int*)(base + w.fg_total);
  double* part = (double*)(base + w.part);
  double* ce_part = (double*)(base + w.ce_part);

  if (C == 2)
    hipLaunchKernelGGL((seg_prep<2>), dim3(kPrepGrid), dim3(kBlock), 0, s, pred, target, g, ignore_index, keys_in, vals_in, lab, ce_part);
  else
    hipLaunchKernelGGL((seg_prep<3>), dim3(kPrepGrid), dim3(kBlock), 0, s, pred, target, g, ignore_index, keys_in, vals_in, lab, ce_part);
  int rc = check_launch("seg_loss prep");
  if (rc != SMOS_OK) return rc;
  size_t cub_bytes = w.cub_bytes;
  if (hipcub::DeviceRadixSort::SortPairs(base + w.cub, cub_bytes, (const uint64_t*)keys_in, keys_out, (const uint32_t*)vals_in, vals_out,
                                         (int)((size_t)(C + 1) * n), 0, kSegKeyBits, s) != hipSuccess) {
    set_error("seg_loss: radix sort failed");
    return SMOS_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(seg_count, dim3(w.tiles, C), dim3(kBlock), 0, s, keys_out, vals_out, lab, n, w.tiles, tile_cnt);
  hipLaunchKernelGGL(seg_tilescan, dim3(C), dim3(kBlock), 0, s, tile_cnt, w.tiles, tile_off, fg_total);
  hipLaunchKernelGGL(seg_apply, dim3(w.tiles, C + 1), dim3(kBlock), 0, s, keys_out, vals_out, lab, n, w.tiles, (int)C, k, tile_off,
                     fg_total, coef, part);
  hipLaunchKernelGGL(seg_finish, dim3(1), dim3(kBlock), 0, s, part, ce_part, fg_total, w.tiles, (int)C, n, k, top_weight,
                     lovasz_weight, loss, stats);
  return check_launch("seg_loss_fwd");
}

extern "C" int smos_seg_loss_bwd(const float* pred, const int64_t* pred_stride, const int64_t* target, const float* coef,
                                 const float* stats, const float* grad_out, int64_t B, int32_t C, int64_t P, int64_t k,
                                 float top_weight, float lovasz_weight, int64_t ignore_index, float* grad,
                                 const int64_t* grad_stride, smos_stream_t stream) {
  SMOS_REQUIRE(C == 2 || C == 3, "seg_loss_bwd: %d classes; the kernels are built for 2 and 3", (int)C);
  SMOS_REQUIRE(B > 0 && P > 0 && B * P * (C + 1) < (1LL << 30), "seg_loss_bwd: bad sizes B=%lld P=%lld", (long long)B, (long long)P);
  SMOS_REQUIRE(k >= 1 && k <= B * P, "seg_loss_bwd: top-k size %lld outside [1, %lld]", (long long)k, (long long)(B * P));
  SMOS_REQUIRE(pred && pred_stride && target && coef && stats && grad_out && grad && grad_stride, "seg_loss_bwd: null pointer");
  SegGeom g, gg;
  const int n = (int)(B * P);
  g.sb = pred_stride[0]; g.sc = pred_stride[1]; g.sp = pred_stride[2]; g.P = P; g.n = n;
  gg.sb = grad_stride[0]; gg.sc = grad_stride[1]; gg.sp = grad_stride[2]; gg.P = P; gg.n = n;
  const float w_mean = (float)(1.0 / (double)n), w_top = (float)((double)top_weight / (double)k);
  hipStream_t s = (hipStream_t)stream;
  const dim3 gr(grid_for(n, kBlock, kMaxGrid));
  if (C == 2)
    hipLaunchKernelGGL((seg_bwd<2>), gr, dim3(kBlock), 0, s, pred, target, g, gg, ignore_index, coef, stats, grad_out, w_mean, w_top,
                       lovasz_weight, grad);
  else
    hipLaunchKernelGGL((seg_bwd<3>), gr, dim3(kBlock), 0, s, pred, target, g, gg, ignore_index, coef, stats, grad_out, w_mean, w_top,
                       lovasz_weight, grad);
  return check_launch("seg_loss_bwd");
}
