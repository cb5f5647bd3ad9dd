// Fixed-order ("store and sum") backward of the two operators whose gradients are otherwise summed with float atomics:
// the grid gradient of the bilinear gather (smos_bilinear_gather_bwd_det) and grad_value of multi-scale deformable
// attention (smos_msda_bwd_det).  Both have one structure: a destination row of C floats is the sum, over the (source, tap)
// PAIRS that reach it, of a scalar weight times a source row of grad_out.  Three steps, no atomics on the data:
//
//   emit   one pass per operator writes, for every pair in its natural order, a 32-bit key (the destination row id; an
//          absent pair gets the sentinel R = one past the last row), the pair index as the payload and the pair's weight
//          into a table indexed by pair;
//   sort   ONE stable hipcub::DeviceRadixSort::SortPairs over the significant bits of R: the pairs of a destination end up
//          next to each other in ascending pair index;
//   sum    segsum_starts finds where every destination's pairs begin (a binary search per row), segsum_rows adds them up.
//
// The sum is a defined float32 number.  For a destination with terms t_0 .. t_{m-1} in ascending pair index,
// t_j[c] = __fmul_rn(w_j, src_j[c]); the terms are cut into chunks of kSegL consecutive terms; a chunk is summed left to
// right starting from its first term (__fadd_rn, no FMA); the chunk partials are added left to right in chunk order.  A
// destination without a term is exactly 0.  Nothing here depends on the grid, on the device or on a previous call.
// segsum_rows walks the chunks of one destination on one lane group; since the chunk rule fixes the number, a later kernel
// may give the chunks of a much-hit destination to several waves without changing a bit.
//
// Lane = channel: a group of kG lanes owns a destination row.  Lane j of the group also owns the bookkeeping of term
// j0 + j of the current batch (pair, weight, source offset), handed to the group by wave shuffles.  The trip counts are
// those of the busiest group of the wave and every load is unconditional: a lane without a term, a row or a channel reads
// a clamped address and its value is dropped by a select.
#include <hipcub/hipcub.hpp>

#include "bilinear_taps.h"
#include "smos_common.h"

namespace smos {

constexpr int kSegL = 64;   // terms per chunk: one bookkeeping batch of a full-wave group

struct SumGeom {
  int64_t ds_b, ds_c, ds_h, ds_w;  // destination strides; row r = (b * H + y) * W + x
  int64_t ss_b, ss_n, ss_c;        // source strides; source row = b * Nn + n = pair / div
  uint32_t HW, W;
  uint32_t Nn, div;
  int C;
};

struct SegWork {
  size_t keys_in, keys_out, vals_in, vals_out, wt, start, rows, cub, cub_bytes, total;
  int bits;
};

// pairs: number of (source, tap) pairs, R: destination rows, row_floats: floats of a dense copy of the source (0: none)
static void segsum_layout(int64_t pairs, int64_t R, int64_t row_floats, SegWork& w) {
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) & ~(size_t)255; return at; };
  const size_t np = (size_t)pairs;
  w.keys_in = take(np * 4); w.keys_out = take(np * 4); w.vals_in = take(np * 4); w.vals_out = take(np * 4);
  w.wt = take(np * 4);
  w.start = take(((size_t)R + 1) * 4);
  w.rows = take((size_t)row_floats * 4);
  w.bits = 1;
  while (w.bits < 32 && ((uint64_t)R >> w.bits) != 0) ++w.bits;      // the sentinel R is the largest key
  // The sort's scratch from the sizes alone (the library's own query asks the device for its tuning and fails on a host
  // without one): a second copy of keys and values, 4 bytes of decoupled look-back state per item -- 256 digit counters per
  // block of at least 256 items -- and 64 KiB for histograms and counters.  segsum_run checks the library's figure against it.
  w.cub_bytes = np * 12 + 65536;
  w.cub = take(w.cub_bytes);
  w.total = off;
}

// ---- emit ----
// One thread per point: the four taps of make_taps on a dense map (gs_h = W, gs_w = 1), so a tap's offset is its pixel.
__global__ __launch_bounds__(kBlock) void bil_emit(const float* __restrict__ coord, BilGeom g, int64_t total, int64_t N,
                                                   uint32_t R, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                   float* __restrict__ wt) {
  const uint32_t hw = (uint32_t)g.H * (uint32_t)g.W;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < total; base += (int64_t)gridDim.x * blockDim.x) {
    const bool has = base + threadIdx.x < total;
    const int64_t i = has ? base + threadIdx.x : total - 1;
    const uint32_t b = (uint32_t)(i / N);
    const Taps t = make_taps(coord + i * g.K, g);
    uint32_t k[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = t.o[j] >= 0 ? b * hw + (uint32_t)t.o[j] : R;
    if (has) {
      const uint32_t p0 = (uint32_t)i * 4u;
      reinterpret_cast<uint4*>(keys)[i] = make_uint4(k[0], k[1], k[2], k[3]);
      reinterpret_cast<uint4*>(vals)[i] = make_uint4(p0, p0 + 1, p0 + 2, p0 + 3);
      reinterpret_cast<float4*>(wt)[i] = make_float4(t.w[0], t.w[1], t.w[2], t.w[3]);
    }
  }
}

// grad_sampling_loc and grad_attn_weight with the arithmetic of msda_bwd (csrc/msda.hip) -- the same expressions in the
// same order, so the same bits -- and, in place of its atomic adds, the four pairs of every sample: corner o1..o4, key
// (b * S + lsi[l] + y * W + x) * M + m, weight (wy * wx) * attn.
template <int kGroup>
__global__ __launch_bounds__(kBlock) void msda_bwd_emit(const float* __restrict__ grad_out, const float* __restrict__ value,
                                                        const int64_t* __restrict__ shapes, const int64_t* __restrict__ lsi,
                                                        const float* __restrict__ loc, const float* __restrict__ attn,
                                                        float* __restrict__ grad_loc, float* __restrict__ grad_attn,
                                                        uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                        float* __restrict__ wt, uint32_t R, int64_t n_heads_total, int S, int M,
                                                        int D, int L, int Lq, int P) {
  using T = float;
  constexpr int kGroups = kBlock / kGroup;
  const int lane = threadIdx.x % kGroup;
  const int64_t wstride = (int64_t)M * D;
  for (int64_t hq = (int64_t)blockIdx.x * kGroups + threadIdx.x / kGroup; hq < n_heads_total;
       hq += (int64_t)gridDim.x * kGroups) {
    const int m = (int)(hq % M);
    const int64_t b = hq / ((int64_t)M * Lq);
    int64_t wptr = hq * L * P;
    for (int l = 0; l < L; ++l) {
      const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
      const int64_t base = (b * S + lsi[l]) * wstride + (int64_t)m * D;
      const int64_t row0 = b * S + lsi[l];
      for (int p = 0; p < P; ++p, ++wptr) {
        const T loc_w = loc[2 * wptr], loc_h = loc[2 * wptr + 1], aw = attn[wptr];
        const T h_im = loc_h * H - (T)0.5, w_im = loc_w * W - (T)0.5;
        T g_w = 0, g_h = 0, g_a = 0;
        uint32_t key = R;
        float pw = 0.0f;
        if (h_im > -1 && w_im > -1 && h_im < H && w_im < W) {
          const int h_low = (int)floor(h_im), w_low = (int)floor(w_im);
          const int h_high = h_low + 1, w_high = w_low + 1;
          const T lh = h_im - h_low, lw = w_im - w_low, hh = 1 - lh, hw = 1 - lw;
          const bool t = h_low >= 0, bt = h_high <= H - 1, lf = w_low >= 0, rt = w_high <= W - 1;
          const int64_t o1 = base + ((int64_t)h_low * W + w_low) * wstride, o2 = o1 + wstride;
          const int64_t o3 = o1 + (int64_t)W * wstride, o4 = o3 + wstride;
          if (lane < 4) {
            const bool down = lane >> 1, right = lane & 1;
            const bool in = (down ? bt : t) && (right ? rt : lf);
            const int y = h_low + (down ? 1 : 0), x = w_low + (right ? 1 : 0);
            key = in ? (uint32_t)((row0 + (int64_t)y * W + x) * M + m) : R;
            pw = in ? __fmul_rn(__fmul_rn(down ? lh : hh, right ? lw : hw), aw) : 0.0f;
          }
          for (int c = lane; c < D; c += kGroup) {
            const T top = grad_out[hq * D + c];
            const T tgv = top * aw;
            T gh = 0, gw = 0, val = 0;
            if (t && lf) {
              const T v = value[o1 + c];
              gh -= hw * v; gw -= hh * v; val += hh * hw * v;
            }
            if (t && rt) {
              const T v = value[o2 + c];
              gh -= lw * v; gw += hh * v; val += hh * lw * v;
            }
            if (bt && lf) {
              const T v = value[o3 + c];
              gh += hw * v; gw -= lh * v; val += lh * hw * v;
            }
            if (bt && rt) {
              const T v = value[o4 + c];
              gh += lw * v; gw += lh * v; val += lh * lw * v;
            }
            g_a += top * val;
            g_w += (T)W * gw * tgv;
            g_h += (T)H * gh * tgv;
          }
        }
        if (lane < 4) {
          const int64_t pi = wptr * 4 + lane;
          keys[pi] = key;
          vals[pi] = (uint32_t)pi;
          wt[pi] = pw;
        }
#pragma unroll
        for (int off = kGroup / 2; off > 0; off >>= 1) {
          g_w += __shfl_down(g_w, off, kGroup);
          g_h += __shfl_down(g_h, off, kGroup);
          g_a += __shfl_down(g_a, off, kGroup);
        }
        if (lane == 0) {
          grad_loc[2 * wptr] = g_w;
          grad_loc[2 * wptr + 1] = g_h;
          grad_attn[wptr] = g_a;
        }
      }
    }
  }
}

// ---- a dense [B * N, C] copy of a source whose channel stride is not 1 (the module graph's channel-major grad_out) ----
constexpr int kTrT = 64, kTrPitch = 65;
__global__ __launch_bounds__(kBlock) void segsum_rows_copy(const float* __restrict__ src, int64_t ss_b, int64_t ss_c, int64_t ss_n,
                                                           float* __restrict__ rows, int64_t B, int64_t C, int64_t N) {
  __shared__ float tile[kTrT * kTrPitch];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t tn = (N + kTrT - 1) / kTrT, tc = (C + kTrT - 1) / kTrT, tiles = B * tn * tc;
  for (int64_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
    const int64_t b = tl / (tn * tc), rem = tl - b * tn * tc;
    const int64_t n0 = (rem / tc) * kTrT, c0 = (rem % tc) * kTrT;
    const int64_t nr = min(n0 + lane, N - 1);                       // along n
    for (int i = wave; i < kTrT; i += kBlock / kWave) {
      const int64_t c = min(c0 + i, C - 1);
      tile[lane * kTrPitch + i] = src[b * ss_b + c * ss_c + nr * ss_n];
    }
    __syncthreads();
    const int64_t cw = c0 + lane;                                   // along c
    for (int i = wave; i < kTrT; i += kBlock / kWave) {
      const int64_t n = n0 + i;
      if (n < N && cw < C) rows[(b * N + n) * C + cw] = tile[i * kTrPitch + lane];
    }
    __syncthreads();
  }
}

// ---- sum ----
// start[r] = number of sorted keys below r, r = 0 .. R: the pairs of destination r are start[r] .. start[r + 1] - 1.
// A fixed number of halving steps per row, every load at a clamped index.
__global__ __launch_bounds__(kBlock) void segsum_starts(const uint32_t* __restrict__ keys, uint32_t P, uint32_t top, uint32_t R,
                                                        uint32_t* __restrict__ start) {
  const int64_t total = (int64_t)R + 1;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < total; base += (int64_t)gridDim.x * blockDim.x) {
    const bool has = base + threadIdx.x < total;
    const uint32_t r = has ? (uint32_t)(base + threadIdx.x) : R;
    uint32_t pos = 0;
    for (uint32_t s = top; s > 0; s >>= 1) {
      const uint32_t t = pos + s;                                   // pos < top, so no overflow: t < 2 * top <= 2^32 needs top <= 2^30
      const uint32_t k = keys[(t <= P ? t : P) - 1];
      if (t <= P && k < r) pos = t;
    }
    if (has) start[r] = pos;
  }
}

template <int kG>
__global__ __launch_bounds__(kBlock) void segsum_rows(const uint32_t* __restrict__ pairs, const uint32_t* __restrict__ start,
                                                      const float* __restrict__ wt, const float* __restrict__ src,
                                                      float* __restrict__ dst, SumGeom g, uint32_t R) {
  constexpr int kGroups = kBlock / kG;
  constexpr int kU = 8;   // loads issued ahead of their additions.  32 was measured slower (five sites 2.89 against 2.17 ms):
                          // most rows have fewer than ten terms, and a sub-batch issues all its loads, clamped or not
  const int lane = threadIdx.x % kG, grp = threadIdx.x / kG;
  for (int64_t base = (int64_t)blockIdx.x * kGroups; base < (int64_t)R; base += (int64_t)gridDim.x * kGroups) {
    const bool has = base + grp < (int64_t)R;
    const uint32_t r = has ? (uint32_t)(base + grp) : R - 1;
    const uint32_t s0 = start[r], s1 = start[r + 1];
    const uint32_t m = has ? s1 - s0 : 0u;
    uint32_t mmax = m;
#pragma unroll
    for (int o = 32; o >= kG; o >>= 1) mmax = max(mmax, (uint32_t)__shfl_xor((int)mmax, o));
    const uint32_t db = r / g.HW, drem = r - db * g.HW, dy = drem / g.W, dx = drem - dy * g.W;
    float* __restrict__ drow = dst + (int64_t)db * g.ds_b + (int64_t)dy * g.ds_h + (int64_t)dx * g.ds_w;
    for (int c0 = 0; c0 < g.C; c0 += kG) {
      const int c = c0 + lane;
      const bool chan = c < g.C;
      const int64_t coff = (int64_t)(chan ? c : 0) * g.ss_c;
      float total = 0.0f, part = 0.0f;
      for (uint32_t j0 = 0; j0 < mmax; j0 += kG) {
        // lane j: the bookkeeping of term j0 + j (the sorted list's first entry where there is no such term)
        const uint32_t jj = j0 + lane;
        const uint32_t pair = pairs[jj < m ? s0 + jj : 0u];
        const float w = wt[pair];
        const uint32_t row = pair / g.div, sb = row / g.Nn;
        const int64_t so = (int64_t)sb * g.ss_b + (int64_t)(row - sb * g.Nn) * g.ss_n;
        const int so_lo = (int)(uint32_t)so, so_hi = (int)(so >> 32);
        const uint32_t nb = min((uint32_t)kG, mmax - j0);
        for (uint32_t t0 = 0; t0 < nb; t0 += kU) {
          float x[kU], wv[kU];
#pragma unroll
          for (int u = 0; u < kU; ++u) {
            const int t = (int)t0 + u;
            wv[u] = __shfl(w, t, kG);
            const uint32_t lo = (uint32_t)__shfl(so_lo, t, kG);
            const int64_t hi = (int64_t)__shfl(so_hi, t, kG);
            x[u] = src[((hi << 32) | (int64_t)lo) + coff];
          }
#pragma unroll
          for (int u = 0; u < kU; ++u) {
            const uint32_t j = j0 + t0 + u;
            const bool live = j < m;
            const float term = __fmul_rn(wv[u], x[u]);
            const float sum = (j & (kSegL - 1)) == 0 ? term : __fadd_rn(part, term);
            part = live ? sum : part;
            const bool ends = live && ((j & (kSegL - 1)) == kSegL - 1 || j == m - 1);
            const float tot = j < kSegL ? part : __fadd_rn(total, part);
            total = ends ? tot : total;
          }
        }
      }
      if (has && chan) drow[(int64_t)c * g.ds_c] = total;
    }
  }
}

// zero fill through the destination's strides (a problem without pairs)
__global__ __launch_bounds__(kBlock) void segsum_zero(float* __restrict__ dst, SumGeom g, uint32_t R) {
  const int64_t total = (int64_t)R * g.C;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t r = (uint32_t)(i / g.C);
    const int c = (int)(i - (int64_t)r * g.C);
    const uint32_t db = r / g.HW, drem = r - db * g.HW, dy = drem / g.W, dx = drem - dy * g.W;
    dst[(int64_t)db * g.ds_b + (int64_t)dy * g.ds_h + (int64_t)dx * g.ds_w + (int64_t)c * g.ds_c] = 0.0f;
  }
}

// sort + starts + sum over what an emit pass left in the workspace
static int segsum_run(const char* what, char* base, const SegWork& w, int64_t pairs, uint32_t R, const float* src, float* dst,
                      const SumGeom& g, hipStream_t s) {
  uint32_t* keys_out = (uint32_t*)(base + w.keys_out);
  uint32_t* vals_out = (uint32_t*)(base + w.vals_out);
  uint32_t* start = (uint32_t*)(base + w.start);
  size_t cub_bytes = 0;
  if (hipcub::DeviceRadixSort::SortPairs(nullptr, cub_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr,
                                         (uint32_t*)nullptr, (int)pairs, 0, w.bits, s) != hipSuccess || cub_bytes > w.cub_bytes) {
    set_error("%s: the radix sort asks for %lld bytes of scratch, the workspace sets %lld aside", what, (long long)cub_bytes,
              (long long)w.cub_bytes);
    return SMOS_ERR_UNSUPPORTED;
  }
  cub_bytes = w.cub_bytes;
  if (hipcub::DeviceRadixSort::SortPairs(base + w.cub, cub_bytes, (const uint32_t*)(base + w.keys_in), keys_out,
                                         (const uint32_t*)(base + w.vals_in), vals_out, (int)pairs, 0, w.bits, s) != hipSuccess) {
    set_error("%s: radix sort failed", what);
    return SMOS_ERR_LAUNCH;
  }
  uint32_t top = 1;
  while ((int64_t)top * 2 <= pairs) top <<= 1;
  hipLaunchKernelGGL(segsum_starts, dim3((unsigned)conv_grid_cap(grid_for((int64_t)R + 1, kBlock, kMaxGrid))), dim3(kBlock), 0, s,
                     keys_out, (uint32_t)pairs, top, R, start);
  int kG = 8;
  while (kG < 64 && kG < g.C) kG <<= 1;
  const dim3 gr((unsigned)conv_grid_cap(grid_for((int64_t)R, kBlock / kG, kMaxGrid)));
  const float* wt = (const float*)(base + w.wt);
  switch (kG) {
    case 8: hipLaunchKernelGGL((segsum_rows<8>), gr, dim3(kBlock), 0, s, vals_out, start, wt, src, dst, g, R); break;
    case 16: hipLaunchKernelGGL((segsum_rows<16>), gr, dim3(kBlock), 0, s, vals_out, start, wt, src, dst, g, R); break;
    case 32: hipLaunchKernelGGL((segsum_rows<32>), gr, dim3(kBlock), 0, s, vals_out, start, wt, src, dst, g, R); break;
    default: hipLaunchKernelGGL((segsum_rows<64>), gr, dim3(kBlock), 0, s, vals_out, start, wt, src, dst, g, R); break;
  }
  return check_launch(what);
}

static bool bil_det_supported(int64_t B, int64_t C, int64_t H, int64_t W, int64_t N) {
  return B >= 0 && C >= 0 && N >= 0 && H > 0 && W > 0 && H < (1 << 24) && W < (1 << 24) && B * N < (1LL << 29) &&
         B * H * W < (1LL << 31) - 1 && C < (1LL << 31);
}

static bool msda_det_supported(int64_t N, int64_t S, int64_t M, int64_t D, int64_t L, int64_t Lq, int64_t P) {
  if (!(N >= 0 && S >= 0 && M > 0 && D > 0 && L > 0 && Lq >= 0 && P > 0)) return false;
  if (D >= (1LL << 31) || L * P >= (1LL << 29) || N * Lq * M >= (1LL << 29)) return false;
  return N * Lq * M * L * P < (1LL << 29) && N * S * M < (1LL << 31) - 1;
}

}  // namespace smos

using namespace smos;

extern "C" int32_t smos_segsum_chunk(void) { return kSegL; }

extern "C" int64_t smos_bilinear_gather_bwd_det_work_bytes(int64_t B, int64_t C, int64_t H, int64_t W, int64_t N) {
  if (!bil_det_supported(B, C, H, W, N)) return -1;
  if (B == 0 || C == 0 || N == 0) return 0;
  SegWork w;
  segsum_layout(B * N * 4, B * H * W, B * N * C, w);
  return (int64_t)w.total;
}

extern "C" int smos_bilinear_gather_bwd_det(const float* grad_out, const int64_t* grad_out_stride, const float* coord, int32_t K,
                                            float* grad_grid, const int64_t* grad_grid_stride, int64_t B, int64_t C, int64_t H,
                                            int64_t W, int64_t N, const float* scale, void* work, int64_t work_bytes,
                                            smos_stream_t stream) {
  SMOS_REQUIRE(B >= 0 && C >= 0 && N >= 0 && H > 0 && W > 0, "bilinear_gather_bwd_det: bad sizes");
  SMOS_REQUIRE(K >= 2, "bilinear_gather_bwd_det: coord needs >= 2 columns, got %d", (int)K);
  if (!bil_det_supported(B, C, H, W, N)) {
    set_error("bilinear_gather_bwd_det: B * N = %lld points (< 2^29) or B * H * W = %lld rows (< 2^31 - 1) outside the 32-bit keys",
              (long long)(B * N), (long long)(B * H * W));
    return SMOS_ERR_UNSUPPORTED;
  }
  if (B == 0 || C == 0) return SMOS_OK;
  SMOS_REQUIRE(grad_grid && grad_grid_stride, "bilinear_gather_bwd_det: null pointer");
  for (int d = 0; d < 4; ++d) SMOS_REQUIRE(grad_grid_stride[d] >= 0, "bilinear_gather_bwd_det: negative destination stride");
  hipStream_t s = (hipStream_t)stream;
  const uint32_t R = (uint32_t)(B * H * W);
  SumGeom sg;
  sg.ds_b = grad_grid_stride[0]; sg.ds_c = grad_grid_stride[1]; sg.ds_h = grad_grid_stride[2]; sg.ds_w = grad_grid_stride[3];
  sg.HW = (uint32_t)(H * W); sg.W = (uint32_t)W; sg.C = (int)C; sg.div = 4;
  sg.Nn = (uint32_t)(N > 0 ? N : 1); sg.ss_b = 0; sg.ss_n = 0; sg.ss_c = 0;
  if (N == 0) {
    hipLaunchKernelGGL(segsum_zero, dim3(grid_for((int64_t)R * C, kBlock, kMaxGrid)), dim3(kBlock), 0, s, grad_grid, sg, R);
    return check_launch("bilinear_gather_bwd_det zero");
  }
  SMOS_REQUIRE(grad_out && coord && grad_out_stride && scale && work, "bilinear_gather_bwd_det: null pointer");
  SegWork w;
  const int64_t pairs = B * N * 4;
  segsum_layout(pairs, R, B * N * C, w);
  SMOS_REQUIRE((int64_t)w.total <= work_bytes,
               "bilinear_gather_bwd_det: the workspace holds %lld bytes, %lld are needed", (long long)work_bytes, (long long)w.total);
  char* base = (char*)work;
  BilGeom g;
  g.gs_b = H * W; g.gs_c = 0; g.gs_h = W; g.gs_w = 1;       // a tap's offset is its pixel y * W + x
  g.os_b = g.os_c = g.os_n = 0;
  g.H = (int)H; g.W = (int)W; g.K = K; g.sy = scale[0]; g.sx = scale[1];
  hipLaunchKernelGGL(bil_emit, dim3((unsigned)conv_grid_cap(grid_for(B * N, kBlock, kMaxGrid))), dim3(kBlock), 0, s, coord, g, B * N, N, R,
                     (uint32_t*)(base + w.keys_in), (uint32_t*)(base + w.vals_in), (float*)(base + w.wt));
  int rc = check_launch("bilinear_gather_bwd_det emit");
  if (rc != SMOS_OK) return rc;
  const float* src = grad_out;
  sg.ss_b = grad_out_stride[0]; sg.ss_c = grad_out_stride[1]; sg.ss_n = grad_out_stride[2];
  if (sg.ss_c != 1 && C > 1) {
    float* rows = (float*)(base + w.rows);
    const int64_t tiles = B * ((N + kTrT - 1) / kTrT) * ((C + kTrT - 1) / kTrT);
    hipLaunchKernelGGL(segsum_rows_copy, dim3((unsigned)conv_grid_cap(grid_for(tiles, 1, kMaxGrid))), dim3(kBlock), 0, s, grad_out,
                       sg.ss_b, sg.ss_c, sg.ss_n, rows, B, C, N);
    rc = check_launch("bilinear_gather_bwd_det copy");
    if (rc != SMOS_OK) return rc;
    src = rows;
    sg.ss_b = N * C; sg.ss_n = C; sg.ss_c = 1;
  }
  return segsum_run("bilinear_gather_bwd_det", base, w, pairs, R, src, grad_grid, sg, s);
}

extern "C" int64_t smos_msda_bwd_det_work_bytes(int64_t N, int64_t S, int64_t M, int64_t D, int64_t L, int64_t Lq, int64_t P) {
  if (!msda_det_supported(N, S, M, D, L, Lq, P)) return -1;
  if (N * Lq == 0 || N * S == 0) return 0;
  SegWork w;
  segsum_layout(N * Lq * M * L * P * 4, N * S * M, 0, w);
  return (int64_t)w.total;
}

extern "C" int smos_msda_bwd_det(const float* grad_out, const float* value, const int64_t* spatial_shapes,
                                 const int64_t* level_start_index, const float* sampling_loc, const float* attn_weight,
                                 float* grad_value, float* grad_sampling_loc, float* grad_attn_weight, int64_t N, int64_t S,
                                 int64_t M, int64_t D, int64_t L, int64_t Lq, int64_t P, void* work, int64_t work_bytes,
                                 smos_stream_t stream) {
  SMOS_REQUIRE(N >= 0 && S >= 0 && M > 0 && D > 0 && L > 0 && Lq >= 0 && P > 0, "msda_bwd_det: bad sizes");
  if (!msda_det_supported(N, S, M, D, L, Lq, P)) {
    set_error("msda_bwd_det: %lld samples (< 2^29) or %lld value rows (< 2^31 - 1) outside the 32-bit keys",
              (long long)(N * Lq * M * L * P), (long long)(N * S * M));
    return SMOS_ERR_UNSUPPORTED;
  }
  hipStream_t s = (hipStream_t)stream;
  const int64_t heads = N * Lq * M, rows = N * S * M;
  if (rows == 0 && heads == 0) return SMOS_OK;
  SumGeom sg;
  sg.ds_b = 0; sg.ds_h = 0; sg.ds_w = D; sg.ds_c = 1;
  sg.HW = (uint32_t)(rows > 0 ? rows : 1); sg.W = sg.HW; sg.C = (int)D; sg.div = (uint32_t)(L * P * 4);
  sg.Nn = (uint32_t)(heads > 0 ? heads : 1); sg.ss_b = 0; sg.ss_n = D; sg.ss_c = 1;
  const uint32_t R = (uint32_t)rows;
  if (heads == 0) {
    SMOS_REQUIRE(grad_value, "msda_bwd_det: null device pointer");
    hipLaunchKernelGGL(segsum_zero, dim3(grid_for(rows * D, kBlock, kMaxGrid)), dim3(kBlock), 0, s, grad_value, sg, R);
    return check_launch("msda_bwd_det zero");
  }
  SMOS_REQUIRE(grad_out && value && spatial_shapes && level_start_index && sampling_loc && attn_weight && grad_sampling_loc &&
                   grad_attn_weight && (grad_value || rows == 0) && work, "msda_bwd_det: null device pointer");
  SegWork w;
  const int64_t pairs = heads * L * P * 4;
  segsum_layout(pairs, rows, 0, w);
  SMOS_REQUIRE((int64_t)w.total <= work_bytes,
               "msda_bwd_det: the workspace holds %lld bytes, %lld are needed", (long long)work_bytes, (long long)w.total);
  char* base = (char*)work;
  uint32_t* keys = (uint32_t*)(base + w.keys_in);
  uint32_t* vals = (uint32_t*)(base + w.vals_in);
  float* wt = (float*)(base + w.wt);
#define SMOS_EMIT(G)                                                                                                       \
  hipLaunchKernelGGL((msda_bwd_emit<G>), dim3((unsigned)conv_grid_cap(grid_for(heads * G, kBlock, 256 * 16))), dim3(kBlock), 0, s,   \
                     grad_out, value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_sampling_loc,     \
                     grad_attn_weight, keys, vals, wt, R, heads, (int)S, (int)M, (int)D, (int)L, (int)Lq, (int)P)
  if (D <= 32) SMOS_EMIT(32); else SMOS_EMIT(64);
#undef SMOS_EMIT
  int rc = check_launch("msda_bwd_det emit");
  if (rc != SMOS_OK || rows == 0) return rc;
  return segsum_run("msda_bwd_det", base, w, pairs, R, grad_out, grad_value, sg, s);
}
