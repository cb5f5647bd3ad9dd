// The adjoint of the spatial part of csrc/upconv.hip: what the training backward of the decoder's conv_1 needs between the
// output gradient and the two matrix products at source resolution (ops.upconv3x3_train).
//
// The forward is linear in the tap products z:  out = conv_a + sum_src L_src z_src  with
//     (L z)[b, Y, X, c] = sum_ky sum_kx  up_y( up_x( z[b, :, :, (3 ky + kx) C + c] ) )[Y + ky - 1, X + kx - 1]
// (taps that leave the Ho x Wo image dropped).  The gradient with respect to z is G = L^T g:
//     G[b, ys, xs, (3 ky + kx) C + c] = sum_{Y, X}  wy(Y + ky - 1 -> ys) * wx(X + kx - 1 -> xs) * g[b, Y, X, c],
// w(dst -> src) being the weight with which lerp_of(dst) reads source index src (w0 at i0, w1 at i0 + step, both when step
// is 0).  Separable, mirroring the forward pair in reverse order:
//   y adjoint (upconv_bwd_ypass): S[b, ky, ys, X, c] = sum_D  wy(D -> ys) * g[b, D - ky + 1, X, c]        D = Y + ky - 1 in [0, Ho)
//   x adjoint (upconv_bwd_xpass): G[b, ys, xs, (3 ky + kx) C + c] = sum_D  wx(D -> xs) * S[b, ky, ys, D - kx + 1, c]
// S has the layout of the forward's t [B, 3, Hs, Wo, C], G that of its z [B * Hs * Ws, 9 * C].
//
// Gather form: one thread sums one float4 of S / G over a window of destination indices D in ascending order -- no atomics,
// the same bits on every run and for every grid.  The window: lerp_of(D) reads src when its i0 is src - 1 or src, that is
// when s = r D lies in [src - 1, src + 1), r = (n_src - 1) / (n_dst - 1).  In exact arithmetic these are the D from
// ceil((src - 1) / r) to floor((src + 1) / r); lerp_of's float32 s is off by at most 2 u s, far less than the 1 / (n_dst - 1)
// by which s can miss an integer without hitting it (the host requires n_src * n_dst <= 2^22), so at worst the D whose exact s
// IS src - 1 or src + 1 changes sides -- and both are inside
//     [ floor((src - 1) / r),  floor((src - 1) / r) + ceil(2 / r) + 1 ],
// ceil(2 / r) + 2 indices, the window every thread of a launch scans (n_src = 1: every destination).  Whether a D belongs
// is decided by comparing lerp_of(D)'s own indices with src, and the weight is the one lerp_of returns.
//
// As in the forward, every load of the window is issued unconditionally at a clamped address, and a contribution that does
// not belong is dropped by a select on the VALUE: loads under lane-dependent branches serialise, and
// 0 * Inf of a gradient element outside the stencil must not leak.  Index arithmetic is 32-bit (the host checks the element
// counts), addresses 64-bit.
#include "smos_common.h"
#include "upconv_lerp.h"

namespace smos {

// first destination index of the window of source index src
__device__ __forceinline__ int window_lo(int src, int n_src, int n_dst) {
  return (src > 0 && n_src > 1) ? ((src - 1) * (n_dst - 1)) / (n_src - 1) : 0;
}

// g [B, Ho, Wo, *] (row pitch gp), s [B, 3, Hs, Wo, C]; one thread = 4 channels of one (b, ky, ys, X)
__global__ __launch_bounds__(kBlock) void upconv_bwd_ypass(const float* __restrict__ g, int64_t gp, float* __restrict__ s, int B, int Ho,
                                                           int Wo, int C4, int Hs, int win) {
  const int total = B * 3 * Hs * Wo * C4;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < total; i += (int)(gridDim.x * blockDim.x)) {
    const int q = (i % C4) * 4;
    int r = i / C4;
    const int X = r % Wo;
    r /= Wo;
    const int ys = r % Hs;
    r /= Hs;
    const int ky = r % 3, b = r / 3;
    const int d_lo = window_lo(ys, Hs, Ho);
    const float* gcol = g + ((int64_t)(b * Ho) * Wo + X) * gp + q;
    float4 acc = zero4;
#pragma unroll 4
    for (int j = 0; j < win; ++j) {
      const int D = d_lo + j, Dc = min(D, Ho - 1);
      const int Y = Dc - ky + 1;                       // the output row whose tap ky reads fine row D
      const bool in = (D < Ho) & (Y >= 0) & (Y < Ho);
      const Lerp l = lerp_of(Dc, Hs, Ho);
      const float4 v = *reinterpret_cast<const float4*>(gcol + (int64_t)(min(max(Y, 0), Ho - 1) * Wo) * gp);
      const bool c0 = in & (l.i0 == ys), c1 = in & (l.i0 + l.step == ys);
      const float4 a0 = c0 ? v : zero4, a1 = c1 ? v : zero4;      // select on the value (Inf / NaN outside the stencil stay out)
      lerp_add(acc, l.w0, l.w1, a0, a1);
    }
    *reinterpret_cast<float4*>(s + (int64_t)i * 4) = acc;
  }
}

// s [B, 3, Hs, Wo, C], gz [B * Hs * Ws, *] (row pitch zp, tap-major blocks of C channels); one thread = 4 channels of one
// (b, ys, xs, tap)
__global__ __launch_bounds__(kBlock) void upconv_bwd_xpass(const float* __restrict__ s, float* __restrict__ gz, int64_t zp, int B, int Hs,
                                                           int Ws, int C4, int Wo, int win) {
  const int total = B * Hs * Ws * 9 * C4;
  const int C = C4 * 4;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < total; i += (int)(gridDim.x * blockDim.x)) {
    const int q = (i % C4) * 4;
    int r = i / C4;
    const int t = r % 9;
    r /= 9;
    const int xs = r % Ws;
    r /= Ws;
    const int ys = r % Hs, b = r / Hs;
    const int ky = t / 3, kx = t - 3 * ky;
    const int d_lo = window_lo(xs, Ws, Wo);
    const float* srow = s + ((int64_t)((b * 3 + ky) * Hs + ys) * Wo) * C + q;
    float4 acc = zero4;
#pragma unroll 4
    for (int j = 0; j < win; ++j) {
      const int D = d_lo + j, Dc = min(D, Wo - 1);
      const int X = Dc - kx + 1;                       // the output column whose tap kx reads fine column D
      const bool in = (D < Wo) & (X >= 0) & (X < Wo);
      const Lerp l = lerp_of(Dc, Ws, Wo);
      const float4 v = *reinterpret_cast<const float4*>(srow + (int64_t)(min(max(X, 0), Wo - 1)) * C);
      const bool c0 = in & (l.i0 == xs), c1 = in & (l.i0 + l.step == xs);
      const float4 a0 = c0 ? v : zero4, a1 = c1 ? v : zero4;
      lerp_add(acc, l.w0, l.w1, a0, a1);
    }
    *reinterpret_cast<float4*>(gz + ((int64_t)((b * Hs + ys) * Ws + xs)) * zp + t * C + q) = acc;
  }
}

}  // namespace smos

using namespace smos;

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// destinations every thread scans for an axis n_src -> n_dst: ceil(2 / r) + 2, the whole axis at most (and for n_src = 1)
static int64_t window_len(int64_t n_src, int64_t n_dst) {
  if (n_src == 1) return n_dst;
  const int64_t w = (2 * (n_dst - 1) + n_src - 2) / (n_src - 1) + 2;
  return w < n_dst ? w : n_dst;
}

static unsigned capped_grid(int64_t items, int64_t max_blocks) {
  int64_t grid = grid_for(items, kBlock, 256 * 32);
  if (max_blocks > 0 && grid > max_blocks) grid = max_blocks;
  return (unsigned)grid;
}

extern "C" int smos_upconv_bwd_window(int64_t n_src, int64_t n_dst) {
  return n_src > 0 && n_dst > 0 ? (int)window_len(n_src, n_dst) : 0;
}

extern "C" int smos_upconv_bwd_ypass(const float* g, int64_t g_pitch, float* s, int64_t B, int64_t Ho, int64_t Wo, int64_t C, int64_t Hs,
                                     int64_t max_blocks, smos_stream_t stream) {
  SMOS_REQUIRE(B > 0 && Ho > 0 && Wo > 0 && C > 0 && C % 4 == 0 && Hs > 0 && g_pitch % 4 == 0 && g_pitch >= C && max_blocks >= 0,
               "upconv_bwd_ypass: bad sizes (C %% 4 and g_pitch %% 4 must be 0, g_pitch >= C, max_blocks >= 0)");
  SMOS_REQUIRE(g && s && aligned16(g) && aligned16(s), "upconv_bwd_ypass: null / unaligned pointer");
  SMOS_REQUIRE(B * 3 * Hs * Wo * (C / 4) < kMaxTotal32 && B * Ho * Wo * (C / 4) < kMaxTotal32 && B * 3 * Hs < (1LL << 31) &&
                   Hs * Ho <= (1LL << 22),
               "upconv_bwd_ypass: too many elements for 32-bit indices, or Hs * Ho above 2^22");
  hipLaunchKernelGGL(upconv_bwd_ypass, dim3(capped_grid(B * 3 * Hs * Wo * (C / 4), max_blocks)), dim3(kBlock), 0, (hipStream_t)stream, g,
                     g_pitch, s, (int)B, (int)Ho, (int)Wo, (int)(C / 4), (int)Hs, (int)window_len(Hs, Ho));
  return check_launch("upconv_bwd_ypass");
}

extern "C" int smos_upconv_bwd_xpass(const float* s, float* gz, int64_t gz_pitch, int64_t B, int64_t Hs, int64_t Ws, int64_t C, int64_t Wo,
                                     int64_t max_blocks, smos_stream_t stream) {
  SMOS_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && C > 0 && C % 4 == 0 && Wo > 0 && gz_pitch % 4 == 0 && gz_pitch >= 9 * C && max_blocks >= 0,
               "upconv_bwd_xpass: bad sizes (C %% 4 and gz_pitch %% 4 must be 0, gz_pitch >= 9 C, max_blocks >= 0)");
  SMOS_REQUIRE(s && gz && aligned16(s) && aligned16(gz), "upconv_bwd_xpass: null / unaligned pointer");
  SMOS_REQUIRE(B * 3 * Hs * Wo * (C / 4) < kMaxTotal32 && B * Hs * Ws * 9 * (C / 4) < kMaxTotal32 && B * 3 * Hs < (1LL << 31) &&
                   Ws * Wo <= (1LL << 22),
               "upconv_bwd_xpass: too many elements for 32-bit indices, or Ws * Wo above 2^22");
  hipLaunchKernelGGL(upconv_bwd_xpass, dim3(capped_grid(B * Hs * Ws * 9 * (C / 4), max_blocks)), dim3(kBlock), 0, (hipStream_t)stream, s, gz,
                     gz_pitch, (int)B, (int)Hs, (int)Ws, (int)(C / 4), (int)Wo, (int)window_len(Ws, Wo));
  return check_launch("upconv_bwd_xpass");
}
