// 3x3 convolution of a bilinearly upsampled map without upsampling it first (gfx950).
//
// The decoder (multi_view_encoder.py:441-453) resizes the 128-channel maps of the two coarser stages to 256 x 256
// (F.interpolate, bilinear, align_corners=True), concatenates them with the 64-channel fine map and runs conv_1
// (3x3, 320 -> 128): 48.3 GFLOP per sample, 37 % of all FLOPs of the network -- 80 % of them spent on
// inputs that are interpolations of 16x / 4x smaller maps.  Channel mixing and spatial operators commute:
//     conv3x3(up(x)) = sum_{ky,kx} shift_{ky,kx}( up( W_{ky,kx} x ) ),        W_{ky,kx}: the [Cout, Cin] matrix of one tap,
// so the nine tap products are taken at the SOURCE resolution (one GEMM [pixels, Cin] x [Cin, 9 Cout], 16x / 4x fewer
// pixels) and only the cheap spatial part runs at 256 x 256, separably:
//   x pass (upconv_xpass): T[b, ky, ys, X, c]  = sum_kx  up_x( Z[b, ys, :, (3 ky + kx) C + c] )[X + kx - 1]
//   y pass (upconv_ypass): out[b, Y, X, c]     = act( conv_a + bias + sum_src sum_ky  up_y( T_src[b, ky, :, X, c] )[Y + ky - 1] )
// with the zero padding of the convolution applied at the upsampled resolution (taps that leave the 256 x 256 image are
// dropped) and conv_a the ordinary convolution of the channels that are NOT upsampled.  Exact in real arithmetic;
// in float32 it differs from the direct form by summation order only.  conv_1 falls from 48.3 to 15.7 GFLOP per sample
// and the 320-channel concatenated input (336 MB) is never built.
// Interpolation weights: ATen's align_corners=True formula, as in upsample_concat_cl (cl_kernels.hip).
// The adjoint of the two passes, for the training backward (ops.upconv3x3_train), is csrc/upconv_bwd.hip.
#include "smos_common.h"
#include "upconv_lerp.h"      // Lerp, lerp_of, lerp_add: shared with the adjoint (csrc/upconv_bwd.hip)

namespace smos {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// The statements both forms share, so that -ffp-contract=on forms the same FMAs in the pair and in the one launch:
// one bilinear tap pair added to four channels (lerp_add, upconv_lerp.h), and the epilogue.
__device__ __forceinline__ float4 bias_act(const float4& acc, const float4& bv, int act) {   // act: 0 none, 1 ReLU, 2 LeakyReLU(0.01)
  float4 o = make_float4(acc.x + bv.x, acc.y + bv.y, acc.z + bv.z, acc.w + bv.w);
  if (act == 1) {
    o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f);
  } else if (act == 2) {
    o.x = o.x > 0.f ? o.x : 0.01f * o.x; o.y = o.y > 0.f ? o.y : 0.01f * o.y;
    o.z = o.z > 0.f ? o.z : 0.01f * o.z; o.w = o.w > 0.f ? o.w : 0.01f * o.w;
  }
  return o;
}

// Both passes issue ALL their loads unconditionally and up front: a tap that leaves the image reads a clamped (valid)
// address and enters with weight 0.  Written with "if (outside) continue" every tap's pair of loads sat under its own
// lane-dependent branch, and hipcc's wait-count pass answered each with s_waitcnt vmcnt(0): six to seven serialised memory
// round trips per output.  Index arithmetic is 32-bit (the host checks the element counts), addresses 64-bit.

// z [B, Hs, Ws, 9*C] (tap-major blocks of C channels), t [B, 3, Hs, Wo, C]; one thread = 4 channels of one (b, ky, ys, X)
__global__ __launch_bounds__(kBlock) void upconv_xpass(const float* __restrict__ z, float* __restrict__ t, int B, int Hs, int Ws,
                                                       int C4, int Wo) {
  const int total = B * 3 * Hs * Wo * C4;
  const int C = C4 * 4;
  for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < total; i += (int)(gridDim.x * blockDim.x)) {
    const int q = (i % C4) * 4;
    int r = i / C4;
    const int X = r % Wo;
    r /= Wo;
    const int ys = r % Hs;
    r /= Hs;
    const int ky = r % 3, b = r / 3;
    const float* zrow = z + ((int64_t)(b * Hs + ys) * Ws) * (9 * C) + (3 * ky) * C + q;
    float4 v0[3], v1[3];
    float w0[3], w1[3];
    bool inb[3];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int xs = X + kx - 1;
      const bool in = (xs >= 0) & (xs < Wo);          // zero padding of the convolution, at the upsampled resolution
      const Lerp l = lerp_of(min(max(xs, 0), Wo - 1), Ws, Wo);
      const float* p = zrow + (int64_t)l.i0 * (9 * C) + kx * C;
      v0[kx] = *reinterpret_cast<const float4*>(p);
      v1[kx] = *reinterpret_cast<const float4*>(p + (int64_t)l.step * (9 * C));
      w0[kx] = l.w0;
      w1[kx] = l.w1;
      inb[kx] = in;
    }
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      // the loads are unconditional (clamped address); a padded tap is dropped by a select on the VALUE at its consumer,
      // not by a zero weight: 0 * Inf / NaN of a border element must not leak into the output
      const float4 a0 = inb[kx] ? v0[kx] : zero4, a1 = inb[kx] ? v1[kx] : zero4;
      lerp_add(acc, w0[kx], w1[kx], a0, a1);
    }
    *reinterpret_cast<float4*>(t + (int64_t)i * 4) = acc;
  }
}

struct YSrc {
  const float* t;   // [B, 3, Hs, Wo, C]; an absent source is passed as a copy of the other one with on = 0
  int Hs;
  float on;         // 1 / 0
};

// out = act(conv_a + bias + sum over the sources and ky of the y-interpolated x-pass rows); act: 0 none, 1 ReLU, 2 LeakyReLU(0.01)
__global__ __launch_bounds__(kBlock) void upconv_ypass(const float* __restrict__ conv_a, int64_t ap, const float* __restrict__ bias,
                                                       YSrc s1, YSrc s2, float* __restrict__ out, int64_t op, int B, int Ho, int Wo,
                                                       int C4, int act) {
  const int total = B * Ho * Wo * C4;
  const int C = C4 * 4;
  for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < total; i += (int)(gridDim.x * blockDim.x)) {
    const int q = (i % C4) * 4;
    int r = i / C4;
    const int X = r % Wo;
    r /= Wo;
    const int Y = r % Ho, b = r / Ho;
    const int64_t pix = (int64_t)(b * Ho + Y) * Wo + X;
    float4 acc = *reinterpret_cast<const float4*>(conv_a + pix * ap + q);
    const float4 bv = *reinterpret_cast<const float4*>(bias + q);
    float4 v0[2][3], v1[2][3];
    float w0[2][3], w1[2][3];
    bool inb[2][3];
#pragma unroll
    for (int si = 0; si < 2; ++si) {
      const YSrc s = si == 0 ? s1 : s2;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int ysrc = Y + ky - 1;
        const bool in = (ysrc >= 0) & (ysrc < Ho);
        const Lerp l = lerp_of(min(max(ysrc, 0), Ho - 1), s.Hs, Ho);
        const float* p = s.t + ((int64_t)((b * 3 + ky) * s.Hs + l.i0) * Wo + X) * C + q;
        v0[si][ky] = *reinterpret_cast<const float4*>(p);
        v1[si][ky] = *reinterpret_cast<const float4*>(p + (int64_t)l.step * Wo * C);
        w0[si][ky] = l.w0;
        w1[si][ky] = l.w1;
        inb[si][ky] = in & (s.on != 0.0f);
      }
    }
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int si = 0; si < 2; ++si)
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const float4 a0 = inb[si][ky] ? v0[si][ky] : zero4, a1 = inb[si][ky] ? v1[si][ky] : zero4;   // select on the value (NaN-safe)
        lerp_add(acc, w0[si][ky], w1[si][ky], a0, a1);
      }
    *reinterpret_cast<float4*>(out + pix * op + q) = bias_act(acc, bv, act);
  }
}

// ---- both passes in one kernel: the x-pass rows never leave the CU ----
// One thread = 4 channels of one output COLUMN segment (b, X, rows [Y0, Y0 + strip)): it walks down the strip and keeps,
// per source, a window of three x-pass rows T[ky][i][X] (3 rows x 3 ky x float4).  Output row Y reads the source rows
// i0(Y + ky - 1) and i0 + step for ky = 0..2, all inside [i0(Y - 1), i0(Y - 1) + 2] when the y ratio is below 1/2 (the
// host checks it), so the window only slides down, by one row at a time, and each x-pass row is computed once per strip.
// Same operations in the same order as upconv_xpass followed by upconv_ypass: z is read once (plus 2 rows per strip), t
// (0.3 GB written and read back at the network's sizes) does not exist.
//
// The window lives in LDS, private to its thread ([source][slot][ky][thread] float4: consecutive lanes, consecutive 16
// bytes), and source row i sits in slot i % 3: a slide overwrites the slot of the row that left and moves nothing.
// What depends on the output row alone is worked out once per unit by the first strip + 2 lanes and kept in LDS too:
//   RowTap[fine row][source]  the y taps of fine row Y0 - 1 + e: the slot offsets of rows i0 and i0 + step and the two
//                             weights, from lerp_of itself.  A fine row outside the image gets the offset of a block of
//                             zeros instead, so the tap it drops reads +0 where the select used to put +0;
//   slide[row][source]        the source row whose x pass output row Y0 + r needs first, or -1.
// The row loop holds no select and no index arithmetic.  The x taps that leave the image are dropped by address: z is read
// through a buffer descriptor of one source row, and a dropped tap uses an offset past its end (reads 0, touches nothing).
// The x-pass row of the NEXT output row and its conv_a value are requested before the y pass of the current one.
struct XYSrc {
  const float* z;   // [B, Hs, Ws, 9 * C]; an absent second source is never read
  int Hs, Ws;
};

constexpr int kXyMaxStrip = 32;
constexpr unsigned kXyKy = kBlock * 16;                                 // bytes of one [thread] float4 plane
constexpr unsigned kXySlot = 3 * kXyKy;                                 // one window slot: [ky][thread]
constexpr unsigned kXySrc = 3 * kXySlot;                                // one source's window
constexpr unsigned kXyZero = 2 * kXySrc;                                // [thread] float4 of zeros
constexpr unsigned kXyTab = kXyZero + kXyKy;                            // RowTap [strip + 2][2]
constexpr unsigned kXySlide = kXyTab + (kXyMaxStrip + 2) * 2 * 16;      // int [strip + 1][2]
constexpr unsigned kXyLds = kXySlide + (kXyMaxStrip + 1) * 2 * 4;       // 79 176 bytes: two blocks per CU
constexpr unsigned kXyOob = 0x80000000u;                                // a buffer offset past the end of any row

struct XTaps {      // the three kx taps of one thread's column X in one source: byte offsets into a z row and weights
  unsigned o0[3], o1[3];
  float w0[3], w1[3];
};

__device__ __forceinline__ XTaps x_taps(int X, int Ws, int Wo, int C, int q) {
  XTaps t;
#pragma unroll
  for (int kx = 0; kx < 3; ++kx) {
    const int xs = X + kx - 1;
    const bool in = (xs >= 0) & (xs < Wo);             // zero padding of the convolution, at the upsampled resolution
    const Lerp l = lerp_of(min(max(xs, 0), Wo - 1), Ws, Wo);
    t.o0[kx] = in ? (unsigned)(l.i0 * (9 * C) + kx * C + q) * 4u : kXyOob;
    t.o1[kx] = in ? (unsigned)((l.i0 + l.step) * (9 * C) + kx * C + q) * 4u : kXyOob;
    t.w0[kx] = l.w0;
    t.w1[kx] = l.w1;
  }
  return t;
}

struct XRow {       // the 18 float4 of z one x-pass row reads
  float4 v0[3][3], v1[3][3];
};

__device__ __forceinline__ float4 xy_as_float4(u32x4 v) {
  return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}

// requests row ys of one sample's z [Hs, Ws, 9 C]: a descriptor of that row alone, every load unconditional
__device__ __forceinline__ void x_load(const float* zb, int ys, int Ws, int C, const XTaps& xt, XRow& r) {
  const unsigned row_bytes = (unsigned)(Ws * 9 * C) * 4u;
  // the row's address is the same for every lane; said explicitly, or hipcc may work it out in vector registers and then
  // wraps each of the 18 loads into a loop over the descriptor's distinct values
  const uint64_t row = reinterpret_cast<uint64_t>(zb + (int64_t)ys * (Ws * 9 * C));
  const uint64_t urow = ((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(row >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)row);
  const __amdgpu_buffer_rsrc_t srd = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<float*>(urow), 0, (int)row_bytes, 0x00020000);
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      r.v0[ky][kx] = xy_as_float4(__builtin_amdgcn_raw_buffer_load_b128(srd, xt.o0[kx], 3 * ky * C * 4, 0));
      r.v1[ky][kx] = xy_as_float4(__builtin_amdgcn_raw_buffer_load_b128(srd, xt.o1[kx], 3 * ky * C * 4, 0));
    }
}

// T[ky][ys][X] for ky = 0..2 (upconv_xpass's sum, same order) into the thread's window slot at LDS byte address `at`
__device__ __forceinline__ void x_sum(const XRow& r, const XTaps& xt, unsigned char* at) {
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) lerp_add(acc, xt.w0[kx], xt.w1[kx], r.v0[ky][kx], r.v1[ky][kx]);
    *reinterpret_cast<float4*>(at + ky * kXyKy) = acc;
  }
}

// TWO: both sources; else s1 alone (the host passes a lone source as s1)
template <bool TWO>
__global__ __launch_bounds__(kBlock, 2) void upconv_xy(const float* __restrict__ conv_a, int64_t ap, const float* __restrict__ bias, XYSrc s1,
                                                    XYSrc s2, float* __restrict__ out, int64_t op, int B, int Ho, int Wo, int C4,
                                                    int strip, int act) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = (int)threadIdx.x;
  unsigned char* const mine = smem + (unsigned)tid * 16u;       // this thread's float4 of every [thread] plane
  *reinterpret_cast<float4*>(mine + kXyZero) = make_float4(0.f, 0.f, 0.f, 0.f);
  const int C = C4 * 4;
  const int per_row = Wo * C4;                       // threads of one (b, strip): a block never straddles two of them
  const int blocks_per_row = (per_row + kBlock - 1) / kBlock;
  const int n_strips = (Ho + strip - 1) / strip;
  const int n_units = B * n_strips * blocks_per_row;
  // units are numbered column block fastest.  Blocks b, b + 8, b + 16 .. share an XCD and its L2 (dispatch is round-robin
  // over the 8 XCDs): they take consecutive units, so the column blocks of one (sample, strip), which read the same z
  // columns at their seams, meet in one L2 (speed only)
  const int nb = (int)gridDim.x, xq = nb >> 3, xr = nb & 7, xcd = (int)blockIdx.x & 7;       // 8 XCDs, as conv_igemm numbers its blocks
  const int lblock = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + ((int)blockIdx.x >> 3);
  for (int unit = lblock; unit < n_units; unit += nb) {
    const int i = (unit % blocks_per_row) * kBlock + tid;
    const int bs = unit / blocks_per_row;
    const int Y0 = (bs % n_strips) * strip, b = bs / n_strips;
    const int Y1 = min(Y0 + strip, Ho), rows = Y1 - Y0;
    __syncthreads();                                 // the previous unit's rows have been read by every wave
    if (tid < strip + 2) {
#pragma unroll
      for (int si = 0; si < (TWO ? 2 : 1); ++si) {
        const XYSrc s = si == 0 ? s1 : s2;
        const int f = Y0 - 1 + tid;                  // the fine row of RowTap[tid]
        const bool in = (f >= 0) & (f < Ho);
        const Lerp l = lerp_of(min(max(f, 0), Ho - 1), s.Hs, Ho);
        // a row above the image is only ever the ky = 0 tap (of Y = 0), one below it only the ky = 2 tap (of Y = Ho - 1):
        // the offset that lands on the zeros behind that tap's constant part of the address
        const unsigned zeros = kXyZero - si * kXySrc - (f < 0 ? 0u : 2u) * kXyKy;
        int4 e;
        e.x = (int)(in ? (unsigned)(l.i0 % 3) * kXySlot : zeros);
        e.y = (int)(in ? (unsigned)((l.i0 + l.step) % 3) * kXySlot : zeros);
        e.z = __float_as_int(l.w0);
        e.w = __float_as_int(l.w1);
        *reinterpret_cast<int4*>(smem + kXyTab + (unsigned)(tid * 2 + si) * 16u) = e;
        if (tid <= strip) {                          // output row Y0 + tid: the window slides when i0(Y - 1) moves
          const int Y = Y0 + tid;
          int ys = -1;
          if (tid >= 1 && Y < Y1) {
            const int lo = lerp_of(max(Y - 1, 0), s.Hs, Ho).i0, before = lerp_of(max(Y - 2, 0), s.Hs, Ho).i0;
            if (lo > before && lo + 2 <= s.Hs - 1) ys = lo + 2;      // (a row past the last one is never a tap)
          }
          *reinterpret_cast<int*>(smem + kXySlide + (unsigned)(tid * 2 + si) * 4u) = ys;
        }
      }
    }
    __syncthreads();
    if (i >= per_row) continue;
    const int q = (i % C4) * 4, X = i / C4;
    const float4 bv = *reinterpret_cast<const float4*>(bias + q);
    // conv_a and out: a uniform row pointer plus this thread's 32-bit byte offset inside the row (the host checks the row)
    const unsigned aoff = (unsigned)(X * (int)ap + q) * 4u, ooff = (unsigned)(X * (int)op + q) * 4u;
    const char* arow = reinterpret_cast<const char*>(conv_a + (int64_t)(b * Ho + Y0) * Wo * ap);
    char* orow = reinterpret_cast<char*>(out + (int64_t)(b * Ho + Y0) * Wo * op);
    const int64_t astep = (int64_t)Wo * ap * 4, ostep = (int64_t)Wo * op * 4;
    float4 a_next = *reinterpret_cast<const float4*>(arow + aoff);
    XTaps xt[2];
    const float* zb[2];
    // the window of the strip's first row: source rows base .. base + 2
    int base[2] = {0, 0};
#pragma unroll
    for (int si = 0; si < (TWO ? 2 : 1); ++si) {
      const XYSrc s = si == 0 ? s1 : s2;
      xt[si] = x_taps(X, s.Ws, Wo, C, q);
      zb[si] = s.z + (int64_t)b * s.Hs * s.Ws * (9 * C);
      base[si] = __builtin_amdgcn_readfirstlane(lerp_of(max(Y0 - 1, 0), s.Hs, Ho).i0);
    }
#pragma unroll 1
    for (int k = 0; k < 3; ++k) {                    // rolled: one row's 18 loads in flight at a time
#pragma unroll
      for (int si = 0; si < (TWO ? 2 : 1); ++si) {
        const XYSrc s = si == 0 ? s1 : s2;
        if (base[si] + k > s.Hs - 1) continue;       // (a row past the last one is never a tap)
        XRow zr;
        x_load(zb[si], base[si] + k, s.Ws, C, xt[si], zr);
        x_sum(zr, xt[si], mine + si * kXySrc + (unsigned)((base[si] + k) % 3) * kXySlot);
      }
    }
    for (int r = 0; r < rows; ++r) {
      float4 acc = a_next;
      // what the next output row needs from memory travels during this row's y pass: its conv_a value and, if source 1's
      // window slides there, that x-pass row (both sources' rows at once do not fit the registers of two waves per SIMD;
      // source 2, a quarter of the slides at the network's sizes, is fetched behind the store)
      XRow zr;
      int ys[2] = {-1, -1};
#pragma unroll
      for (int si = 0; si < (TWO ? 2 : 1); ++si)
        ys[si] = __builtin_amdgcn_readfirstlane(*reinterpret_cast<const int*>(smem + kXySlide + (unsigned)((r + 1) * 2 + si) * 4u));
      if (ys[0] >= 0) x_load(zb[0], ys[0], s1.Ws, C, xt[0], zr);
      a_next = *reinterpret_cast<const float4*>(arow + (int64_t)min(r + 1, rows - 1) * astep + aoff);
#pragma unroll
      for (int si = 0; si < (TWO ? 2 : 1); ++si) {
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          const int4 e = *reinterpret_cast<const int4*>(smem + kXyTab + (unsigned)((r + ky) * 2 + si) * 16u);
          const float4 r0 = *reinterpret_cast<const float4*>(mine + (unsigned)e.x + (si * kXySrc + ky * kXyKy));
          const float4 r1 = *reinterpret_cast<const float4*>(mine + (unsigned)e.y + (si * kXySrc + ky * kXyKy));
          lerp_add(acc, __int_as_float(e.z), __int_as_float(e.w), r0, r1);
        }
      }
      *reinterpret_cast<float4*>(orow + (int64_t)r * ostep + ooff) = bias_act(acc, bv, act);
      // the next row's slides, behind this row's reads of the slots they overwrite
      if (ys[0] >= 0) x_sum(zr, xt[0], mine + (unsigned)(ys[0] % 3) * kXySlot);
      if (TWO && ys[1] >= 0) {
        x_load(zb[1], ys[1], s2.Ws, C, xt[1], zr);
        x_sum(zr, xt[1], mine + kXySrc + (unsigned)(ys[1] % 3) * kXySlot);
      }
    }
  }
}

}  // namespace smos

using namespace smos;

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" int smos_upconv_xpass(const float* z, float* t, int64_t B, int64_t Hs, int64_t Ws, int64_t C, int64_t Wo,
                                 smos_stream_t stream) {
  SMOS_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && C > 0 && C % 4 == 0 && Wo > 0, "upconv_xpass: bad sizes (C %% 4 must be 0)");
  SMOS_REQUIRE(z && t && aligned16(z) && aligned16(t), "upconv_xpass: null / unaligned pointer");
  SMOS_REQUIRE(B * 3 * Hs * Wo * (C / 4) < kMaxTotal32 && B * Hs < (1LL << 31), "upconv_xpass: too many elements for 32-bit indices");
  hipLaunchKernelGGL(upconv_xpass, dim3(grid_for(B * 3 * Hs * Wo * (C / 4), kBlock, 256 * 32)), dim3(kBlock), 0, (hipStream_t)stream, z, t,
                     (int)B, (int)Hs, (int)Ws, (int)(C / 4), (int)Wo);
  return check_launch("upconv_xpass");
}

extern "C" int smos_upconv_ypass(const float* conv_a, int64_t a_pitch, const float* bias, const float* t1, int64_t H1, const float* t2,
                                 int64_t H2, float* out, int64_t out_pitch, int64_t B, int64_t Ho, int64_t Wo, int64_t C, int32_t act,
                                 smos_stream_t stream) {
  SMOS_REQUIRE(B > 0 && Ho > 0 && Wo > 0 && C > 0 && C % 4 == 0 && act >= 0 && act <= 2 && a_pitch % 4 == 0 && out_pitch % 4 == 0,
               "upconv_ypass: bad arguments");
  SMOS_REQUIRE(conv_a && bias && out && aligned16(conv_a) && aligned16(out) && aligned16(bias) && (!t1 || (aligned16(t1) && H1 > 0)) &&
                   (!t2 || (aligned16(t2) && H2 > 0)), "upconv_ypass: null / unaligned pointer");
  SMOS_REQUIRE(B * Ho * Wo * (C / 4) < kMaxTotal32 && (t1 || t2) && B * 3 * (H1 > H2 ? H1 : H2) < (1LL << 31),
               "upconv_ypass: too many elements for 32-bit indices / no source");
  // an absent source: the other one again, switched off -- every load of the kernel stays unconditional
  YSrc s1{t1 ? t1 : t2, (int)(t1 ? H1 : H2), t1 ? 1.0f : 0.0f}, s2{t2 ? t2 : t1, (int)(t2 ? H2 : H1), t2 ? 1.0f : 0.0f};
  hipLaunchKernelGGL(upconv_ypass, dim3(grid_for(B * Ho * Wo * (C / 4), kBlock, 256 * 32)), dim3(kBlock), 0, (hipStream_t)stream, conv_a,
                     a_pitch, bias, s1, s2, out, out_pitch, (int)B, (int)Ho, (int)Wo, (int)(C / 4), (int)act);
  return check_launch("upconv_ypass");
}

extern "C" int smos_upconv_xy_ok(int64_t Hs, int64_t Ho) { return Hs > 0 && Ho > 0 && 2 * (Hs - 1) < Ho - 1 + (Ho == 1); }

// the strip height smos_upconv_xy chooses: long strips amortise the two extra x-pass rows a strip computes before its first
// output row; short ones give more blocks.  32 rows where that still leaves >= 8 waves per CU, else 16, else 8.  (Measured at
// the network's geometry, interpolation only, r04: 8 rows 0.218 ms, 16 0.188, 32 0.162, 64 0.166, 128 0.164; the x pass + y pass pair 0.259.)
static int xy_strip(int64_t B, int64_t Ho, int64_t Wo, int64_t C) {
  const int64_t per_row_blocks = (Wo * (C / 4) + kBlock - 1) / kBlock;
  int strip = 32;
  while (strip > 8 && B * ((Ho + strip - 1) / strip) * per_row_blocks < 512) strip >>= 1;
  return strip;
}

extern "C" int smos_upconv_xy(const float* conv_a, int64_t a_pitch, const float* bias, const float* z1, int64_t H1, int64_t W1,
                              const float* z2, int64_t H2, int64_t W2, float* out, int64_t out_pitch, int64_t B, int64_t Ho, int64_t Wo,
                              int64_t C, int32_t act, smos_stream_t stream) {
  return smos_upconv_xy_units(conv_a, a_pitch, bias, z1, H1, W1, z2, H2, W2, out, out_pitch, B, Ho, Wo, C, act, xy_strip(B, Ho, Wo, C), 0,
                              stream);
}

extern "C" int smos_upconv_xy_units(const float* conv_a, int64_t a_pitch, const float* bias, const float* z1, int64_t H1, int64_t W1,
                                    const float* z2, int64_t H2, int64_t W2, float* out, int64_t out_pitch, int64_t B, int64_t Ho,
                                    int64_t Wo, int64_t C, int32_t act, int32_t strip, int64_t max_blocks, smos_stream_t stream) {
  SMOS_REQUIRE(B > 0 && Ho > 0 && Wo > 0 && C > 0 && C % 4 == 0 && act >= 0 && act <= 2 && a_pitch % 4 == 0 && out_pitch % 4 == 0,
               "upconv_xy: bad arguments");
  SMOS_REQUIRE(conv_a && bias && out && aligned16(conv_a) && aligned16(out) && aligned16(bias) && (z1 || z2) &&
                   (!z1 || (aligned16(z1) && H1 > 0 && W1 > 0)) && (!z2 || (aligned16(z2) && H2 > 0 && W2 > 0)),
               "upconv_xy: null / unaligned pointer or no source");
  SMOS_REQUIRE((!z1 || smos_upconv_xy_ok(H1, Ho)) && (!z2 || smos_upconv_xy_ok(H2, Ho)),
               "upconv_xy: a source is taller than half the output (use the x pass + y pass pair)");
  SMOS_REQUIRE(B * Ho * Wo * (C / 4) < kMaxTotal32 && (!z1 || B * H1 * W1 * 9 * C < kMaxTotal32) && (!z2 || B * H2 * W2 * 9 * C < kMaxTotal32),
               "upconv_xy: too many elements for 32-bit indices");
  SMOS_REQUIRE((strip == 8 || strip == 16 || strip == 32) && max_blocks >= 0, "upconv_xy: strip must be 8, 16 or 32, max_blocks >= 0");
  // the kernel addresses a row of conv_a / out and a row of z with 32-bit byte offsets
  SMOS_REQUIRE(a_pitch >= C && out_pitch >= C && Wo * a_pitch < (1LL << 29) && Wo * out_pitch < (1LL << 29) &&
                   (!z1 || W1 * 9 * C < (1LL << 29)) && (!z2 || W2 * 9 * C < (1LL << 29)),
               "upconv_xy: a row of conv_a, out or z is 2 GiB or longer, or a pitch below C");
  const bool two = z1 && z2;
  const XYSrc s1 = z1 ? XYSrc{z1, (int)H1, (int)W1} : XYSrc{z2, (int)H2, (int)W2}, s2 = two ? XYSrc{z2, (int)H2, (int)W2} : s1;
  KernelSetup ks;
  if (int rc = kernel_setup(reinterpret_cast<const void*>(two ? &upconv_xy<true> : &upconv_xy<false>), kXyLds, 0, &ks, "upconv_xy")) return rc;
  const int64_t per_row_blocks = (Wo * (C / 4) + kBlock - 1) / kBlock;
  int64_t grid = B * ((Ho + strip - 1) / strip) * per_row_blocks;      // units of work; a block walks several beyond the cap
  if (grid > 256 * 32) grid = 256 * 32;
  if (max_blocks > 0 && grid > max_blocks) grid = max_blocks;
  hipLaunchKernelGGL(two ? upconv_xy<true> : upconv_xy<false>, dim3((unsigned)grid), dim3(kBlock), kXyLds, (hipStream_t)stream, conv_a, a_pitch,
                     bias, s1, s2, out, out_pitch, (int)B, (int)Ho, (int)Wo, (int)(C / 4), (int)strip, (int)act);
  return check_launch("upconv_xy");
}
