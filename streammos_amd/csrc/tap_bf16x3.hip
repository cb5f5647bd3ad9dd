// The decoder's tap products z = x W^T (csrc/upconv.hip: [B Hs Ws, 128] x [128, 9 * C]) on the bf16 matrix pipe at fp32
// accuracy: every fp32 operand is split EXACTLY into three bf16 limbs and the six leading limb products are summed in fp32.
//
// The split.  hi = bf16(v), mid = bf16(v - hi), lo = bf16(v - hi - mid), round-to-nearest-even (v_cvt_pk_bf16_f32).  Both
// subtractions are exact in fp32 and 3 x 8 significand bits make 24, so hi + mid + lo == v.  A product of two limbs is exact
// in fp32 (8 x 8 bits).  Of the nine limb products of x w the kernel sums six -- hh, hm, mh, hl, lh, mm -- and drops
// |xm wl| + |xl wm| + |xl wl| <= (2^-24 + 2^-24 + 2^-32) |x| |w| per term: about 2 u with u = 2^-24, the size of ONE fp32
// rounding of that product.  The sum runs in fp32 on one accumulator per output (v_mfma_f32_32x32x16_bf16: 16 terms per
// instruction), 8 k steps x 6 products in a fixed order, low-order products first inside a k step:
//     xl wh, xh wl, xm wm, xm wh, xh wm, xh wh.
// At most 48 chained accumulations of 16 terms each: inside the bound the fp32 form has, Cin u |x| |W|^T with Cin = 128
// (tests/util.py::tap_products_bound).  The order depends on nothing but the output's own k index, so a column range of W gives
// the bits of the whole matrix, and a second call gives the bits of the first.
//
// Contract.  Inputs are finite with magnitudes whose low limb stays a normal number (|v| >~ 2^-110, or exactly 0): the split
// of a smaller value loses its low bits.  A non-finite input gives a non-finite output, but Inf - Inf in the split makes it
// NaN where fp32 arithmetic gives Inf.  Inputs that sit wholly in their high limb (small integers, k / 64) give the exact
// product sum.  Results are deterministic.
//
// Mapping.  Unlike the fp32 kernels of this code base the TOKEN sits on the MFMA row (A = x) and the output channel on the
// column (B = W): a register of the 32 x 32 accumulator then holds 32 consecutive outputs of one token in lanes 0..31 and of
// another in lanes 32..63, so every store instruction writes two whole 128-byte segments of z rows as it stands -- once the
// matrix side is cheap, the z writes are what the launch waits for.  (The transposed form stores 16-byte pieces, four partial
// writes per 64-byte line: 0.171 ms alone against 0.144 ms, profiles/tap_bf16x3.txt.)  A wave owns 32 tokens; lane (r = lane & 31, h =
// lane >> 5) loads channels 16 s + 8 h + 0..7 of token r for every k step s = 0..7 (two 16-byte buffer loads; a row past
// `tokens` uses an offset past the descriptor's end and reads 0), splits them once and keeps the 8 x 3 A fragments (96 VGPRs)
// for the whole walk over the output tiles -- 64 values per lane, 96 v_cvt_pk_bf16_f32 and 256 other vector instructions, once,
// against 48 MFMAs per tile.  The weights arrive pre-split
// (ops.tap_limbs_pack) as a stream of B fragments in consumption order,
//     [tile of 32 outputs][k step s][limb lo, mid, hi][lane][8 bf16]      lane (r, h): W_limb[32 tile + r][16 s + 8 h + j]
// 24 KB per tile, which the four waves of a block (128 tokens) consume in lock step from LDS: two buffers, one barrier per
// tile, tile o + 1 written to LDS from registers whose loads were issued two tiles earlier (two staging sets).  One
// ds_read_b128 per limb and k step feeds two or three MFMAs: 24 reads per 48 MFMAs.  Accumulator register g of lane (r, h) is
// output 32 o + r of token 4 h + (g & 3) + 8 (g >> 2) of the wave's 32: sixteen dword stores per tile, their row offsets
// computed once per wave, the tile's column as the instruction's scalar offset.
#include "conv_common.h"

namespace smos {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kTapC = 128;                 // input channels
constexpr int kTapKSteps = kTapC / 16;     // k steps of v_mfma_f32_32x32x16_bf16
constexpr int kTapTileQ = kTapKSteps * 3 * 64;   // u32x4 per tile of 32 outputs: 8 k steps x 3 limbs x 64 lanes
constexpr int kTapTileBytes = kTapTileQ * 16;    // 24 KB
constexpr int kTapStageQ = kTapTileQ / 256;      // u32x4 a thread stages per tile

struct TapJob {
  const float* x;       // [tokens, *] pitch xp
  const u32x4* wlimbs;  // tiles x 24 KB
  float* out;           // [tokens, *] pitch op
  int64_t xp, op;
  int cout, tiles;      // channels stored; 32-output tiles streamed
  int tokens;
};
struct TapArgs {
  TapJob job[8];
};

__device__ __forceinline__ unsigned tap_pack_bf16(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));      // round-to-nearest-even
  return r;
}

// two values -> their three limbs, packed in pairs
__device__ __forceinline__ void tap_split(float v0, float v1, unsigned& hi, unsigned& mid, unsigned& lo) {
  hi = tap_pack_bf16(v0, v1);
  float r0 = __fsub_rn(v0, __uint_as_float(hi << 16)), r1 = __fsub_rn(v1, __uint_as_float(hi & 0xffff0000u));
  mid = tap_pack_bf16(r0, r1);
  r0 = __fsub_rn(r0, __uint_as_float(mid << 16));
  r1 = __fsub_rn(r1, __uint_as_float(mid & 0xffff0000u));
  lo = tap_pack_bf16(r0, r1);
}

__device__ __forceinline__ bf16x8 tap_frag(u32x4 v) { return __builtin_bit_cast(bf16x8, v); }

#define TAP_GLOAD(set, tile_)                                                                             \
  do {                                                                                                    \
    _Pragma("unroll") for (int i_ = 0; i_ < kTapStageQ; ++i_)                                             \
        g[set][i_] = __builtin_amdgcn_raw_buffer_load_b128(wsrd, (unsigned)(tile_) * (unsigned)kTapTileBytes + i_ * 4096u + tid * 16u, 0, 0); \
  } while (0)
#define TAP_PARK(set, buf_)                                                                               \
  do {                                                                                                    \
    _Pragma("unroll") for (int i_ = 0; i_ < kTapStageQ; ++i_) lds[(buf_) * kTapTileQ + i_ * 256 + tid] = g[set][i_]; \
  } while (0)

// One tile of 32 outputs: barrier (tile o visible in buffer o & 1, everybody done with the other buffer), tile o + 1 goes from
// staging set SET into the other buffer and tile o + 3 is requested into that set; 48 MFMAs on one accumulator; sixteen stores.
#define TAP_TILE(o_, SET)                                                                                 \
  do {                                                                                                    \
    ring_barrier();                                                                                       \
    TAP_PARK(SET, ((o_) + 1) & 1);                                                                        \
    TAP_GLOAD(SET, (o_) + 3);                                                                             \
    const u32x4* rd_ = lds + ((o_) & 1) * kTapTileQ + lane;                                               \
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};       \
    _Pragma("unroll") for (int s_ = 0; s_ < kTapKSteps; ++s_) {                                           \
      const bf16x8 wl_ = tap_frag(rd_[(3 * s_ + 0) * 64]);                                                \
      const bf16x8 wm_ = tap_frag(rd_[(3 * s_ + 1) * 64]);                                                \
      const bf16x8 wh_ = tap_frag(rd_[(3 * s_ + 2) * 64]);                                                \
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xl[s_], wh_, acc, 0, 0, 0);                           \
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh[s_], wl_, acc, 0, 0, 0);                           \
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xm[s_], wm_, acc, 0, 0, 0);                           \
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xm[s_], wh_, acc, 0, 0, 0);                           \
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh[s_], wm_, acc, 0, 0, 0);                           \
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh[s_], wh_, acc, 0, 0, 0);                           \
    }                                                                                                     \
    const bool col_ok_ = 32 * (o_) + r < cout;                                                            \
    _Pragma("unroll") for (int g_ = 0; g_ < 16; ++g_)                                                     \
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[g_]), osrd, col_ok_ ? voff[g_] : 0x80000000u, 128 * (o_), 0); \
  } while (0)

__global__ __launch_bounds__(256, 2) void tap_bf16x3(TapArgs a) {
  extern __shared__ __attribute__((aligned(16))) u32x4 lds[];      // two tiles of 24 KB
  const TapJob& jb = a.job[blockIdx.y];
  const int tokens = jb.tokens, cout = jb.cout, tiles = jb.tiles, xp = (int)jb.xp, op = (int)jb.op;
  if ((int)blockIdx.x * 128 >= tokens) return;                     // a shorter job of the launch: the whole block leaves
  const __amdgpu_buffer_rsrc_t xsrd = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(jb.x), 0, tokens * xp * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t osrd = __builtin_amdgcn_make_buffer_rsrc(jb.out, 0, tokens * op * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t wsrd =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<u32x4*>(jb.wlimbs), 0, tiles * kTapTileBytes, 0x00020000);
  const unsigned tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int row0 = (int)blockIdx.x * 128 + wave * 32;              // the wave's first token
  const bool live = row0 + r < tokens;
  unsigned voff[16];          // accumulator register g: token 4 h + (g & 3) + 8 (g >> 2) of the wave's 32, column r of the tile
#pragma unroll
  for (int g_ = 0; g_ < 16; ++g_) {
    const int t = row0 + 4 * h + (g_ & 3) + 8 * (g_ >> 2);
    const unsigned v = ((unsigned)t * (unsigned)op + (unsigned)r) * 4u;      // unsigned: a row past `tokens` may wrap, it is not used
    voff[g_] = t < tokens ? v : 0x80000000u;
  }

  // the weight stream's first tiles and the token rows are requested together (a tile past the stream's end reads zeros)
  u32x4 g[2][kTapStageQ];
  TAP_GLOAD(0, 0);
  TAP_GLOAD(1, 1);
  const unsigned x_off = live ? ((unsigned)(row0 + r) * (unsigned)xp + 8u * h) * 4u : 0x80000000u;
  u32x4 xv[kTapKSteps][2];
#pragma unroll
  for (int s = 0; s < kTapKSteps; ++s) {
    xv[s][0] = __builtin_amdgcn_raw_buffer_load_b128(xsrd, x_off + 64u * s, 0, 0);
    xv[s][1] = __builtin_amdgcn_raw_buffer_load_b128(xsrd, x_off + 64u * s + 16u, 0, 0);
  }
  TAP_PARK(0, 0);
  TAP_GLOAD(0, 2);
  bf16x8 xh[kTapKSteps], xm[kTapKSteps], xl[kTapKSteps];
#pragma unroll
  for (int s = 0; s < kTapKSteps; ++s) {
    unsigned fh[4], fm[4], fl[4];
    tap_split(__uint_as_float(xv[s][0].x), __uint_as_float(xv[s][0].y), fh[0], fm[0], fl[0]);
    tap_split(__uint_as_float(xv[s][0].z), __uint_as_float(xv[s][0].w), fh[1], fm[1], fl[1]);
    tap_split(__uint_as_float(xv[s][1].x), __uint_as_float(xv[s][1].y), fh[2], fm[2], fl[2]);
    tap_split(__uint_as_float(xv[s][1].z), __uint_as_float(xv[s][1].w), fh[3], fm[3], fl[3]);
    xh[s] = tap_frag(u32x4{fh[0], fh[1], fh[2], fh[3]});
    xm[s] = tap_frag(u32x4{fm[0], fm[1], fm[2], fm[3]});
    xl[s] = tap_frag(u32x4{fl[0], fl[1], fl[2], fl[3]});
  }
  // two tiles per round, so that the staging set of a tile is a compile-time index; an odd count runs one tile of zeros past
  // the stream's end, whose columns are all >= cout: nothing of it is stored
#pragma unroll 1
  for (int o = 0; o < tiles; o += 2) {
    TAP_TILE(o, 1);
    TAP_TILE(o + 1, 0);
  }
}

}  // namespace smos

using namespace smos;

// out[j] = x[j] W[j]^T for up to eight jobs in one launch, fp32 in and out, computed as six bf16 limb products per term (header
// comment: accuracy and contract).  The job contract of smos_tfusion_project without a bias: x[j] [tokens[j], *] rows of 128
// channels, pitch x_pitch[j] floats (>= 128, a multiple of 4); wlimbs[j] = streammos_amd.ops.tap_limbs_pack(W[j]) (cout
// rounded up to a multiple of 32, zero padded); out[j] [tokens[j], *] rows of pitch out_pitch[j] >= cout[j] (a job may fill a
// column range of a wider matrix); cout a multiple of 4, <= 2048; 0 < tokens < 2^22; operands below 2 GiB.
extern "C" int smos_tap_products_bf16x3(int32_t n_jobs, const float* const* x, const int64_t* x_pitch, const void* const* wlimbs,
                                        float* const* out, const int64_t* out_pitch, const int64_t* cout, const int64_t* tokens,
                                        smos_stream_t stream) {
  SMOS_REQUIRE(n_jobs >= 1 && n_jobs <= 8 && x && x_pitch && wlimbs && out && out_pitch && cout && tokens,
               "tap_products_bf16x3: 1..8 jobs");
  TapArgs a;
  int64_t most = 0;
  for (int j = 0; j < n_jobs; ++j) {
    SMOS_REQUIRE(x[j] && wlimbs[j] && out[j] && x_pitch[j] >= kTapC && x_pitch[j] % 4 == 0 && cout[j] > 0 && cout[j] % 4 == 0 &&
                     cout[j] <= 2048 && out_pitch[j] >= cout[j] && out_pitch[j] % 4 == 0 && tokens[j] > 0 && tokens[j] < (1LL << 22),
                 "tap_products_bf16x3: bad job (pitch >= 128, cout a multiple of 4 and <= 2048, out pitch >= cout, 0 < tokens < 2^22)");
    SMOS_REQUIRE(((reinterpret_cast<uintptr_t>(x[j]) | reinterpret_cast<uintptr_t>(wlimbs[j]) | reinterpret_cast<uintptr_t>(out[j])) & 15) == 0,
                 "tap_products_bf16x3: pointers must be 16-byte aligned");
    SMOS_REQUIRE(tokens[j] * x_pitch[j] * 4 < (1LL << 31) && tokens[j] * out_pitch[j] * 4 < (1LL << 31),
                 "tap_products_bf16x3: an operand larger than 2 GiB");
    a.job[j].x = x[j]; a.job[j].wlimbs = reinterpret_cast<const u32x4*>(wlimbs[j]); a.job[j].out = out[j];
    a.job[j].xp = x_pitch[j]; a.job[j].op = out_pitch[j]; a.job[j].cout = (int)cout[j]; a.job[j].tiles = (int)((cout[j] + 31) / 32);
    a.job[j].tokens = (int)tokens[j];
    most = tokens[j] > most ? tokens[j] : most;
  }
  for (int j = n_jobs; j < 8; ++j) a.job[j] = a.job[0];
  const size_t lds = (size_t)2 * kTapTileBytes;
  KernelSetup ks;
  if (int rc = kernel_setup(reinterpret_cast<const void*>(&tap_bf16x3), lds, 0, &ks, "tap_bf16x3")) return rc;
  hipLaunchKernelGGL(tap_bf16x3, dim3((unsigned)((most + 127) / 128), (unsigned)n_jobs), dim3(256), lds, (hipStream_t)stream, a);
  return check_launch("tap_bf16x3");
}
