// Shared by the conv kernels: argument block, ring barrier, scheduling fence, half-wave sum (csrc/conv_igemm.hip and
// csrc/conv_rows.hip) and the host-side operand checks of every conv entry point.
#pragma once
#include "smos_common.h"
#include "conv_diag.h"

namespace smos {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct ConvArgs {
  const float* x;      // [B, H, W, *] row pitch xp (floats)
  const float4* w;     // operand order [cout tile][stage][k-step / 4][mt][lane][k-step % 4]
  const float* bias;   // [Cout] or null
  const float* res;    // [B, Ho, Wo, *] row pitch rp, or null
  float* out;          // [B, Ho, Wo, *] row pitch op
  float* sums;         // SUMS: [B][hq * xt * 4][Cout] per-(item, row) channel sums of the output, or unused
  int64_t xp, rp, op;
  int B, H, W, Ho, Wo;
  int KH, KW, S, PH, PW;
  int nch;             // Cin / 32
  int nstage;          // KH * KW * nch
  int nct;             // Cout / (32 * MT)
  int hq, xt;          // ceil(Ho / 4), ceil(Wo / 32)
  int n_items;         // B * hq * xt * nct
  float slope;         // activation: max(v, 0) + slope * min(v, 0) -- 1 none, 0 ReLU, 0.01 LeakyReLU
  SMOS_STAMPS_ARG
  int x_bytes;         // B * H * W * xp * 4 (< 2^31: lanes outside the image use offset 2^31)
  int r_bytes, o_bytes, cout;   // B * Ho * Wo * rp * 4, B * Ho * Wo * op * 4, Cout
};

// Ring barrier.  __syncthreads() would also do, but its workgroup fence makes hipcc wait vmcnt(0) -- draining the operand
// prefetch once per stage.  Only LDS traffic has to be ordered here: every wave drains its own LDS queue (ring stores
// landed, fragment reads returned), then the barrier.  The "memory" clobbers keep the compiler from moving ring accesses
// across it.
__device__ __forceinline__ void ring_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if (SMOS_CONV_KEEPS(1)) __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// Scheduling fence: a wave issues in order, and an MFMA that depends on the previous one (same accumulator) cannot issue
// before it has finished (64 cycles) -- so everything that is NOT an MFMA only overlaps with the matrix pipe if it sits
// BETWEEN MFMAs in program order.  The stage body below is cut into MFMA groups (G) and small bookkeeping segments (M);
// the fences keep hipcc from collecting the segments in front of or behind the MFMA block.
#define SMOS_FENCE()                                                                          \
  do {                                                                                        \
    asm volatile("" ::: "memory"); /* IR level: loads and stores stay on their side */        \
    __builtin_amdgcn_sched_barrier(0); /* machine scheduler: nothing crosses, MFMAs included */ \
  } while (0)

// Sum over the 32 lanes of each half wave, delivered in its last lane (31 / 63): four row_shr steps inside the 16-lane DPP
// rows (an inclusive scan by doubling; lanes without a source read 0), then row_bcast:15 carries lane 15 / 47 into the next
// row.  One fixed order, so the sums are run-to-run identical.
__device__ __forceinline__ float half_wave_sum(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xF, 0xF, true));   // row_shr:1
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x112, 0xF, 0xF, true));   // row_shr:2
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x114, 0xF, 0xF, true));   // row_shr:4
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x118, 0xF, 0xF, true));   // row_shr:8
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x142, 0xA, 0xF, false));  // row_bcast:15 -> rows 1, 3
  return v;
}

struct ConvTile {      // where a wave's 32-pixel row segment lies (everything scalar; recomputed once per tile)
  int b, y, x0, ct;
  bool valid;
};

// Host side, shared by the extern "C" entry points of the conv kernels (`who`: the entry point's name, the prefix of its
// error messages).  An entry point keeps its own shape rules and checks them first (the pixel counts here are positive).
struct ConvBytes {
  int x, r, o;         // B * H * W * x_pitch * 4, B * Ho * Wo * res_pitch * 4 (0 without a residual), B * Ho * Wo * out_pitch * 4
};

// The operand rules every conv kernel has: x / wprep / out present, row pitches (floats) that cover the channels and keep
// rows 16-byte aligned, every pointer 16-byte aligned, every map below 2 GiB (the kernels address through 32-bit buffer
// offsets; the byte counts come back in *bytes), at most 2048 output channels, channel sums only without a residual.
// res / chan_sums are null where the kernel takes none.
inline int conv_check_operands(const char* who, const void* x, int64_t x_pitch, const void* wprep, const void* bias, const void* res,
                               int64_t res_pitch, const void* out, int64_t out_pitch, const void* chan_sums, int64_t Cin,
                               int64_t Cout, int64_t in_pixels, int64_t out_pixels, ConvBytes* bytes) {
  SMOS_REQUIRE(Cout <= 2048, "%s: more than 2048 output channels", who);
  SMOS_REQUIRE(x && wprep && out && x_pitch >= Cin && out_pitch >= Cout && x_pitch % 4 == 0 && out_pitch % 4 == 0 &&
                   (!res || (res_pitch >= Cout && res_pitch % 4 == 0)), "%s: null pointer / bad pitch", who);
  SMOS_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(res) |
                 reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(wprep) | reinterpret_cast<uintptr_t>(chan_sums)) & 15) == 0,
               "%s: pointers must be 16-byte aligned", who);
  SMOS_REQUIRE(in_pixels * x_pitch * 4 < (1LL << 31) && out_pixels * out_pitch * 4 < (1LL << 31) &&
                   (!res || out_pixels * res_pitch * 4 < (1LL << 31)), "%s: a tensor larger than 2 GiB (32-bit buffer offsets)", who);
  SMOS_REQUIRE(!(chan_sums && res), "%s: channel sums need res == NULL", who);
  bytes->x = (int)(in_pixels * x_pitch * 4);
  bytes->r = res ? (int)(out_pixels * res_pitch * 4) : 0;
  bytes->o = (int)(out_pixels * out_pitch * 4);
  return SMOS_OK;
}

// activation code of the C ABI (0 none, 1 ReLU, 2 LeakyReLU) -> slope of max(v, 0) + slope * min(v, 0)
inline float act_slope(int act) { return act == 0 ? 1.0f : act == 1 ? 0.0f : 0.01f; }

// none / ReLU / LeakyReLU without a branch: max(v, 0) + slope * min(v, 0), slope = 1 / 0 / 0.01 (one of the two terms is
// always zero, so this is exact).  The maximum is a select, not fmaxf: fmaxf(NaN, 0) and fminf(NaN, 0) are both 0, which
// turned a NaN sum into a stored 0 -- the reference's ReLU / LeakyReLU hand a NaN on, and so does this (NaN <= 0 is false).
// For every other v the select is fmaxf(v, 0): the stored bits are unchanged.
__device__ __forceinline__ float conv_act(float v, float slope) {
  return __builtin_fmaf(slope, fminf(v, 0.f), v <= 0.f ? 0.f : v);
}

}  // namespace smos
