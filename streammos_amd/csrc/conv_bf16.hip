// Channels-last convolution on the bf16 matrix cores (the opt-in conv_precision="bf16" mode of the engine): the contract of
// smos_conv_cl (KH, KW <= 7, stride 1 or 2, explicit padding, Cin and Cout multiples of 32, act none / ReLU / LeakyReLU,
// optional bias / residual / channel sums, channel slices of wider buffers) with both operands rounded to bf16:
//
//     out = act( sum_{tap, cin} bf16(W[cout][cin][tap]) * bf16(X[pixel * stride + tap - pad][cin]) + bias [+ residual] )
//
// Products are exact, the sum runs in fp32 (v_mfma_f32_32x32x16_bf16), bias / residual / activation / channel sums / the
// stored output are fp32.  The weights are rounded once on the host (ops.conv_bf16_prepare, round-to-nearest-even), the
// activations when they are staged (v_cvt_pk_bf16_f32, round-to-nearest-even).
//
// Transposed form as in csrc/conv_igemm.hip: output channel on the MFMA row (A = weights), 32 consecutive output pixels of
// one image row on the column (B = activations).  What does not carry over from conv_igemm is its B operand: in fp32 one
// 32-channel x one-tap stage is 16 MFMAs per 32-channel output block and the per-tap re-reads of fp32 activations from L1 / L2
// hide behind them; in bf16 the same stage is 2 MFMAs at 1/16 of the cycles, so those re-reads would bound the kernel.
//
//   work item  = rb output rows x 32 columns x (32 * MT * wc) output channels.  The block's 4 waves are wc cout groups x
//                (4 / wc) row groups; a wave owns RW rows x 32 columns x 32 * MT channels (RW * MT accumulator tiles).
//                Persistent blocks own contiguous item ranges, XCD-aware (as conv_igemm).
//   stage      = one 32-channel chunk x one tap; the K loop of an item is (chunk, ky, kx), 2 * RW * MT MFMAs per wave.
//   B operand  = the item's input region (rb output rows plus halo x 32 columns plus halo) of ONE channel chunk, staged
//                once per chunk into LDS as bf16 (converted during the fill; 80-byte pixels = 32 channels + 16 bytes of pad,
//                conflict-free ds_read_b128 at stride 1).  Every tap reads its fragments from there, and each fragment
//                serves all MT output tiles of the wave.  The next chunk's region is requested into registers at the
//                chunk's first tap (through a buffer descriptor: lanes outside the image read zeros) and written at its
//                last tap, between two barriers (one region buffer: LDS stays low enough for >= 2 blocks per CU).
//   A operand  = bf16 weights, pre-packed in fragment order, streamed through a four-slot LDS ring: the slice of stage
//                g + 3 is requested in stage g into one of two register sets and parked in the ring in stage g + 2.
//   waits      = every weight slice is requested two stages before it is parked; the region one chunk ahead; the residual
//                tile at the first stage of the item's last chunk.  No global load sits under a lane-dependent branch and
//                the epilogue issues no load (bias lives in LDS).
//   epilogue   = out = act(acc + bias [+ residual]) from the accumulators, 16-byte stores; channel sums per 32-pixel row
//                segment in the table layout of smos_conv_cl (smos_conv_cl_sum_chunks), so channel_gate_apply reads them.
//
// Every output element is summed by one wave in one fixed order (chunk, ky, kx, k-step), whatever the block shape: results
// are bit-identical from run to run and across grid sizes, streams, batch sizes and block configurations.
#include <stdio.h>
#include <stdlib.h>

#include "conv_common.h"

namespace smos {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

struct ConvBf16Args {
  const float* x;      // [B, H, W, *] row pitch xp (floats)
  const u32x4* w;      // bf16 operand order (smos.h): [stage][Cout / 32][k-step][lane][8]
  const float* bias;   // [Cout] or null
  const float* res;    // [B, Ho, Wo, *] row pitch rp, or null
  float* out;          // [B, Ho, Wo, *] row pitch op
  float* sums;         // SUMS: [B][hq * xt * 4][Cout]
  int64_t xp, rp, op;
  int B, H, W, Ho, Wo;
  int KH, KW, S, PH, PW;
  int ntap, nstage;    // KH * KW, ntap * Cin / 32
  int wc, rb;          // cout groups per block (1, 2, 4), output rows per block ((4 / wc) * RW)
  int nq;              // Cout / 32
  int nct, hb, xt, hq; // cout tiles (Cout / (32 * MT * wc)), row groups ceil(Ho / rb), column tiles ceil(Wo / 32), ceil(Ho / 4)
  int n_items;         // B * hb * xt * nct
  int rr, cc, n_units; // staged region: rows (rb - 1) * S + KH, columns 31 * S + KW, 8-channel units rr * cc * 4
  float slope;         // activation: max(v, 0) + slope * min(v, 0)
  SMOS_STAMPS_ARG      // diagnostic builds only (conv_diag.h, tools/conv_bf16_stamps.py)
  int x_bytes, r_bytes, o_bytes, w_bytes, cout;
};

constexpr int kPixQ = 5;          // u32x4 per staged pixel: 32 bf16 channels + 16 bytes of pad (80 B)
constexpr int kUnits = 8;         // 8-channel units a thread stages per chunk: regions of <= 2048 units
constexpr int kLdsBudget = 80 * 1024;

__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));      // round-to-nearest-even
  return r;
}

template <int MT, int RW, bool RES, bool SUMS>
__global__ __launch_bounds__(256, 2) void conv_bf16(ConvBf16Args a) {
  extern __shared__ __attribute__((aligned(16))) u32x4 lds[];   // ring 4 x slot_q | region rr * cc * 5 | bias Cout floats
  const int G = a.wc * MT;                  // 32-channel output blocks per item
  const int slot_q = G * 128;               // u32x4 per ring slot (G blocks x 2 k-steps x 64 lanes)
  u32x4* ring = lds;
  u32x4* region = lds + 4 * slot_q;
  float* bias_lds = reinterpret_cast<float*>(region + a.rr * a.cc * kPixQ);
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int p = lane & 31, h = lane >> 5;
  const int wcg = wave % a.wc, wr = wave / a.wc;      // this wave's cout group and row group

  const int per_block = (a.n_items + (int)gridDim.x - 1) / (int)gridDim.x;
  const int nb = (int)gridDim.x, xq = nb >> 3, xr = nb & 7, xcd = (int)blockIdx.x & 7;
  const int lblock = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + ((int)blockIdx.x >> 3);
  const int first = lblock * per_block;
  const int iters = a.n_items - first < per_block ? a.n_items - first : per_block;
  const int total = iters * a.nstage;
  if (total <= 0) return;

  struct Item {
    int b, yb, x0, ct;
    bool valid;
  };
  auto item_of = [&](int it) {
    Item t;
    t.valid = it < iters;
    const int q = t.valid ? first + it : first;
    t.ct = q % a.nct;
    int u = q / a.nct;
    t.x0 = (u % a.xt) * 32;
    u /= a.xt;
    t.yb = (u % a.hb) * a.rb;
    t.b = u / a.hb;
    return t;
  };

  const __amdgpu_buffer_rsrc_t xsrd = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, a.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t wsrd = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32x4*>(a.w), 0, a.w_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrd =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.res), 0, a.res ? a.r_bytes : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t osrd = __builtin_amdgcn_make_buffer_rsrc(a.out, 0, a.o_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t bsrd =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.bias), 0, a.bias ? a.cout * 4 : 0, 0x00020000);
  float bias_r[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) bias_r[k] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(bsrd, (unsigned)(tid + 256 * k) * 4u, 0, 0));

  // ---- weight slices: stage g of the stream = stage s of item it; slice = G consecutive 2 KB blocks ----
  int pw_s = 0, pw_it = 0, pw_ct = item_of(0).ct;
  auto load_w = [&](u32x4 (&wr_)[2]) {
    const bool ok = pw_it < iters;
    const unsigned base = (unsigned)((pw_s * a.nq + pw_ct * G) * 128);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const unsigned e = (unsigned)(tid + 256 * k);
      const unsigned off = (ok & (e < (unsigned)slot_q)) ? (base + e) * 16u : 0x80000000u;
      wr_[k] = __builtin_amdgcn_raw_buffer_load_b128(wsrd, off, 0, 0);
    }
    if (++pw_s == a.nstage) {        // wave-uniform
      pw_s = 0;
      ++pw_it;
      pw_ct = item_of(pw_it).ct;
    }
  };
  auto park = [&](const u32x4 (&wr_)[2], int slot) {
#pragma unroll
    for (int k = 0; k < 2; ++k)
      if (tid + 256 * k < slot_q) ring[slot * slot_q + tid + 256 * k] = wr_[k];
  };

  // ---- input region: this thread's units (pixel of the region, 8-channel group) are the same for every item and chunk ----
  int urc[kUnits];                   // (row << 8 | column) of the region pixel, or -1 past the region
#pragma unroll
  for (int k = 0; k < kUnits; ++k) {
    const int u = tid + 256 * k;
    const int pix = u >> 2;
    urc[k] = u < a.n_units ? ((pix / a.cc) << 8) | (pix % a.cc) : -1;
  }
  u32x4 xr_[2 * kUnits];
  auto load_region = [&](int it, int ch) {
    const Item t = item_of(it);
    const int y0 = t.yb * a.S - a.PH, x0 = t.x0 * a.S - a.PW;
    const int xp = (int)a.xp;
#pragma unroll
    for (int k = 0; k < kUnits; ++k) {
      const int yi = y0 + (urc[k] >> 8), xi = x0 + (urc[k] & 255);
      const bool ok = t.valid & (urc[k] >= 0) & ((unsigned)yi < (unsigned)a.H) & ((unsigned)xi < (unsigned)a.W);
      const unsigned off = ok ? (unsigned)(((t.b * a.H + yi) * a.W + xi) * xp + ch * 32 + (tid & 3) * 8) * 4u : 0x80000000u;
      xr_[2 * k] = __builtin_amdgcn_raw_buffer_load_b128(xsrd, off, 0, 0);
      xr_[2 * k + 1] = __builtin_amdgcn_raw_buffer_load_b128(xsrd, off + 16u, 0, 0);
    }
  };
  auto write_region = [&]() {
#pragma unroll
    for (int k = 0; k < kUnits; ++k) {
      const u32x4 lo = xr_[2 * k], hi = xr_[2 * k + 1];
      u32x4 v;
      v.x = pack_bf16(__uint_as_float(lo.x), __uint_as_float(lo.y));
      v.y = pack_bf16(__uint_as_float(lo.z), __uint_as_float(lo.w));
      v.z = pack_bf16(__uint_as_float(hi.x), __uint_as_float(hi.y));
      v.w = pack_bf16(__uint_as_float(hi.z), __uint_as_float(hi.w));
      const int u = tid + 256 * k;
      if (urc[k] >= 0) region[(u >> 2) * kPixQ + (u & 3)] = v;
    }
  };

  f32x16 acc[RW][MT];
#pragma unroll
  for (int rw = 0; rw < RW; ++rw)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[rw][mt][r] = 0.0f;

  // ---- the stage being computed ----
  const int nch = a.nstage / a.ntap;
  int c_s = 0, c_it = 0, c_ch = 0, c_ky = 0, c_kx = 0;
  Item cur = item_of(0);
  const int lane_b = p * a.S * kPixQ + h;           // this lane's pixel column (times stride) and k half in the region

  u32x4 rres[RES ? 4 * RW * MT : 1];
  auto request_residual = [&]() {
    if constexpr (RES) {
      const int x = cur.x0 + p;
#pragma unroll
      for (int rw = 0; rw < RW; ++rw) {
        const int y = cur.yb + wr * RW + rw;
        const bool want = (y < a.Ho) & (x < a.Wo);
        const int pix = (cur.b * a.Ho + y) * a.Wo + x;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const int cb = (cur.ct * G + wcg * MT + mt) * 32 + 4 * h;
          const unsigned roff = want ? (unsigned)(pix * (int)a.rp + cb) * 4u : 0x80000000u;
#pragma unroll
          for (int g = 0; g < 4; ++g) rres[(rw * MT + mt) * 4 + g] = __builtin_amdgcn_raw_buffer_load_b128(rsrd, roff + 32u * g, 0, 0);
        }
      }
    }
  };

  auto epilogue = [&]() {
    const int x = cur.x0 + p;
#pragma unroll
    for (int rw = 0; rw < RW; ++rw) {
      const int y = cur.yb + wr * RW + rw;
      const bool store = (y < a.Ho) & (x < a.Wo);
      const int pix = (cur.b * a.Ho + y) * a.Wo + x;
      float* srow = nullptr;
      if constexpr (SUMS) {
        // row segment (y, x0 .. x0 + 31) = chunk ((y / 4) * xt + x0 / 32) * 4 + y % 4; rows past the image but inside the
        // table (y < 4 * hq) write zeros -- the host sizes the row groups to cover all 4 * hq rows under SUMS, so every
        // chunk of the table is written
        const int chunk = (((y >> 2) * a.xt + (cur.x0 >> 5)) << 2) + (y & 3);
        srow = y < 4 * a.hq ? a.sums + ((int64_t)cur.b * (a.hq * a.xt * 4) + chunk) * a.cout : nullptr;
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int cb = (cur.ct * G + wcg * MT + mt) * 32 + 4 * h;
        const unsigned ooff = store ? (unsigned)(pix * (int)a.op + cb) * 4u : 0x80000000u;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float4 bv = *reinterpret_cast<const float4*>(bias_lds + cb + 8 * g);
          const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
          float o[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            float v = acc[rw][mt][4 * g + c] + bb[c];
            if constexpr (RES) v += __uint_as_float(rres[(rw * MT + mt) * 4 + g][c]);
            o[c] = conv_act(v, a.slope);
            acc[rw][mt][4 * g + c] = 0.0f;
          }
          if constexpr (SUMS) {
            float4 sv;
            sv.x = half_wave_sum(store ? o[0] : 0.f);
            sv.y = half_wave_sum(store ? o[1] : 0.f);
            sv.z = half_wave_sum(store ? o[2] : 0.f);
            sv.w = half_wave_sum(store ? o[3] : 0.f);
            if (p == 31 && srow) *reinterpret_cast<float4*>(srow + cb + 8 * g) = sv;
          }
          u32x4 ov;
          ov.x = __float_as_uint(o[0]); ov.y = __float_as_uint(o[1]); ov.z = __float_as_uint(o[2]); ov.w = __float_as_uint(o[3]);
          __builtin_amdgcn_raw_buffer_store_b128(ov, osrd, ooff + 32u * g, 0, 0);
        }
      }
    }
  };

  auto compute = [&](int slot) {
    const int rbase = ((wr * RW * a.S + c_ky) * a.cc + c_kx) * kPixQ + lane_b;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 bf[RW], af[MT];
#pragma unroll
      for (int rw = 0; rw < RW; ++rw) bf[rw] = __builtin_bit_cast(bf16x8, region[rbase + rw * a.S * a.cc * kPixQ + 2 * ks]);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        af[mt] = __builtin_bit_cast(bf16x8, ring[slot * slot_q + ((wcg * MT + mt) * 2 + ks) * 64 + lane]);
#pragma unroll
      for (int rw = 0; rw < RW; ++rw)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[rw][mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[mt], bf[rw], acc[rw][mt], 0, 0, 0);
    }
  };

  // ---- prologue: slice 0 in the ring, slices 1 and 2 in registers, the first region and the bias in LDS ----
  u32x4 wa[2], wb[2];
  load_w(wa);
  park(wa, 0);
  load_w(wa);
  load_w(wb);
  load_region(0, 0);
  write_region();
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (256 * k + tid < a.cout) bias_lds[tid + 256 * k] = bias_r[k];
  ring_barrier();

  // one stage g (wn holds slice g + 1):
  //   park slice g + 1 in slot (g + 1) % 4 (last read in stage g - 3), request slice g + 3 into wn;
  //   first tap of a chunk: request the next chunk's region (this item's next chunk, or the next item's first);
  //   first stage of the item's last chunk: request the residual tile;
  //   2 * RW * MT MFMAs from slot g % 4 and the region;
  //   last tap of a chunk: barrier (every wave is done with the region), then write the requested region;
  //   last stage of the item: epilogue; barrier.
  // diagnostic builds (-DSMOS_CONV_STAMPS): cycles per segment -- 0 weight ring, 1 region / residual requests, 2 fragments +
  // MFMAs, 3 region write (barrier, wait, convert, store), 4 epilogue, 5 end-of-stage barrier, 6 stage bookkeeping
  SMOS_STAMPS_DECLARE();
  auto stage = [&](u32x4 (&wn)[2], int g) {
    SMOS_STAMP(6);
    park(wn, (g + 1) & 3);
    load_w(wn);
    SMOS_STAMP(0);
    const bool chunk_first = (c_ky | c_kx) == 0;
    const bool chunk_last = c_ky == a.KH - 1 && c_kx == a.KW - 1;
    const bool item_last = c_s == a.nstage - 1;
    if (chunk_first) {
      if (c_ch + 1 < nch) load_region(c_it, c_ch + 1);
      else load_region(c_it + 1, 0);
    }
    if (RES && c_s == a.nstage - a.ntap) request_residual();
    SMOS_STAMP(1);
    compute(g & 3);
    SMOS_STAMP(2);
    if (chunk_last) {
      ring_barrier();
      write_region();
    }
    SMOS_STAMP(3);
    if (item_last) epilogue();
    SMOS_STAMP(4);
    ring_barrier();
    SMOS_STAMP(5);
    // advance (wave-uniform)
    ++c_s;
    if (++c_kx == a.KW) {
      c_kx = 0;
      if (++c_ky == a.KH) {
        c_ky = 0;
        ++c_ch;
      }
    }
    if (c_s == a.nstage) {
      c_s = c_ch = 0;
      ++c_it;
      cur = item_of(c_it);
    }
  };

  SMOS_STAMPS_BEGIN();
  int g = 0;
#pragma unroll 1
  for (; g + 2 <= total; g += 2) {
    stage(wa, g);
    stage(wb, g + 1);
  }
  if (g < total) stage(wa, g);
  SMOS_STAMPS_END();
}

}  // namespace smos

using namespace smos;

namespace {

struct Bf16Cfg {
  int mt = 0, wc = 0, rw = 0, rb = 0, rr = 0, cc = 0;
  size_t lds = 0;
};

// Block shapes the kernel is instantiated for; false if none fits (region > 2048 units or LDS over budget).
bool pick_cfg(int64_t B, int64_t Ho, int64_t Wo, int64_t Cout, int KH, int KW, int S, bool res, Bf16Cfg* out) {
  const int64_t nq = Cout / 32;
  bool found = false;
  int64_t best_key = -1;
  for (int mt : {4, 2, 1})
    for (int wc : {1, 2, 4})
      for (int rw : {2, 1}) {
        const int G = mt * wc;
        if (G > 4 || nq % G || mt * rw > 4 || (res && mt * rw > 2)) continue;
        const int rb = (4 / wc) * rw, rr = (rb - 1) * S + KH, cc = 31 * S + KW;
        if (rr * cc * 4 > 256 * kUnits) continue;
        const size_t lds = (size_t)(4 * G * 128 + rr * cc * kPixQ) * 16 + (size_t)Cout * 4;
        if (lds > (size_t)kLdsBudget) continue;
        // enough items to give every CU two blocks, then the widest cout group (least re-staging), the widest wave tile
        const int64_t items = B * ((Ho + rb - 1) / rb) * ((Wo + 31) / 32) * (nq / G);
        const int64_t key = ((items < 512 ? items : 512) * 8 + G) * 64 + mt * 8 + rw;
        if (key > best_key) {
          best_key = key;
          out->mt = mt; out->wc = wc; out->rw = rw; out->rb = rb; out->rr = rr; out->cc = cc; out->lds = lds;
          found = true;
        }
      }
  return found;
}

template <int MT, int RW, bool RES, bool SUMS>
int launch_bf16(const ConvBf16Args& a, size_t lds, hipStream_t s) {
  KernelSetup ks;
  if (int rc = kernel_setup(reinterpret_cast<const void*>(&conv_bf16<MT, RW, RES, SUMS>), kLdsBudget, 0, &ks, "conv_bf16_cl"))
    return rc;
  int per_cu = (int)(160 * 1024 / lds);
  per_cu = per_cu < 1 ? 1 : per_cu > 2 ? 2 : per_cu;
  const int64_t cap = conv_grid_cap((int64_t)ks.cus * per_cu);
  const unsigned grid = (unsigned)(a.n_items < cap ? a.n_items : cap);
  hipLaunchKernelGGL((conv_bf16<MT, RW, RES, SUMS>), dim3(grid), dim3(256), lds, s, a);
  return check_launch("conv_bf16_cl");
}

template <bool RES, bool SUMS>
int dispatch(const ConvBf16Args& a, const Bf16Cfg& c, hipStream_t s) {
  if constexpr (!RES) {       // a residual tile in registers: mt * rw <= 2 (pick_cfg)
    if (c.mt == 4) return launch_bf16<4, 1, RES, SUMS>(a, c.lds, s);
    if (c.mt == 2 && c.rw == 2) return launch_bf16<2, 2, RES, SUMS>(a, c.lds, s);
  }
  if (c.mt == 2) return launch_bf16<2, 1, RES, SUMS>(a, c.lds, s);
  return c.rw == 2 ? launch_bf16<1, 2, RES, SUMS>(a, c.lds, s) : launch_bf16<1, 1, RES, SUMS>(a, c.lds, s);
}

}  // namespace

extern "C" int smos_conv_bf16_cl_supported(int64_t Cin, int64_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t has_res) {
  if (Cin <= 0 || Cout <= 0 || Cin % 32 || Cout % 32 || Cout > 2048 || KH < 1 || KW < 1 || KH > 7 || KW > 7 ||
      (stride != 1 && stride != 2))
    return 0;
  Bf16Cfg c;
  return pick_cfg(1, 1, 1, Cout, KH, KW, stride, has_res != 0, &c) ? 1 : 0;
}

extern "C" int smos_conv_bf16_cl(const float* x, int64_t x_pitch, const uint16_t* wprep, const float* bias, const float* res,
                                 int64_t res_pitch, float* out, int64_t out_pitch, int64_t B, int64_t H, int64_t W, int64_t Cin,
                                 int64_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad_h, int32_t pad_w, int32_t act,
                                 float* chan_sums, smos_stream_t stream) {
  SMOS_REQUIRE(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && Cin % 32 == 0 && Cout % 32 == 0,
               "conv_bf16_cl: Cin and Cout must be multiples of 32");
  SMOS_REQUIRE(KH >= 1 && KW >= 1 && KH <= 7 && KW <= 7 && (stride == 1 || stride == 2) && pad_h >= 0 && pad_w >= 0 &&
                   act >= 0 && act <= 2, "conv_bf16_cl: kernel up to 7 x 7, stride 1 or 2");
  const int64_t Ho = (H + 2 * pad_h - KH) / stride + 1, Wo = (W + 2 * pad_w - KW) / stride + 1;
  SMOS_REQUIRE(H + 2 * pad_h >= KH && W + 2 * pad_w >= KW && Ho > 0 && Wo > 0, "conv_bf16_cl: empty output");
  ConvBytes nb;
  if (int rc = conv_check_operands("conv_bf16_cl", x, x_pitch, wprep, bias, res, res_pitch, out, out_pitch, chan_sums, Cin, Cout,
                                   B * H * W, B * Ho * Wo, &nb))
    return rc;
  Bf16Cfg c;
  SMOS_REQUIRE(pick_cfg(B, Ho, Wo, Cout, KH, KW, stride, res != nullptr, &c),
               "conv_bf16_cl: no block shape fits this kernel / stride (smos_conv_bf16_cl_supported)");
  const int64_t nq = Cout / 32, G = c.mt * c.wc;
  // with channel sums the row groups span the whole table (4 * ceil(Ho / 4) rows, those past Ho written as zeros), whatever
  // the block's row count rb: the rows of a table row segment past Ho belong to no output row group otherwise
  const int64_t rows = chan_sums ? (Ho + 3) / 4 * 4 : Ho;
  const int64_t hb = (rows + c.rb - 1) / c.rb, xt = (Wo + 31) / 32, nct = nq / G;
  SMOS_REQUIRE(B * hb * xt * nct < (1LL << 30) && Cout * Cin * KH * KW * 2 < (1LL << 31), "conv_bf16_cl: too many tiles");
  ConvBf16Args a;
  a.x = x; a.w = reinterpret_cast<const u32x4*>(wprep); a.bias = bias; a.res = res; a.out = out; a.sums = chan_sums;
  a.xp = x_pitch; a.rp = res_pitch; a.op = out_pitch;
  a.B = (int)B; a.H = (int)H; a.W = (int)W; a.Ho = (int)Ho; a.Wo = (int)Wo;
  a.KH = KH; a.KW = KW; a.S = stride; a.PH = pad_h; a.PW = pad_w;
  a.ntap = KH * KW; a.nstage = a.ntap * (int)(Cin / 32);
  a.wc = c.wc; a.rb = c.rb; a.nq = (int)nq;
  a.nct = (int)nct; a.hb = (int)hb; a.xt = (int)xt; a.hq = (int)((Ho + 3) / 4);
  a.n_items = (int)(B * hb * xt * nct);
  a.rr = c.rr; a.cc = c.cc; a.n_units = c.rr * c.cc * 4;
  a.slope = act_slope(act);
  SMOS_STAMPS_HOST(a);
  a.x_bytes = nb.x;
  a.r_bytes = nb.r;
  a.o_bytes = nb.o;
  a.w_bytes = (int)(Cout * Cin * KH * KW * 2);
  a.cout = (int)Cout;
  const hipStream_t s = (hipStream_t)stream;
  if (chan_sums) return dispatch<false, true>(a, c, s);
  if (res) return dispatch<true, false>(a, c, s);
  return dispatch<false, false>(a, c, s);
}
