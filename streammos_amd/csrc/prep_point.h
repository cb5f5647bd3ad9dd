// Per-point arithmetic of the device-side preprocessing, shared by the validation kernels (csrc/preprocess.hip) and the
// training sample builder (csrc/train_prep.hip): the grid geometry, BEV / range-view quantisation (datasets/utils.py:151-192)
// and the 7-channel point feature (datasets/data_StreamMOS.py:25-50).  One definition: the same bits in both paths.
#pragma once
#include "smos_common.h"

namespace smos {

struct PrepGeom {
  float lo[3], hi[3], cell[3];
  float phi_hi, dphi, th_hi, dtheta;
};

struct EmitArgs {
  const float* moved;     // [n, 4]
  const int32_t* mask;    // [n]
  const int32_t* prefix;  // [n] inclusive prefix sum of mask
  float* xyzi;            // [V, T, 7, N]
  float* coord;           // [V, T, N, 3]
  float* sphere;          // [V, T, N, 2]
  int64_t n, N;
  int t, T, V;
  float sx[4], sy[4];
  PrepGeom g;
};

__device__ __forceinline__ void emit_point(const EmitArgs& a, int64_t j, float x0, float y0, float z, float inten) {
#pragma unroll 1
  for (int v = 0; v < a.V; ++v) {
    const float x = __fmul_rn(x0, a.sx[v]), y = __fmul_rn(y0, a.sy[v]);
    const float qx = __fdiv_rn(__fsub_rn(x, a.g.lo[0]), a.g.cell[0]);
    const float qy = __fdiv_rn(__fsub_rn(y, a.g.lo[1]), a.g.cell[1]);
    const float qz = __fdiv_rn(__fsub_rn(z, a.g.lo[2]), a.g.cell[2]);
    // d = sqrt(x^2 + y^2 + z^2) + 1e-12 in float32, summed left to right
    // the float32 square root is taken in float64 and rounded once: correctly rounded like numpy's (v_sqrt_f32 is not)
    const float ss = __fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z));
    const float d = __fadd_rn((float)sqrt((double)ss), 1e-12f);
    const float phi_q = __fdiv_rn(__fsub_rn(a.g.phi_hi, atan2f(x, y)), a.g.dphi);
    const float th_q = __fdiv_rn(__fsub_rn(a.g.th_hi, asinf(__fdiv_rn(z, d))), a.g.dtheta);
    const int64_t s = (int64_t)v * a.T + a.t;
    float* f = a.xyzi + s * 7 * a.N + j;
    f[0] = x;
    f[a.N] = y;
    f[2 * a.N] = z;
    f[3 * a.N] = inten;
    f[4 * a.N] = d;
    f[5 * a.N] = __fsub_rn(qx, floorf(qx));
    f[6 * a.N] = __fsub_rn(qy, floorf(qy));
    float* c = a.coord + (s * a.N + j) * 3;
    c[0] = qx;
    c[1] = qy;
    c[2] = qz;
    float* sp = a.sphere + (s * a.N + j) * 2;
    sp[0] = th_q;
    sp[1] = phi_q;
  }
}

static void fill_geom(PrepGeom& g, const double* range6, const int64_t* bev_size3, const double* rv4) {
  // the reference keeps the cell sizes as Python doubles and numpy rounds them to float32 at use
  for (int d = 0; d < 3; ++d) {
    g.lo[d] = (float)range6[2 * d];
    g.hi[d] = (float)range6[2 * d + 1];
    g.cell[d] = (float)((range6[2 * d + 1] - range6[2 * d]) / (double)bev_size3[d]);
  }
  g.phi_hi = (float)rv4[0];
  g.dphi = (float)rv4[1];
  g.th_hi = (float)rv4[2];
  g.dtheta = (float)rv4[3];
}

}  // namespace smos
