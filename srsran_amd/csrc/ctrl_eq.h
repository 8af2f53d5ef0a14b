// srsran_amd/csrc/ctrl_eq.h -- the control-channel equalisers and the QPSK demapper as device functions, shared by
// the PCFICH / PDCCH kernels (pdcch_kernels.hip) and the PBCH kernels (pbch_kernels.hip).  They evaluate the
// reference's formulas operation by operation: every file that includes this is built with -ffp-contract=off, so
// the results equal oracle/orc_pdcch.c (orc_ctrl_equalize) bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include "pdcch_internal.h"

namespace mi355 {

namespace {

__device__ __forceinline__ float2 ld(const float2* p, uint32_t i) { return p[i]; }
// an estimate at grid index re: row 0 when the estimates are time-invariant (CtrlArgs::ce_row)
__device__ __forceinline__ float2 ldh(const CtrlArgs& a, const float2* p, uint32_t re) { return p[a.ce_row ? re % a.ce_row : re]; }

// 1 port: x = sum_r y_r conj(h_r) / (sum_r |h_r|^2 + noise)
__device__ __forceinline__ float2 eq_single(const CtrlArgs& a, const CtrlJob& J, uint32_t re, float noise)
{
  float rr = 0.f, ri = 0.f, hh = 0.f;
  for (uint32_t r = 0; r < a.nof_rx; r++) {
    const float2 y = ld(J.grid[r], re), h = ldh(a, J.ce[0][r], re);
    rr += y.x * h.x + y.y * h.y;
    ri += y.y * h.x - y.x * h.y;
    hh += h.x * h.x + h.y * h.y;
  }
  hh += noise;
  return make_float2(rr / hh, ri / hh);
}

// 2 ports, one SFBC pair (symbols 2i, 2i+1 at REs re0, re1); sse: the diversity2_sse form, else diversity_gen_
__device__ __forceinline__ void eq_pair(const CtrlArgs& a, const CtrlJob& J, uint32_t re0, uint32_t re1, bool sse,
                                        float2& d0, float2& d1)
{
  float x0r = 0.f, x0i = 0.f, x1r = 0.f, x1i = 0.f, hh = 0.f;
  for (uint32_t p = 0; p < a.nof_rx; p++) {
    const float2 h00 = ldh(a, J.ce[0][p], re0), h01 = ldh(a, J.ce[0][p], re1), h10 = ldh(a, J.ce[1][p], re0),
                 h11 = ldh(a, J.ce[1][p], re1);
    const float2 r0 = ld(J.grid[p], re0), r1 = ld(J.grid[p], re1);
    const float a0r = h00.x * r0.x + h00.y * r0.y, a0i = h00.x * r0.y - h00.y * r0.x;
    const float b0r = h11.x * r1.x + h11.y * r1.y, b0i = h11.y * r1.x - h11.x * r1.y;
    const float a1r = h01.x * r1.x + h01.y * r1.y, a1i = h01.x * r1.y - h01.y * r1.x;
    const float b1r = h10.x * r0.x + h10.y * r0.y, b1i = h10.y * r0.x - h10.x * r0.y;
    x0r += a0r + b0r;
    x0i += a0i + b0i;
    if (sse) {
      x1r += a1r - b1r;
      x1i += a1i - b1i;
      hh += (h00.x * h00.x + h00.y * h00.y) + (h11.x * h11.x + h11.y * h11.y);
    } else {
      x1r += -b1r + a1r;
      x1i += -b1i + a1i;
      hh += ((h00.x * h00.x + h00.y * h00.y) + h11.x * h11.x) + h11.y * h11.y;
      if (hh == 0.f) hh = 1e-4f;
    }
  }
  if (sse) {
    const float s2 = 1.41421354f; // (float)M_SQRT2
    d0 = make_float2((x0r / hh) * s2, (x0i / hh) * s2);
    d1 = make_float2((x1r / hh) * s2, (x1i / hh) * s2);
  } else {
    const double s2 = 1.4142135623730951;
    d0 = make_float2((float)((double)(x0r / hh) * s2), (float)((double)(x0i / hh) * s2));
    d1 = make_float2((float)((double)(x1r / hh) * s2), (float)((double)(x1i / hh) * s2));
  }
}

// 4 ports, one group of 4 symbols at REs re[0..3] (diversity_gen_ 4-port branch)
__device__ __forceinline__ void eq_quad(const CtrlArgs& a, const CtrlJob& J, const uint32_t* re, float2* d)
{
  float hh02 = 0.f, hh13 = 0.f, x[4][2] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
  for (uint32_t p = 0; p < a.nof_rx; p++) {
    const float2 h0 = ldh(a, J.ce[0][p], re[0]), h1 = ldh(a, J.ce[1][p], re[2]), h2 = ldh(a, J.ce[2][p], re[0]),
                 h3 = ldh(a, J.ce[3][p], re[2]);
    hh02 += (h0.x * h0.x + h0.y * h0.y) + (h2.x * h2.x + h2.y * h2.y);
    hh13 += (h1.x * h1.x + h1.y * h1.y) + (h3.x * h3.x + h3.y * h3.y);
    const float2 r0 = ld(J.grid[p], re[0]), r1 = ld(J.grid[p], re[1]), r2 = ld(J.grid[p], re[2]),
                 r3 = ld(J.grid[p], re[3]);
    x[0][0] += (h0.x * r0.x + h0.y * r0.y) + (h2.x * r1.x + h2.y * r1.y);
    x[0][1] += (h0.x * r0.y - h0.y * r0.x) + (h2.y * r1.x - h2.x * r1.y);
    x[1][0] += -(h2.x * r0.x + h2.y * r0.y) + (h0.x * r1.x + h0.y * r1.y);
    x[1][1] += -(h2.y * r0.x - h2.x * r0.y) + (h0.x * r1.y - h0.y * r1.x);
    x[2][0] += (h1.x * r2.x + h1.y * r2.y) + (h3.x * r3.x + h3.y * r3.y);
    x[2][1] += (h1.x * r2.y - h1.y * r2.x) + (h3.y * r3.x - h3.x * r3.y);
    x[3][0] += -(h3.x * r2.x + h3.y * r2.y) + (h1.x * r3.x + h1.y * r3.y);
    x[3][1] += -(h3.y * r2.x - h3.x * r2.y) + (h1.x * r3.y - h1.y * r3.x);
  }
  const double s2 = 1.4142135623730951;
  for (int q = 0; q < 4; q++) {
    const float g = q < 2 ? hh02 : hh13;
    d[q]          = make_float2((float)((double)(x[q][0] / g) * s2), (float)((double)(x[q][1] / g) * s2));
  }
}

// QPSK soft bits: symbol * (float)(-sqrt2), then the +-1 scrambling sequence
__device__ __forceinline__ float2 demod(float2 d, uint32_t c0, uint32_t c1)
{
  const float g = -1.41421354f;
  return make_float2(d.x * g * (c0 ? -1.f : 1.f), d.y * g * (c1 ? -1.f : 1.f));
}

} // namespace

} // namespace mi355
