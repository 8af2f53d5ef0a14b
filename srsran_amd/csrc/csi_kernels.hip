// srsran_amd/csrc/csi_kernels.hip -- the UE's channel-state feedback on gfx950: the sums behind the PMI / RI selection
// (srslte_precoding_pmi_select, precoding.c:2363-2478 and :2609-2759) and the condition number (srslte_precoding_cn,
// precoding.c:2813-2854 over srslte_mat_2x2_cn, mat.c:127-159) of 2x2 channel estimates.
//
//   csi_feedback  one wave per subframe, four subframes per workgroup.  Lane l takes the samples m = l, l + 64, ...
//                 (estimate 24 m of each of the four grids, loaded once as float2) and feeds eight accumulators from
//                 each: the four 1-layer SINRs, the two 2-layer SINRs, the condition number and its sample count.  The
//                 SINR accumulators take the samples m < 8 G only (the reference's AVX2 loop stops at whole groups of
//                 eight); the rest of the grid enters the condition number alone.  The lanes' partial sums meet in a
//                 fixed xor-shuffle tree, so a result repeats bit for bit, and lane 0 writes the 32-byte record.
//                 No LDS, no atomics.
//
// A strided gather and a few dozen flops per sample: nothing here is GEMM-shaped.  Each 8-byte load touches a cache
// line of its own (192-byte stride), 4 lines per sample.  The formulas are the reference's, operation by operation and
// without FMA contraction (built with -ffp-contract=off); where the reference approximates 1 / x with _mm256_rcp_ps the
// division here is exact, and the sums are taken in this kernel's order, not in the reference's (csi.h: tolerances).
#include <hip/hip_runtime.h>

#include "csi_internal.h"

namespace mi355 {

namespace {

constexpr uint32_t CSI_BLOCK = 256; // four waves: four subframes

__device__ inline float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ inline float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ inline float2 cconj(float2 a) { return make_float2(a.x, -a.y); }
__device__ inline float2 cmulj(float2 a) { return make_float2(-a.y, a.x); }
// srslte_simd_cf_prod without LV_HAVE_FMA
__device__ inline float2 cprod(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ inline float2 cscale(float2 a, float s) { return make_float2(a.x * s, a.y * s); }

// gamma0 + gamma1 of one sample for C = (c00 c01; c10 c11) (precoding.c:2692-2718): C / 4 + noise I, the real part of
// the determinant kept above 1e-10, gamma_k = 1 / (noise c_kk / det) - 1 kept above 1e-9 (a NaN passes both selects)
__device__ inline float gamma_2l(float2 c00, float2 c01, float2 c10, float2 c11, float noise)
{
  c00 = cscale(c00, 0.25f), c01 = cscale(c01, 0.25f), c10 = cscale(c10, 0.25f), c11 = cscale(c11, 0.25f);
  c00 = cadd(c00, make_float2(noise, 0.f));
  c11 = cadd(c11, make_float2(noise, 0.f));
  float det = cprod(c00, c11).x - cprod(c01, c10).x;
  if (det < 1e-10f) det = 1e-10f;
  const float inv = noise * (1.0f / det);
  float       g0 = 1.0f / (c00.x * inv) - 1.0f, g1 = 1.0f / (c11.x * inv) - 1.0f;
  if (g0 < 1e-9f) g0 = 1e-9f;
  if (g1 < 1e-9f) g1 = 1e-9f;
  return g0 + g1;
}

__global__ __launch_bounds__(CSI_BLOCK) void csi_feedback(CsiArgs a)
{
  const uint32_t lane = threadIdx.x % 64;
  const uint32_t job  = blockIdx.x * (CSI_BLOCK / 64) + threadIdx.x / 64;
  if (job >= a.nsf) return; // the whole wave leaves: the shuffles below stay inside one wave
  const CsiJob   J     = a.jobs[job];
  const float    noise = J.noise;
  const uint32_t n_pmi = CSI_SIMD * a.groups;
  float          acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; // sinr_1l[4] | sinr_2l[2] | cn | cn count
  for (uint32_t m = lane; m < a.n_cn; m += 64) {
    uint32_t j = CSI_STEP * m;
    if (a.ce_row) j %= a.ce_row;
    // h[tx port][rx antenna] -> the reference's h00 = h[0][0], h01 = h[1][0], h10 = h[0][1], h11 = h[1][1]
    const float2 h00 = J.ce[0][0][j], h01 = J.ce[1][0][j], h10 = J.ce[0][1][j], h11 = J.ce[1][1][j];
    if (m < n_pmi) {
      // A = W' H' per 1-layer codebook index i (w_i = (1, {1, -1, j, -j}_i)): a0 = h00* +- h01*, h00* -+ j h01*
      const float2 q00 = cconj(h00), q01 = cconj(h01), q10 = cconj(h10), q11 = cconj(h11);
      const float2 a0[4] = {cadd(q00, q01), csub(q00, q01), csub(q00, cmulj(q01)), cadd(q00, cmulj(q01))};
      const float2 a1[4] = {cadd(q10, q11), csub(q10, q11), csub(q10, cmulj(q11)), cadd(q10, cmulj(q11))};
      float2       b0[4], b1[4];
      for (int i = 0; i < 4; i++) {
        // B = A H
        b0[i] = cadd(cprod(a0[i], h00), cprod(a1[i], h10));
        b1[i] = cadd(cprod(a0[i], h01), cprod(a1[i], h11));
      }
      // 1 layer: Re(B w_i) / 2 (precoding.c:2423-2440)
      acc[0] += cadd(b0[0], b1[0]).x * 0.5f;
      acc[1] += csub(b0[1], b1[1]).x * 0.5f;
      acc[2] += cadd(b0[2], cmulj(b1[2])).x * 0.5f;
      acc[3] += csub(b0[3], cmulj(b1[3])).x * 0.5f;
      // 2 layers: the rows of W' H' H for codebook 0 are the 1-layer rows 0 and 1, for codebook 1 the rows 2 and 3
      // (precoding.c:2651-2691)
      acc[4] += gamma_2l(cadd(b0[0], b1[0]), csub(b0[0], b1[0]), cadd(b0[1], b1[1]), csub(b0[1], b1[1]), noise);
      acc[5] += gamma_2l(cadd(b0[2], cmulj(b1[2])), csub(b0[2], cmulj(b1[2])), cadd(b0[3], cmulj(b1[3])),
                         csub(b0[3], cmulj(b1[3])), noise);
    }
    // srslte_mat_2x2_cn: the eigenvalues of H H' from its trace and determinant
    const float  a00 = h00.x * h00.x + h01.x * h01.x + h00.y * h00.y + h01.y * h01.y;
    const float2 a01 = cadd(cprod(h00, cconj(h10)), cprod(h01, cconj(h11)));
    const float  a11 = h10.x * h10.x + h11.x * h11.x + h10.y * h10.y + h11.y * h11.y;
    const float  b = a00 + a11, c = a00 * a11 - (a01.x * a01.x + a01.y * a01.y);
    const float  sqr = sqrtf(b * b - 4.0f * c);
    float        xmax = b + sqr, xmin = b - sqr;
    if (!(isnan(xmin) || isinf(xmin) || isnan(xmax) || isinf(xmax))) {
      xmin = xmin > 1e-9f ? xmin : 1e-9f;
      xmax = xmax < 1e+9f ? xmax : 1e+9f;
      acc[6] += 10.0f * log10f(xmax / xmin);
      acc[7] += 1.0f; // at most 700 per subframe: exact in float
    }
  }
  for (int k = 0; k < 8; k++)
    for (int d = 32; d >= 1; d >>= 1) acc[k] += __shfl_xor(acc[k], d);
  if (lane == 0) {
    // precoding.c:2452-2463, 2732-2743: every group's sum over 8, then the mean over the groups (and the noise)
    const float G = (float)a.groups;
    CsiOut      o;
    for (int i = 0; i < 4; i++) o.sinr_1l[i] = a.groups ? (acc[i] / (float)CSI_SIMD) / (noise * G) : 1e+9f;
    for (int i = 0; i < 2; i++) o.sinr_2l[i] = a.groups ? (acc[4 + i] / (float)CSI_SIMD) / G : 1e+9f;
    o.cn_count = (uint32_t)acc[7];
    o.cn       = o.cn_count ? acc[6] / (float)o.cn_count : 0.f;
    a.out[job] = o;
  }
}

} // namespace

hipError_t csi_launch(const CsiArgs& a, hipStream_t s)
{
  if (!a.nsf) return hipSuccess;
  const uint32_t per = CSI_BLOCK / 64, blocks = (a.nsf + per - 1) / per;
  hipLaunchKernelGGL(csi_feedback, dim3(blocks), dim3(CSI_BLOCK), 0, s, a);
  return hipGetLastError();
}

} // namespace mi355
