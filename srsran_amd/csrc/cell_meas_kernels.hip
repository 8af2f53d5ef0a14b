// srsran_amd/csrc/cell_meas_kernels.hip -- neighbour-cell measurement (srslte_refsignal_dl_sync_*,
// lib/src/phy/sync/refsignal_dl_sync.c) for batches of (capture, cell) pairs.
//
//   cm_grid        workgroup per (cell, subframe): the zeroed resource grid with PSS / SSS (subframes 0 and 5) and the
//                  CRS of every port put (set_cell :229-255); ofdm_tx (ofdm_kernels.hip) modulates and scales it.
//   cm_corr        the hot path: workgroup per (group of <= CM_CELLS jobs on one capture, block, tile of CM_TILE lags).
//                  corr[i] = sum_k x[n + i + k] conj(seq0[k]), k < sf_len, in direct form: the samples of the tile
//                  and CM_KT taps of each cell's sequence are staged in LDS as double, each thread keeps CM_LPT lags x
//                  CM_CELLS cells of complex double accumulators, and the workgroup reduces them to max |c|^2, its
//                  lowest lag and sum |c|^2.  The correlation itself never reaches HBM.
//   cm_measure     workgroup per job: combines the partials (refsignal_sf_correlate's peak and rms per block, the
//                  strictly-greater peak update, rms_avg, the 4 rms threshold), runs the half-frame check (:339-353)
//                  and the per-subframe loop (:393-428), one wave per symbol correlation, and writes the per-subframe
//                  records for the host's decision.
//   cm_measure_sf  workgroup per (input, cell, sf_idx): srslte_refsignal_dl_sync_measure_sf alone.
//
// Every loop is bounded by the kernel's arguments; no workgroup waits for another.  Sums are formed in double in a
// fixed order and rounded to float once, so a job's result does not depend on what else is in the batch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "cell_meas_internal.h"
#include "lte_common.h"

namespace mi355 {

namespace {

constexpr uint32_t CM_WAVES = 4; // 256 threads

__device__ __forceinline__ double shfl_down_d(double v, uint32_t off) { return __shfl_down(v, off, 64); }

// ---------------------------------------------------------------------------- symbol correlations

// sum a[i] conj(b[i]) and sum |a[i]|^2 over n samples by one wave; every lane returns the totals
__device__ __forceinline__ float4 wave_dot(const float2* __restrict__ a, const float2* __restrict__ b, uint32_t n,
                                           uint32_t lane)
{
  double cr = 0, ci = 0, pw = 0;
  for (uint32_t i = lane; i < n; i += 64) {
    const float2 x = a[i], y = b[i];
    cr += (double)x.x * y.x + (double)x.y * y.y;
    ci += (double)x.y * y.x - (double)x.x * y.y;
    pw += (double)x.x * x.x + (double)x.y * x.y;
  }
  for (uint32_t off = 32; off; off >>= 1) {
    cr += __shfl_xor(cr, off, 64);
    ci += __shfl_xor(ci, off, 64);
    pw += __shfl_xor(pw, off, 64);
  }
  return make_float4((float)cr, (float)ci, (float)pw, 0.f);
}

struct CmGeom {
  uint32_t N, cp0, cp1, sf_len, nof_prb;
};

// FFT window of CRS symbol l of port 0 (measure_sf :538-543) and of the SSS (refsignal_dl_pss_sss_strength :119)
__device__ __forceinline__ uint32_t crs_offset(const CmGeom& g, uint32_t l)
{
  const uint32_t off = g.cp0 + (g.N + g.cp1) * crs_nsymbol(l, 7, 0);
  return l >= 2 ? off + g.cp0 - g.cp1 : off;
}
__device__ __forceinline__ uint32_t sss_offset(const CmGeom& g) { return g.cp0 + g.cp1 * 5 + g.N * 5; }

// One of the ten correlations of a subframe that starts at buf, by one wave:
//   slot 0-3  CRS symbol l against the sequence of sf_idx, with the symbol's power (measure_sf)
//   slot 4, 5 the SSS symbol against the sequences of sf_idx and sf_idx + 5 (sss_strength, sss_strength_false)
//   slot 6-9  CRS symbol l against the sequence of sf_false (the false RSRP)
// cell_seq: the cell's ten sequences.  Reads buf[0 .. sf_len).
__device__ __forceinline__ float4 cm_slot(const CmGeom& g, const float2* __restrict__ buf,
                                          const float2* __restrict__ cell_seq, uint32_t sf_idx, uint32_t sf_false,
                                          uint32_t slot, uint32_t lane)
{
  uint32_t off, sf;
  if (slot < 4) off = crs_offset(g, slot), sf = sf_idx % 10;
  else if (slot < 6) off = sss_offset(g), sf = (sf_idx + (slot == 5 ? 5u : 0u)) % 10;
  else off = crs_offset(g, slot - 6), sf = sf_false % 10;
  return wave_dot(buf + off, cell_seq + (size_t)sf * g.sf_len + off, g.N, lane);
}

__device__ __forceinline__ float pw2(float4 c) { return c.x * c.x + c.y * c.y; } // __real__(c * conjf(c))
// cargf(p * conjf(q)): the product is exact in double, so the angle is rounded once
__device__ __forceinline__ float carg_prod_conj(float4 p, float4 q)
{
  return (float)atan2((double)p.y * q.x - (double)p.x * q.y, (double)p.x * q.x + (double)p.y * q.y);
}

// measure_sf's outputs from the four symbol correlations r[0..3] (:548-591), operation by operation
__device__ void cm_finish_sf(const CmGeom& g, const float4* r, uint32_t sf_idx, bool full, mi355_cell_meas_sf_t* o)
{
  float rsrp_lin = 0.0f, rssi_lin = 0.0f;
  for (uint32_t l = 0; l < 4; l++) {
    rsrp_lin += pw2(r[l]);
    rssi_lin += r[l].z;
  }
  o->sf_idx = sf_idx;
  o->rsrp   = rsrp_lin * 4;
  o->rssi   = (float)g.nof_prb * rssi_lin / 4.0f * 7.41f;
  const float distance_1 = (g.cp1 + g.N) * 4.0f;
  const float distance_2 = (g.cp1 + g.N) * 3.0f + (g.cp0 - g.cp1);
  const float low_w = 0.5f / 2.0f, medium_w = 0.3f / 2.0f, high_w = 0.2f;
  float       cfo = 0;
  // (2.0f * M_PI is a double product in the reference, so each term is formed in double and added to the float)
  cfo = (float)(cfo + carg_prod_conj(r[2], r[0]) / (2.0f * M_PI * 7.5f) * 15000.0f * low_w);
  cfo = (float)(cfo + carg_prod_conj(r[3], r[1]) / (2.0f * M_PI * 7.5f) * 15000.0f * low_w);
  cfo = (float)(cfo + carg_prod_conj(r[1], r[0]) / (2.0f * M_PI * distance_1) * (15000.0f * g.N) * medium_w);
  cfo = (float)(cfo + carg_prod_conj(r[3], r[2]) / (2.0f * M_PI * distance_1) * (15000.0f * g.N) * medium_w);
  cfo = (float)(cfo + carg_prod_conj(r[2], r[1]) / (2.0f * M_PI * distance_2) * (15000.0f * g.N) * high_w);
  o->cfo = cfo;
  o->sss_strength = o->sss_strength_false = o->rsrp_false = 0.0f;
  if (full) {
    const float k = (float)(8 * g.nof_prb) / 62.0f; // srslte_refsignal_cs_nof_re(port 0) / SRSLTE_PSS_LEN
    o->sss_strength       = k * pw2(r[4]);
    o->sss_strength_false = k * pw2(r[5]);
    float f = 0.0f;
    for (uint32_t l = 0; l < 4; l++) f += pw2(r[6 + l]);
    o->rsrp_false = f * 4;
  }
}

} // namespace

// ---------------------------------------------------------------------------- sequences: the grid
__global__ __launch_bounds__(256) void cm_grid(CmGridArgs a)
{
  const uint32_t cell = blockIdx.y, sf = blockIdx.x;
  const uint32_t nre = 12 * a.nof_prb, nref = 2 * a.nof_prb;
  float2*        g   = a.grids + ((size_t)cell * 10 + sf) * 14 * nre;
  const CmCellDev c  = a.cells[cell];
  for (uint32_t i = threadIdx.x; i < 14 * nre; i += 256) g[i] = make_float2(0.f, 0.f);
  __syncthreads();
  if (sf % 5 == 0) { // srslte_pss_put_slot / srslte_sss_put_slot: last and second last symbol of slot 0
    const uint32_t k = nre / 2 - 31;
    for (uint32_t i = threadIdx.x; i < 62; i += 256) {
      g[6 * nre + k + i] = a.pss[(c.id % 3) * 62 + i];
      g[5 * nre + k + i] = make_float2(a.sss[((size_t)cell * 2 + (sf ? 1 : 0)) * 62 + i], 0.f);
    }
  }
  // srslte_refsignal_cs_put_sf for every port (the ports' positions are disjoint)
  for (uint32_t t = threadIdx.x; t < c.nof_ports * 4 * nref; t += 256) {
    const uint32_t p = t / (4 * nref), l = (t % (4 * nref)) / nref, i = t % nref;
    if (l >= (p < 2 ? 4u : 2u)) continue;
    const uint32_t s = crs_nsymbol(l, 7, p), f = crs_fidx(c.id, l, p);
    g[s * nre + f + 6 * i] = a.pilots[(((size_t)cell * 2 + p / 2) * 10 + sf) * 4 * nref + l * nref + i];
  }
}

// ---------------------------------------------------------------------------- stage 1: sliding correlation
__global__ __launch_bounds__(256) void cm_corr(CmArgs a)
{
  __shared__ double2  xs[CM_TILE + CM_KT];
  __shared__ double2  ss[CM_CELLS][CM_KT];
  __shared__ double   r_max[CM_CELLS][CM_WAVES], r_sum[CM_CELLS][CM_WAVES];
  __shared__ uint32_t r_arg[CM_CELLS][CM_WAVES];

  const CmGroup& G = a.groups[blockIdx.z];
  const uint32_t b = blockIdx.y;
  if (b >= G.nblocks) return;
  const uint32_t t = threadIdx.x, L = a.sf_len, tile0 = blockIdx.x * CM_TILE;
  const float2*  in   = (const float2*)G.in;
  const size_t   base = (size_t)b * L + tile0; // sample under lag tile0, tap 0

  double2 acc[CM_LPT][CM_CELLS];
#pragma unroll
  for (uint32_t j = 0; j < CM_LPT; j++)
#pragma unroll
    for (uint32_t c = 0; c < CM_CELLS; c++) acc[j][c] = make_double2(0.0, 0.0);

  for (uint32_t k0 = 0; k0 < L; k0 += CM_KT) {
    __syncthreads();
    for (uint32_t i = t; i < CM_TILE + CM_KT; i += 256) {
      const size_t idx = base + k0 + i;
      const float2 v   = idx < G.nsamples ? in[idx] : make_float2(0.f, 0.f); // lags past sf_len only; masked below
      xs[i]            = make_double2((double)v.x, (double)v.y);
    }
    for (uint32_t i = t; i < CM_CELLS * CM_KT; i += 256) {
      const uint32_t c = i / CM_KT, k = i % CM_KT;
      float2         v = make_float2(0.f, 0.f);
      if (c < G.ncell && k0 + k < L) v = a.seq[(size_t)G.cell[c] * 10 * L + k0 + k]; // subframe 0's sequence
      ss[c][k] = make_double2((double)v.x, -(double)v.y);
    }
    __syncthreads();
#pragma unroll 2
    for (uint32_t k = 0; k < CM_KT; k++) {
      double2 s[CM_CELLS], x[CM_LPT];
#pragma unroll
      for (uint32_t c = 0; c < CM_CELLS; c++) s[c] = ss[c][k];
#pragma unroll
      for (uint32_t j = 0; j < CM_LPT; j++) x[j] = xs[t + 256 * j + k];
#pragma unroll
      for (uint32_t j = 0; j < CM_LPT; j++)
#pragma unroll
        for (uint32_t c = 0; c < CM_CELLS; c++) {
          acc[j][c].x = fma(x[j].x, s[c].x, acc[j][c].x);
          acc[j][c].x = fma(-x[j].y, s[c].y, acc[j][c].x);
          acc[j][c].y = fma(x[j].x, s[c].y, acc[j][c].y);
          acc[j][c].y = fma(x[j].y, s[c].x, acc[j][c].y);
        }
    }
  }

  const uint32_t lane = t % 64, wave = t / 64;
#pragma unroll
  for (uint32_t c = 0; c < CM_CELLS; c++) {
    double   m = -1.0, sum = 0.0;
    uint32_t arg = 0;
#pragma unroll
    for (uint32_t j = 0; j < CM_LPT; j++) {
      const uint32_t lag = tile0 + t + 256 * j;
      if (lag < L) {
        const double p = acc[j][c].x * acc[j][c].x + acc[j][c].y * acc[j][c].y;
        sum += p;
        if (p > m) m = p, arg = lag;
      }
    }
    for (uint32_t off = 32; off; off >>= 1) {
      const double   m2 = shfl_down_d(m, off);
      const uint32_t a2 = __shfl_down(arg, off, 64);
      sum += shfl_down_d(sum, off);
      if (m2 > m || (m2 == m && a2 < arg)) m = m2, arg = a2;
    }
    if (lane == 0) r_max[c][wave] = m, r_sum[c][wave] = sum, r_arg[c][wave] = arg;
  }
  __syncthreads();
  if (t < G.ncell) {
    double   m = r_max[t][0], sum = r_sum[t][0];
    uint32_t arg = r_arg[t][0];
    for (uint32_t w = 1; w < CM_WAVES; w++) {
      sum += r_sum[t][w];
      if (r_max[t][w] > m || (r_max[t][w] == m && r_arg[t][w] < arg)) m = r_max[t][w], arg = r_arg[t][w];
    }
    CmPartial& P = a.part[((size_t)G.job[t] * CM_MAX_BLOCKS + b) * a.ntiles + blockIdx.x];
    P.pmax = m, P.psum = sum, P.arg = arg, P.pad = 0;
  }
}

// ---------------------------------------------------------------------------- stages 1b and 2
__global__ __launch_bounds__(256) void cm_measure(CmArgs a)
{
  __shared__ float4   raw[CM_SF_LDS][10];
  __shared__ float    bpeak[CM_MAX_BLOCKS], brms[CM_MAX_BLOCKS];
  __shared__ uint32_t barg[CM_MAX_BLOCKS];
  __shared__ int32_t  s_peak;

  const uint32_t job = blockIdx.x, t = threadIdx.x, lane = t % 64, wave = t / 64;
  const CmJobDev J   = a.jobs[job];
  const CmGeom   g{a.N, a.cp0, a.cp1, a.sf_len, a.nof_prb};
  const uint32_t L = a.sf_len, ns = J.nsamples;
  const uint32_t lim = cm_limited(ns, L), nblocks = cm_nblocks(ns, L);
  const float2*  cell_seq = a.seq + (size_t)J.cell * 10 * L;

  // refsignal_sf_correlate per block: the peak and the rms of its sf_len lags
  if (t < nblocks) {
    const CmPartial* P = a.part + ((size_t)job * CM_MAX_BLOCKS + t) * a.ntiles;
    double           m = P[0].pmax, sum = P[0].psum;
    uint32_t         arg = P[0].arg;
    for (uint32_t i = 1; i < a.ntiles; i++) {
      sum += P[i].psum;
      if (P[i].pmax > m) m = P[i].pmax, arg = P[i].arg; // tiles in ascending lag: the lowest lag wins a tie
    }
    bpeak[t] = (float)sqrt(m);
    brms[t]  = (float)sqrt(sum / (double)L);
    barg[t]  = arg;
  }
  __syncthreads();
  if (t == 0) { // find_peak :316-336
    float    peak_value = 0.0f, rms_avg = 0;
    uint32_t peak_idx = 0;
    for (uint32_t b = 0; b < nblocks; b++) {
      rms_avg += brms[b];
      if (bpeak[b] > peak_value) peak_value = bpeak[b], peak_idx = barg[b] + b * L;
    }
    rms_avg /= floorf((float)lim / L);
    const bool found = peak_value > rms_avg * 4.0f;
    CmHead&    H     = a.head[job];
    H.peak_value = peak_value, H.rms_avg = rms_avg;
    H.stage1_peak = peak_idx, H.stage1_found = found, H.peak_shifted = 0;
    H.sf_count = 0, H.pad = 0;
    s_peak = found ? (int32_t)peak_idx : -1;
  }
  __syncthreads();
  int32_t peak = s_peak;
  if (peak > 0) { // the half-frame check (:339-353) at the peak as subframe 0: it reads in[peak .. peak + sf_len)
    for (uint32_t slot = wave; slot < 10; slot += CM_WAVES) {
      const float4 r = cm_slot(g, J.in + peak, cell_seq, 0, 5, slot, lane);
      if (lane == 0) raw[0][slot] = r;
    }
    __syncthreads();
    if (t == 0) {
      mi355_cell_meas_sf_t o;
      cm_finish_sf(g, raw[0], 0, true, &o);
      if (o.sss_strength_false > o.sss_strength && o.rsrp_false > o.rsrp) {
        s_peak               = peak + (int32_t)(5 * L);
        a.head[job].peak_shifted = 1;
      }
    }
    __syncthreads();
    peak = s_peak;
    __syncthreads(); // raw[0] is reused below
  }
  if (t == 0) a.head[job].peak_idx = peak;
  if (peak < 0 || !a.stage2) return;

  // stage 2 (:390-428): subframes from n_init on while a whole one is left
  const uint32_t sf_init = (20 - (uint32_t)peak / L) % 10, n_init = (uint32_t)peak % L;
  uint32_t       count   = n_init + L <= ns ? (ns - L - n_init) / L + 1 : 0;
  if (count > a.max_nof_sf) count = a.max_nof_sf;
  for (uint32_t c0 = 0; c0 < count; c0 += CM_SF_LDS) {
    const uint32_t nc = count - c0 < CM_SF_LDS ? count - c0 : CM_SF_LDS;
    for (uint32_t task = wave; task < nc * 10; task += CM_WAVES) {
      const uint32_t i = task / 10, slot = task % 10, sf_idx = (sf_init + c0 + i) % 10;
      if (slot >= 4 && sf_idx % 5) continue;
      const float4 r = cm_slot(g, J.in + n_init + (size_t)(c0 + i) * L, cell_seq, sf_idx, sf_idx + 1, slot, lane);
      if (lane == 0) raw[i][slot] = r;
    }
    __syncthreads();
    if (t < nc) {
      const uint32_t sf_idx = (sf_init + c0 + t) % 10;
      cm_finish_sf(g, raw[t], sf_idx, sf_idx % 5 == 0, &a.sf[(size_t)job * a.max_nof_sf + c0 + t]);
    }
    __syncthreads();
  }
  if (t == 0) a.head[job].sf_count = count;
}

__global__ __launch_bounds__(256) void cm_measure_sf(CmArgs a, const CmSfJobDev* __restrict__ jobs,
                                                     mi355_cell_meas_sf_t* __restrict__ out)
{
  __shared__ float4 raw[4];
  const CmSfJobDev J = jobs[blockIdx.x];
  const CmGeom     g{a.N, a.cp0, a.cp1, a.sf_len, a.nof_prb};
  const uint32_t   lane = threadIdx.x % 64, wave = threadIdx.x / 64;
  const float4 r = cm_slot(g, J.in, a.seq + (size_t)J.cell * 10 * a.sf_len, J.sf_idx, 0, wave, lane);
  if (lane == 0) raw[wave] = r;
  __syncthreads();
  if (threadIdx.x == 0) cm_finish_sf(g, raw, J.sf_idx, false, &out[blockIdx.x]);
}

// ---------------------------------------------------------------------------- launches
hipError_t cm_launch_grid(const CmGridArgs& a, hipStream_t s)
{
  if (!a.n) return hipSuccess;
  hipLaunchKernelGGL(cm_grid, dim3(10, a.n), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t cm_launch_corr(const CmArgs& a, hipStream_t s)
{
  for (uint32_t g0 = 0; g0 < a.ngroups; g0 += 65535) { // grid.z limit
    CmArgs b  = a;
    b.groups  = a.groups + g0;
    b.ngroups = a.ngroups - g0 < 65535 ? a.ngroups - g0 : 65535;
    hipLaunchKernelGGL(cm_corr, dim3(a.ntiles, a.max_blocks, b.ngroups), dim3(256), 0, s, b);
  }
  return hipGetLastError();
}

hipError_t cm_launch_measure(const CmArgs& a, hipStream_t s)
{
  if (!a.njobs) return hipSuccess;
  hipLaunchKernelGGL(cm_measure, dim3(a.njobs), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t cm_launch_measure_sf(const CmArgs& a, const CmSfJobDev* jobs, uint32_t n, mi355_cell_meas_sf_t* out,
                                hipStream_t s)
{
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(cm_measure_sf, dim3(n), dim3(256), 0, s, a, jobs, out);
  return hipGetLastError();
}

} // namespace mi355
