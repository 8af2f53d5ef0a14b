// srsran_amd/csrc/pbch_kernels.hip -- PBCH (MIB) decoding on gfx950.
//
//   pbch_llr       one workgroup per (radio frame, port hypothesis): the 240 PBCH REs of the grid and of each port's
//                  estimate (srslte_pbch_get order, index table in HBM) equalised for a single port / transmit
//                  diversity and QPSK-demapped into 480 float LLRs (pbch.c:501-515).
//   pbch_decode    one wave per (radio frame, port hypothesis of that frame, window of n consecutive frames ending at
//                  it, 40 ms phase dst): decode_frame (pbch.c:399-434) -- the window's LLRs descrambled at offset
//                  480 dst into a 1920-entry vector in LDS, SRSLTE_RX_NULL elsewhere, then the rate dematcher, the
//                  1 / (2 n) scale, the quantiser, the tail-biting Viterbi decoder and the CRC16 of conv_decode.h
//                  for F = 40 -> the decided bits and the unmasked CRC remainder the host replay compares with each
//                  port mask.  Older frames of a window are read under the last hypothesis tried in their call: the
//                  reference's history slot holds what the last hypothesis wrote (pbch.c:515).
//   pbch_save_hist the last three frames' LLRs under the last hypothesis -> the object's history.
//
// Built with -ffp-contract=off: the equalisers (ctrl_eq.h) evaluate the reference's formulas operation by operation.
#include <hip/hip_runtime.h>

#include "conv_decode.h"
#include "ctrl_eq.h"
#include "pbch_internal.h"

namespace mi355 {

namespace {

__global__ __launch_bounds__(256) void pbch_llr(PbchArgs a)
{
  const uint32_t job = blockIdx.x / a.nhyp, h = blockIdx.x % a.nhyp, nant = a.ports[h], t = threadIdx.x;
  const PbchJob& P   = a.jobs[job];
  // the control-channel equalisers' view of this frame: one receive antenna, an estimate per grid RE
  CtrlArgs c{};
  c.nof_rx = 1;
  c.ce_row = 0;
  CtrlJob J{};
  J.grid[0] = P.grid;
  for (uint32_t p = 0; p < MI355_MAX_PORTS; p++) J.ce[p][0] = P.ce[p];
  float* out = a.llr + (size_t)blockIdx.x * PBCH_NBITS;
  if (nant == 1) {
    if (t < PBCH_NRE) reinterpret_cast<float2*>(out)[t] = demod(eq_single(c, J, a.re[t], P.noise), 0u, 0u);
  } else if (nant == 2) {
    // 240 symbols: srslte_predecoding_diversity takes its SSE form for all of them (n > 32, n % 4 == 0)
    if (t < PBCH_NRE / 2) {
      float2 d0, d1;
      eq_pair(c, J, a.re[2 * t], a.re[2 * t + 1], true, d0, d1);
      const float2 l0 = demod(d0, 0u, 0u), l1 = demod(d1, 0u, 0u);
      reinterpret_cast<float4*>(out)[t] = make_float4(l0.x, l0.y, l1.x, l1.y);
    }
  } else {
    if (t < PBCH_NRE / 4) {
      float2 d[4];
      eq_quad(c, J, a.re + 4 * t, d);
      for (int q = 0; q < 4; q++) reinterpret_cast<float2*>(out)[4 * t + q] = demod(d[q], 0u, 0u);
    }
  }
}

__global__ __launch_bounds__(64) void pbch_decode(PbchArgs a)
{
  __shared__ WaveLds lds;
  __shared__ float   s_vec[4 * PBCH_NBITS];
  __shared__ DciCand s_out; // decode_cand's record; the PBCH keeps w0 and the remainder only
  const uint32_t lane = threadIdx.x;
  const uint32_t job = blockIdx.x / (a.nhyp * PBCH_WIN), h = (blockIdx.x / PBCH_WIN) % a.nhyp, w = blockIdx.x % PBCH_WIN;
  const uint32_t n = w < 4 ? 1u : w < 7 ? 2u : w < 9 ? 3u : 4u, dst = w - pbch_win(n, 0);
  PbchRec*       rec = a.rec + blockIdx.x;
  if (n - 1 > a.jobs[job].navail) { // the window reaches past the frames received since the last reset
    if (lane == 0) *rec = PbchRec{0u, PBCH_REC_NONE};
    return;
  }
  for (uint32_t j = lane; j < 4 * PBCH_NBITS; j += 64) {
    const uint32_t q = j / PBCH_NBITS, k = j % PBCH_NBITS;
    float          v = RX_NULL;
    if (q >= dst && q < dst + n) {
      const uint32_t back = n - 1 - (q - dst); // 0: the newest frame, under this wave's hypothesis
      const int      fr   = (int)job - (int)back;
      const float    x    = back == 0 ? a.llr[((size_t)job * a.nhyp + h) * PBCH_NBITS + k]
                            : fr >= 0 ? a.llr[((size_t)fr * a.nhyp + (a.nhyp - 1)) * PBCH_NBITS + k]
                                      : a.hist[(size_t)((int)PBCH_HIST + fr) * PBCH_NBITS + k];
      v                   = x * (((a.seq[j >> 5] >> (j & 31)) & 1u) ? -1.f : 1.f); // srslte_scrambling_f_offset
    }
    s_vec[j] = v;
  }
  __syncthreads();
  // 1.0 / ((float)2 * n) passed as a float (pbch.c:420)
  const float scale = n == 1 ? 0.5f : n == 2 ? 0.25f : n == 3 ? (float)(1.0 / 6.0) : 0.125f;
  uint32_t    w0;
  const uint32_t rem = decode_cand<true>(lds, s_vec, 4 * PBCH_NBITS, MI355_BCH_PAYLOAD_LEN, 0, 0, &s_out, w0, scale);
  if (lane == 0) *rec = PbchRec{w0, rem};
}

__global__ __launch_bounds__(256) void pbch_save_hist(const float* llr, float* hist, uint32_t njobs, uint32_t nhyp)
{
  constexpr uint32_t TOT = PBCH_HIST * PBCH_NBITS, PER = (TOT + 255) / 256;
  float              v[PER];
  // every source is read before any destination is written: with fewer than three new frames the history moves up
  // in place
#pragma unroll
  for (uint32_t u = 0; u < PER; u++) {
    const uint32_t i = threadIdx.x + 256 * u;
    v[u]             = 0.f;
    if (i < TOT) {
      const uint32_t s = i / PBCH_NBITS, k = i % PBCH_NBITS;
      const int      f = (int)njobs - (int)PBCH_HIST + (int)s; // frame of this call that lands in slot s
      v[u] = f >= 0 ? llr[((size_t)f * nhyp + (nhyp - 1)) * PBCH_NBITS + k] : hist[(size_t)(s + njobs) * PBCH_NBITS + k];
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t u = 0; u < PER; u++) {
    const uint32_t i = threadIdx.x + 256 * u;
    if (i < TOT) hist[i] = v[u];
  }
}

} // namespace

hipError_t pbch_launch_llr(const PbchArgs& a, uint32_t njobs, hipStream_t s)
{
  if (!njobs) return hipSuccess;
  hipLaunchKernelGGL(pbch_llr, dim3(njobs * a.nhyp), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t pbch_launch_decode(const PbchArgs& a, uint32_t njobs, hipStream_t s)
{
  if (!njobs) return hipSuccess;
  hipLaunchKernelGGL(pbch_decode, dim3(njobs * a.nhyp * PBCH_WIN), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t pbch_launch_save_hist(const PbchArgs& a, float* hist, uint32_t njobs, hipStream_t s)
{
  if (!njobs) return hipSuccess;
  hipLaunchKernelGGL(pbch_save_hist, dim3(1), dim3(256), 0, s, (const float*)a.llr, hist, njobs, a.nhyp);
  return hipGetLastError();
}

} // namespace mi355
