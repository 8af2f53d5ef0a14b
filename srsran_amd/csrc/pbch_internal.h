// srsran_amd/csrc/pbch_internal.h -- descriptors shared by the PBCH kernels (pbch_kernels.hip) and their host
// runtime (pbch_runtime.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/srsran_amd/pbch.h"

namespace mi355 {

constexpr uint32_t PBCH_NRE   = MI355_PBCH_NOF_RE; // REs per radio frame
constexpr uint32_t PBCH_NBITS = 2 * PBCH_NRE;      // 480 LLRs per radio frame, 4 x 480 = the 1920 rate-matched bits
constexpr uint32_t PBCH_HYPS  = 3;                 // port hypotheses 1, 2, 4
constexpr uint32_t PBCH_HIST  = 3;                 // older radio frames the decoder can combine with the newest
// windows of n consecutive frames ending at the newest, placed at 40 ms phase dst: (n, dst) with dst + n <= 4
constexpr uint32_t PBCH_WIN   = 10;
constexpr uint32_t pbch_win(uint32_t n, uint32_t dst) { return (n == 1 ? 0u : n == 2 ? 4u : n == 3 ? 7u : 9u) + dst; }

// srslte_pbch_get / srslte_pbch_put's RE order (pbch.c:54-102 over prb_cp_ref / prb_cp, prb_dl.c:46-85) as grid
// indices: slot 1, symbols 0 .. 3, the 72 central subcarriers from nof_prb * 6 - 36; symbols 0 and 1 skip
// k % 3 == cell.id % 3, the CRS positions of four ports.  (prb_cp_ref leaves its grid pointer one RE short of 72 when
// the row's last RE is a skipped one, cell.id % 3 == 2: that is the reference's extra pointer step after those symbols.)
inline std::vector<uint32_t> pbch_re(const mi355_cell_t& c)
{
  std::vector<uint32_t> re;
  const uint32_t        nre = 12 * c.nof_prb, k0 = c.nof_prb * 6 - 36;
  for (uint32_t l = 0; l < 4; l++)
    for (uint32_t k = 0; k < 72; k++)
      if (l >= 2 || k % 3 != c.id % 3) re.push_back((7 + l) * nre + k0 + k);
  return re;
}

// One radio frame's subframe 0 (device pointers, receive antenna 0)
struct PbchJob {
  const float2* grid;
  const float2* ce[MI355_MAX_PORTS];
  float         noise;
  uint32_t      navail; // older frames in front of this one that a window may reach back to (0 .. PBCH_HIST)
};

// One decode: the 40 decided bits and the CRC remainder before any port mask.  w0: bits 0 .. 31, MSB first (the 24
// payload bits, then the first 8 parity bits); rem: received parity ^ CRC16(payload), so the whole parity is
// rem ^ CRC16(payload).  rem = PBCH_REC_NONE: not decoded (the window reaches past navail).
struct PbchRec {
  uint32_t w0, rem;
};
constexpr uint32_t PBCH_REC_NONE = 0xFFFFFFFFu;

struct PbchArgs {
  const PbchJob*  jobs;
  const uint32_t* re;    // [240] grid indices in srslte_pbch_get order
  const uint32_t* seq;   // [60] the cell's 1920 scrambling bits, bit j of word w = c(32 w + j)
  float*          llr;   // [job][nhyp][480]
  const float*    hist;  // [PBCH_HIST][480]: the frames in front of job 0 under the last hypothesis, newest last
  PbchRec*        rec;   // [job][nhyp][PBCH_WIN]
  uint32_t        nhyp;  // hypotheses tried
  uint32_t        ports[PBCH_HYPS];
};

hipError_t pbch_launch_llr(const PbchArgs& a, uint32_t njobs, hipStream_t s);
hipError_t pbch_launch_decode(const PbchArgs& a, uint32_t njobs, hipStream_t s);
// hist <- the last PBCH_HIST frames of (hist, this call's njobs frames) under the last hypothesis
hipError_t pbch_launch_save_hist(const PbchArgs& a, float* hist, uint32_t njobs, hipStream_t s);

} // namespace mi355
