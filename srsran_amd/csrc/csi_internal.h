// srsran_amd/csrc/csi_internal.h -- records shared by the CSI feedback kernel (csi_kernels.hip), its runtime
// (mi355_ue_dl_csi_batch in ue_dl_feedback.cpp) and the host decisions (csi_host.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace mi355 {

constexpr uint32_t CSI_STEP = 24; // PMI_SEL_PRECISION: every 24th estimate of a grid is a sample
constexpr uint32_t CSI_SIMD = 8;  // SRSLTE_SIMD_CF_SIZE of the AVX2 build: the PMI selection takes whole groups of eight

// samples of the condition number (every j = 24 m < 14 * 12 * nof_prb) and groups of the PMI selection
// (j = 0, 192, ... while j < N - 192 + 1)
inline uint32_t csi_cn_samples(uint32_t nof_prb) { return 14 * 12 * nof_prb / CSI_STEP; }
inline uint32_t csi_pmi_groups(uint32_t nof_prb)
{
  const uint32_t N = 14 * 12 * nof_prb, g = CSI_STEP * CSI_SIMD;
  return N < g ? 0 : (N - g) / g + 1;
}

struct CsiJob {
  const float2* ce[2][2]; // [port][rx]
  float         noise;    // bounded (precoding.c:2796)
  uint32_t      pad;
};
// what the kernel writes per subframe: the head of mi355_csi_res_t
struct CsiOut {
  float    sinr_1l[4];
  float    sinr_2l[2];
  float    cn;
  uint32_t cn_count;
};
struct CsiArgs {
  const CsiJob* jobs;
  CsiOut*       out;    // [nsf]
  uint32_t      nsf;
  uint32_t      n_cn;   // samples m < n_cn enter the condition number
  uint32_t      groups; // samples m < 8 groups enter the SINRs
  uint32_t      ce_row; // estimates hold row 0 only: sample j is read at j % ce_row (0: at j)
};
hipError_t csi_launch(const CsiArgs& a, hipStream_t s);

} // namespace mi355
