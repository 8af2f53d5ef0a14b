// srsran_amd/csrc/sync_internal.h -- descriptors shared by the cell-search kernels (sync_kernels.hip), their host
// runtime (sync_runtime.cpp) and the host functions (sync_host.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/srsran_amd/sync.h"
#include "../../include/srsran_amd/tdec.h"

namespace mi355 {

constexpr uint32_t SSS_N        = 31;   // SRSLTE_SSS_N
constexpr uint32_t SYNC_HYPS    = 3;    // N_id_2 hypotheses
constexpr uint32_t SYNC_TILE    = 256;  // correlation outputs per workgroup
constexpr uint32_t SYNC_TAPS    = 128;  // replica taps staged in LDS at a time
constexpr uint32_t SYNC_MAX_FFT = 2048;
constexpr uint32_t N_ID_1_NONE  = 1000; // srslte_sync_init's q->N_id_1

// srslte_pss_generate (sync/pss.c:346-373) for one N_id_2, the same float / double expression
inline void pss_sequence(uint32_t n_id_2, float2* pss62)
{
  const float root_value[] = {25.0, 29.0, 34.0};
  const int   sign         = -1;
  const float root         = root_value[n_id_2];
  for (int i = 0; i < 62; i++) {
    const float arg = i < 31 ? (float)sign * M_PI * root * ((float)i * ((float)i + 1.0)) / 63.0
                             : (float)sign * M_PI * root * (((float)i + 2.0) * ((float)i + 1.0)) / 63.0;
    pss62[i] = make_float2(cosf(arg), sinf(arg));
  }
}

// SRSLTE_CP_LEN and its users (phy_common.h:121-128)
__host__ __device__ inline uint32_t sync_cp_len(uint32_t fft, uint32_t c) { return (uint32_t)(int)ceilf(((float)c * (float)fft) / 2048.0f); }
__host__ __device__ inline uint32_t sync_cp_sz(uint32_t fft, uint32_t cp) { return sync_cp_len(fft, cp == MI355_CP_NORM ? 144u : 512u); }
// the DFT bin of entry j of the 62 central subcarriers under the reference's mirror / dc placement: -31 .. -1, 1 .. 31
__host__ __device__ inline int central_bin(uint32_t j) { return j < 31 ? (int)j - 31 : (int)j - 30; }

// sss.c's tables: generate_sss_all_tables + convert_tables (gen_sss.c, find_sss.c:194-218) and generate_N_id_1_table
struct SssTables {
  float    s[SSS_N][SSS_N];
  float    z1[SSS_N][SSS_N];
  float    sd[SSS_N][SSS_N - 1];
  float    c[SYNC_HYPS][2][SSS_N];
  uint32_t n_id_1[30][30];
};
void sss_tables(SssTables* t);
// N_id_1 -> (m0, m1), 36.211 table 6.11.2.1-1
void sss_m0m1(uint32_t n_id_1, uint32_t* m0, uint32_t* m1);

struct SyncJob {
  const float2* in;
  uint32_t      find_offset;
  uint32_t      pad;
};

// per (hypothesis) state between the calls of a sequence
struct SyncState {
  float    cfo_pss_mean;
  uint32_t cfo_pss_is_set;
  float    M_norm_avg, M_ext_avg;
  uint32_t cp;
  uint32_t pad[3];
};

// what the peak kernel leaves for the scan and the SSS stage, per (job, hypothesis)
struct SyncRec {
  uint32_t found;     // over threshold
  uint32_t space;     // room for SSS / CP in front of the peak
  uint32_t cfo_valid; // cfo_pss computed in this call
  uint32_t pad;
  float    m_norm, m_ext; // M_norm / nof_symbols, M_ext / nof_symbols
  uint32_t r_norm_gt;     // R_norm > R_ext
  uint32_t cp_in;         // the CP that places this call's SSS
};

struct SyncArgs {
  const SyncJob*   jobs;
  const float2*    pss_time; // [3][fft]: conjugated, scaled time-domain replicas (srslte_pss_init_N_id_2)
  const float2*    tw;       // [fft]: exp(-j 2 pi m / fft)
  const SssTables* sss;
  float*           avg;      // [job][nhyp][L]: the call's conv_output_avg
  float*           avg_state;// [nhyp][L]
  SyncState*       state;    // [nhyp]
  SyncRec*         rec;      // [job][nhyp]
  mi355_sync_res_t* res;     // [job][nhyp]
  uint32_t         njobs, nhyp, hyp0; // hypothesis h is N_id_2 = hyp0 + h
  uint32_t         fft, N, L, nout;   // window, buffer length N + fft + 1, outputs that are computed (conv_output_len - 1)
  uint32_t         shortwin;          // N < fft (pss.c:491-496)
  uint32_t         seq;
  mi355_sync_cfg_t cfg;
};

hipError_t sync_launch_corr(const SyncArgs& a, hipStream_t s);
hipError_t sync_launch_ema_scan(const SyncArgs& a, hipStream_t s);
hipError_t sync_launch_peak(const SyncArgs& a, hipStream_t s);
hipError_t sync_launch_scan(const SyncArgs& a, hipStream_t s);
hipError_t sync_launch_sss(const SyncArgs& a, hipStream_t s);
hipError_t sync_launch_clear(float* p, size_t n, SyncState* st, uint32_t nhyp, uint32_t cp, hipStream_t s);

} // namespace mi355
