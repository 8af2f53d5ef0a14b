// srsran_amd/csrc/cell_meas_host.cpp -- host function of the neighbour-cell measurement: stage 3 of
// srslte_refsignal_dl_sync_run (refsignal_dl_sync.c:430-511) over the per-subframe records, and the check of a job list
// against the input contract.  No GPU work here.
#include <math.h>

#include "../../include/srsran_amd/cell_meas.h"
#include "../../include/srsran_amd/tdec.h"
#include "cell_meas_plan.h"

namespace {

// the reference's constants (refsignal_dl_sync.c:49-58)
constexpr float CFO_MIN_MAX_MILD = 1000.0f, CFO_MIN_MAX_SEVERE = 2000.0f;
constexpr float RSRP_MIN_MAX_MILD = 6.0f, RSRP_MIN_MAX_SEVERE = 10.0f;
constexpr float RSRP_FALSE_RATIO_MILD = 4.0f, RSRP_FALSE_RATIO_SEVERE = 3.0f;
constexpr float SSS_FALSE_RATIO_MILD = 15.0f, SSS_FALSE_RATIO_SEVERE = 1.5f;
constexpr uint32_t MAX_FAULT_CHECK = 1;

inline float power_to_dB(float v) { return 10.0f * log10f(v); }
inline float power_to_dBm(float v) { return power_to_dB(v) + 30.0f; }
inline float fmin2(float a, float b) { return a < b ? a : b; } // SRSLTE_MIN / SRSLTE_MAX
inline float fmax2(float a, float b) { return a > b ? a : b; }

void not_found(mi355_cell_meas_res_t* r)
{
  r->found      = 0;
  r->rsrp_dBfs  = NAN;
  r->rssi_dBfs  = NAN;
  r->rsrq_dB    = NAN;
  r->cfo_Hz     = NAN;
  r->peak_index = MI355_CELL_MEAS_NOT_FOUND;
}

} // namespace

extern "C" int mi355_cell_meas_decide(const mi355_cell_meas_sf_t* sf, uint32_t n, uint32_t nof_prb, uint32_t peak_idx,
                                      mi355_cell_meas_res_t* res)
{
  if (!res || !n || !sf || !nof_prb) return MI355_ERROR_INVALID_INPUTS;
  uint32_t sf_count = 0;
  float    rsrp_lin = 0.0f, rsrp_lin_min = +INFINITY, rsrp_lin_max = -INFINITY, rssi_lin = 0.0f;
  float    cfo_acc = 0.0f, cfo_min = +INFINITY, cfo_max = -INFINITY;
  float    sss_strength_avg = 0.0f, sss_strength_false_avg = 0.0f, rsrp_false_avg = 0.0f;
  bool     false_alarm = false;

  for (uint32_t i = 0; i < n; i++) {
    rsrp_lin += sf[i].rsrp;
    rsrp_lin_min = fmin2(rsrp_lin_min, sf[i].rsrp);
    rsrp_lin_max = fmax2(rsrp_lin_max, sf[i].rsrp);
    rssi_lin += sf[i].rssi;
    cfo_acc += sf[i].cfo;
    cfo_min = fmin2(cfo_min, sf[i].cfo);
    cfo_max = fmax2(cfo_max, sf[i].cfo);
    if (sf[i].sf_idx % 5 == 0) {
      sss_strength_avg += sf[i].sss_strength;
      sss_strength_false_avg += sf[i].sss_strength_false;
      rsrp_false_avg += sf[i].rsrp_false;
    }
    sf_count++;
  }
  if (sf_count) {
    rsrp_lin /= sf_count;
    rssi_lin /= sf_count;
    cfo_acc /= sf_count;
    sss_strength_avg /= (2.0f * sf_count / 10);
    sss_strength_false_avg /= (2.0f * sf_count / 10);
    rsrp_false_avg /= (2.0f * sf_count / 10);
  }
  const float rsrp_dB_min   = power_to_dBm(rsrp_lin_min);
  const float rsrp_dB_max   = power_to_dBm(rsrp_lin_max);
  const float rsrp_dB       = power_to_dBm(rsrp_lin);
  const float rsrp_false_dB = power_to_dBm(rsrp_false_avg);

  uint32_t false_count = 0;
  if (sss_strength_avg < sss_strength_false_avg * SSS_FALSE_RATIO_SEVERE) {
    false_alarm = true;
  } else if (sss_strength_avg < sss_strength_false_avg * SSS_FALSE_RATIO_MILD) {
    false_count++;
  }
  if (cfo_max - cfo_min > CFO_MIN_MAX_SEVERE) {
    false_alarm = true;
  } else if (cfo_max - cfo_min > CFO_MIN_MAX_MILD) {
    false_count++;
  }
  if (rsrp_dB_max - rsrp_dB_min > RSRP_MIN_MAX_SEVERE) {
    false_alarm = true;
  } else if (rsrp_dB_max - rsrp_dB_min > RSRP_MIN_MAX_MILD) {
    false_count++;
  }
  if (rsrp_dB - rsrp_false_dB < RSRP_FALSE_RATIO_SEVERE) {
    false_alarm = true;
  } else if (rsrp_dB - rsrp_false_dB < RSRP_FALSE_RATIO_MILD) {
    false_count++;
  }
  if (false_count > MAX_FAULT_CHECK) false_alarm = true;

  res->sf_count    = sf_count;
  res->false_count = false_count;
  res->false_alarm = false_alarm;
  if (!false_alarm) {
    res->rsrp_dBfs  = rsrp_dB;
    res->rssi_dBfs  = power_to_dBm(rssi_lin);
    res->rsrq_dB    = power_to_dB((float)nof_prb) + res->rsrp_dBfs - res->rssi_dBfs;
    res->found      = 1;
    res->cfo_Hz     = cfo_acc;
    res->peak_index = peak_idx;
  } else {
    not_found(res);
  }
  return MI355_SUCCESS;
}

extern "C" int mi355_cell_meas_check_jobs(const mi355_cell_meas_job_t* jobs, uint32_t njobs, uint32_t nof_prb,
                                          uint32_t max_nof_sf, uint32_t ncells)
{
  const uint32_t sf_len = 15 * mi355::cm_symbol_sz(nof_prb);
  if ((njobs && !jobs) || !sf_len || max_nof_sf < 2) return MI355_ERROR_INVALID_INPUTS;
  for (uint32_t i = 0; i < njobs; i++)
    if (!mi355::cm_job_ok(jobs[i], sf_len, max_nof_sf, ncells)) return MI355_ERROR_INVALID_INPUTS;
  return MI355_SUCCESS;
}
