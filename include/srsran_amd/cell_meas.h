/*
 * include/srsran_amd/cell_meas.h -- C ABI of the MI355X neighbour-cell measurement: RSRP, RSRQ, RSSI, CFO and frame
 * timing of cells named by their PCI, from raw I/Q, for batches of (capture, cell) pairs.
 *
 *   mi355_cell_meas_set_cells         srslte_refsignal_dl_sync_set_cell (sync/refsignal_dl_sync.c:203-270) for n cells
 *   mi355_cell_meas_run_batch         srslte_refsignal_dl_sync_run (:367-513) with srslte_refsignal_dl_sync_find_peak
 *                                     (:301-365) under it
 *   mi355_cell_meas_find_peak_batch   srslte_refsignal_dl_sync_find_peak alone
 *   mi355_cell_meas_measure_sf_batch  srslte_refsignal_dl_sync_measure_sf (:515-593)
 *   mi355_cell_meas_decide            stage 3 of srslte_refsignal_dl_sync_run (:430-511), on the host
 *
 * The sliding correlation is computed in direct form, not through the reference's FFT convolution; it and the symbol
 * correlations are summed in double and rounded to float once.  Float results agree with the reference within the
 * tolerances of tests/cell_meas_ref.py, decisions wherever the reference's own margin exceeds them.
 *
 * Normal CP and the FDD subframe structure only, as the reference (SRSLTE_CP_LEN_NORM throughout): a cell with another
 * CP or frame type is refused with MI355_ERROR_INVALID_INPUTS.
 *
 * Out of scope: the extended CP and TDD special subframes, srslte_refsignal_dl_sync_* names in the drop-in library,
 * intra_measure's ring buffer, timers and rx_gain_offset, and any CFO pre-correction of the capture.
 */
#ifndef SRSRAN_AMD_CELL_MEAS_H
#define SRSRAN_AMD_CELL_MEAS_H

#include <stddef.h>
#include <stdint.h>

#include "pdsch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI355_CELL_MEAS_MAX_CELLS 504
#define MI355_CELL_MEAS_NOT_FOUND UINT32_MAX /* peak_index of a cell that was not found */

typedef struct mi355_cell_meas mi355_cell_meas_t;

typedef struct {
  uint32_t nof_prb;    /* the bandwidth every cell of the object has: 6 .. 110 */
  uint32_t max_nof_sf; /* the longest capture in subframes: >= 2 */
} mi355_cell_meas_cfg_t;

/* One (capture, cell) pair.  input is HBM, complex float; nsamples = m * sf_len with 2 <= m <= max_nof_sf (sf_len =
 * 15 * symbol size; the reference reads past the end of its buffer otherwise); cell indexes the list given to
 * set_cells.  A job reads input[0 .. nsamples) and nothing outside it.  Many jobs may name the same input.  A job that
 * breaks this contract fails the whole call with MI355_ERROR_INVALID_INPUTS before anything is launched. */
typedef struct {
  const void* input;
  uint32_t    nsamples;
  uint32_t    cell;
} mi355_cell_meas_job_t;

/* What srslte_refsignal_dl_sync_measure_sf and refsignal_dl_pss_sss_strength give for one measured subframe.  The
 * last three are computed in subframes 0 and 5 only (sf_idx % 5 == 0) and are 0 elsewhere. */
typedef struct {
  uint32_t sf_idx;
  float    rsrp, rssi, cfo;
  float    sss_strength, sss_strength_false, rsrp_false;
} mi355_cell_meas_sf_t;

typedef struct {
  /* what the reference leaves in its struct; not found: NaN and MI355_CELL_MEAS_NOT_FOUND */
  uint32_t found;
  uint32_t peak_index;
  float    rsrp_dBfs, rssi_dBfs, rsrq_dB, cfo_Hz;
  /* inspection: stage 1 (peak_value = |correlation| at the best lag, rms_avg, the peak before the half-frame shift,
   * stage1_found = peak_value > 4 rms_avg, peak_shifted = the half-frame check moved the peak by 5 sf_len) */
  float    peak_value, rms_avg;
  uint32_t stage1_peak, stage1_found, peak_shifted;
  /* inspection: stages 2 and 3 (0 where stage 1 found nothing) */
  uint32_t sf_count, false_count, false_alarm;
} mi355_cell_meas_res_t;

/* One srslte_refsignal_dl_sync_measure_sf: reads input[0 .. sf_len). */
typedef struct {
  const void* input;
  uint32_t    cell, sf_idx;
} mi355_cell_meas_sf_job_t;

int  mi355_cell_meas_create(mi355_cell_meas_t** q, const mi355_cell_meas_cfg_t* cfg, int device);
void mi355_cell_meas_destroy(mi355_cell_meas_t* q);
/* samples per subframe at the object's bandwidth */
uint32_t mi355_cell_meas_sf_len(const mi355_cell_meas_t* q);

/* The ten time-domain subframes of each cell (PSS / SSS in subframes 0 and 5, the CRS of all nof_ports ports, OFDM
 * modulated, scaled by 1 / nof_re of port 0), generated on the GPU and resident there until the next set_cells:
 * 10 sf_len complex floats per cell.  n <= MI355_CELL_MEAS_MAX_CELLS; cells[i].nof_prb must be the object's. */
int mi355_cell_meas_set_cells(mi355_cell_meas_t* q, const mi355_cell_t* cells, uint32_t n);
/* one sequence read back: host_out receives sf_len complex floats */
int mi355_cell_meas_sequence(mi355_cell_meas_t* q, uint32_t cell, uint32_t sf_idx, float* host_out);

/* Synchronous: res[njobs] is filled on return.  sf_out is optional: per job max_nof_sf records, the first
 * res[job].sf_count of them written (sf_out[job * max_nof_sf + i]). */
int mi355_cell_meas_run_batch(mi355_cell_meas_t* q, const mi355_cell_meas_job_t* jobs, uint32_t njobs,
                              mi355_cell_meas_res_t* res, mi355_cell_meas_sf_t* sf_out, void* stream);
/* Stage 1 alone: res[job] holds peak_value, rms_avg, stage1_peak, stage1_found, peak_shifted and, as peak_index, what
 * srslte_refsignal_dl_sync_find_peak returns (MI355_CELL_MEAS_NOT_FOUND for -1); the other fields are 0. */
int mi355_cell_meas_find_peak_batch(mi355_cell_meas_t* q, const mi355_cell_meas_job_t* jobs, uint32_t njobs,
                                    mi355_cell_meas_res_t* res, void* stream);
/* out[i]: rsrp, rssi, cfo of triple i (sf_idx as given; the false fields 0) */
int mi355_cell_meas_measure_sf_batch(mi355_cell_meas_t* q, const mi355_cell_meas_sf_job_t* jobs, uint32_t njobs,
                                     mi355_cell_meas_sf_t* out, void* stream);

/* Host function: the averages, dB conversions and the four false-alarm rules with their mild / severe thresholds and
 * REFSIGNAL_DL_MAX_FAULT_CHECK over the n measured subframes, in float in the reference's order.  Fills found,
 * peak_index, the four measurements, sf_count, false_count and false_alarm of *res and leaves the stage-1 fields
 * alone.  n >= 1 (run_batch measures at least one subframe once stage 1 has a peak); n = 0 is refused with
 * MI355_ERROR_INVALID_INPUTS.  run_batch applies this function to what the GPU wrote. */
int mi355_cell_meas_decide(const mi355_cell_meas_sf_t* sf, uint32_t n, uint32_t nof_prb, uint32_t peak_idx,
                           mi355_cell_meas_res_t* res);

/* Host function: the input contract of a job list for an object of nof_prb and max_nof_sf with ncells cells set --
 * MI355_SUCCESS, or MI355_ERROR_INVALID_INPUTS if any job breaks it.  The batch calls apply the same rule
 * (srsran_amd/csrc/cell_meas_plan.h) before they launch anything. */
int mi355_cell_meas_check_jobs(const mi355_cell_meas_job_t* jobs, uint32_t njobs, uint32_t nof_prb,
                               uint32_t max_nof_sf, uint32_t ncells);

#ifdef __cplusplus
}
#endif
#endif
