/*
 * include/srsran_amd/sync.h -- C ABI of the MI355X cell search: batched PSS / SSS detection on raw I/Q, plus the
 * host-side sequence generators and the cell-search vote.
 *
 *   mi355_sync_find_batch     srslte_sync_find (sync/sync.c:631-850) and the routines under it: the PSS correlation,
 *                             its moving average, peak and peak-to-side-lobe ratio (srslte_pss_find_pss and
 *                             compute_peak_sidelobe, pss.c:413-540), the threshold test, the PSS filter and the
 *                             PSS-based CFO estimate (pss.c:594-640) with its moving average and 7 kHz rule
 *                             (sync.c:715-737), the SSS search at the FDD and TDD positions (sync.c:739-820,
 *                             find_sss.c, sss.c:128-157) and CP detection (sync.c:452-507).
 *   mi355_pss_generate ...    srslte_pss_generate / srslte_sss_generate and the put_slot functions.
 *   mi355_cellsearch_pick     get_cell (ue/ue_cell_search.c:192-253).
 *
 * The correlation is computed in direct form, not through the reference's FFT convolution; its taps are summed in
 * double and stored as float.  Float results agree with the reference within the tolerances of tests/sync_ref.py,
 * decisions wherever the reference's own margin exceeds them.
 *
 * Out of scope (a configuration that asks for one of these is refused with MI355_ERROR_INVALID_INPUTS): the integer
 * CFO search (cfo_i_enable, pss_i[]), the CP-based CFO pre-correction (cfo_cp_enable, cp.c), decimation, the
 * known-N_id_1 tracking branch of sync_sss_symbol (sync.c:519-548), sss_channel_equalize, ue_sync's find / track
 * state machine, and srslte_sync_* names in the drop-in library.
 */
#ifndef SRSRAN_AMD_SYNC_H
#define SRSRAN_AMD_SYNC_H

#include <stddef.h>
#include <stdint.h>

#include "pdsch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI355_PSS_LEN 62
#define MI355_SSS_LEN 62
#define MI355_SYNC_N_ID_2_ALL 3 /* cfg.n_id_2: three independent hypotheses, three results per job */

/* srslte_sync_find_ret_t */
enum { MI355_SYNC_FOUND = 1, MI355_SYNC_FOUND_NOSPACE = 2, MI355_SYNC_NOFOUND = 0 };
/* sss_alg_t */
enum { MI355_SSS_FULL = 0, MI355_SSS_PARTIAL_3 = 1, MI355_SSS_DIFF = 2 };
/* cfg.unsupported: the reference's switches this stage does not implement; any bit set is refused at create */
enum {
  MI355_SYNC_CFO_I_ENABLE         = 1u << 0,
  MI355_SYNC_CFO_CP_ENABLE        = 1u << 1,
  MI355_SYNC_DECIMATE             = 1u << 2,
  MI355_SYNC_KNOWN_N_ID_1         = 1u << 3,
  MI355_SYNC_SSS_CHANNEL_EQUALIZE = 1u << 4
};

typedef struct mi355_sync mi355_sync_t;

/* ---------------------------------------------------------------- host functions (no GPU) */

/* srslte_pss_generate (pss.c:346-373): 62 complex values (124 floats, re / im interleaved) */
int mi355_pss_generate(uint32_t n_id_2, float* pss62);
/* srslte_sss_generate (gen_sss.c): the 62 real values of subframe 0 and of subframe 5 */
int mi355_sss_generate(uint32_t cell_id, float* sf0_62, float* sf5_62);
/* srslte_pss_put_slot (pss.c:377-384) / srslte_sss_put_slot (sss.c:106-120): slot is a host grid of one slot
 * (complex float, nsymb x 12 nof_prb); the sequence goes into its last / second last symbol with five nulled REs on
 * either side.  cp: MI355_CP_NORM or MI355_CP_EXT. */
void mi355_pss_put_slot(const float* pss62, float* slot, uint32_t nof_prb, uint32_t cp);
void mi355_sss_put_slot(const float* sss62, float* slot, uint32_t nof_prb, uint32_t cp);

/* ---------------------------------------------------------------- the object */

typedef struct {
  uint32_t fft_size;   /* 64 .. 2048, multiple of 64 (fft_size_isvalid) */
  uint32_t max_offset; /* PSS search window in samples: the reference's pss.frame_size */
  uint32_t n_id_2;     /* 0, 1, 2 or MI355_SYNC_N_ID_2_ALL */
  float    threshold;  /* srslte_sync_set_threshold: on the peak-to-side-lobe ratio; 0 accepts every peak */
  float    ema_alpha;  /* srslte_sync_set_em_alpha: correlation average, used when 0 < alpha < 1 */
  float    cfo_ema_alpha;
  uint32_t cfo_pss_enable;
  uint32_t pss_filt_enable;
  uint32_t sss_en;
  uint32_t sss_alg; /* MI355_SSS_* */
  uint32_t detect_cp, cp;                 /* cp: the CP assumed until (or unless) one is detected */
  uint32_t detect_frame_type, frame_type; /* MI355_FDD / MI355_TDD */
  float    sss_corr_threshold;            /* srslte_sss_set_threshold */
  uint32_t unsupported;                   /* MI355_SYNC_* bits of the out-of-scope list: must be 0 */
} mi355_sync_cfg_t;

/* One call of srslte_sync_find: input is HBM, complex float.  The call reads input[0 .. find_offset + max_offset +
 * fft_size): max_offset + fft_size samples from find_offset on (max_offset for the correlation where max_offset >=
 * fft_size, max_offset + fft_size - 1 where it is smaller, pss.c:491-496; the CFO estimate reads the fft_size
 * samples that end at the peak, which may lie up to fft_size - 2 past the window), and, for the SSS and the CP
 * metrics, samples in front of the peak down to input[0], so up to find_offset samples before find_offset. */
typedef struct {
  const void* input;
  uint32_t    find_offset;
} mi355_sync_job_t;

/* What srslte_sync_find leaves behind, per job and hypothesis (res[job * nhyp + h], nhyp = 3 for N_ID_2_ALL).
 * Fields a call does not compute are returned at their reset values (0; n_id_1 = 1000, cell_id = -1). */
typedef struct {
  int32_t  ret;        /* MI355_SYNC_FOUND / FOUND_NOSPACE / NOFOUND */
  uint32_t n_id_2;     /* the hypothesis */
  uint32_t peak_pos;   /* *peak_position */
  float    peak_value; /* srslte_sync_get_peak_value: the peak-to-side-lobe ratio (0 when threshold == 0) */
  float    peak_abs;   /* pss.peak_value: the averaged |correlation|^2 at the peak */
  float    cfo_pss, cfo_pss_mean;
  uint32_t sss_available, sss_detected;
  uint32_t m0, m1;
  float    m0_value, m1_value, sss_corr;
  uint32_t n_id_1, sf_idx;
  int32_t  cell_id; /* srslte_sync_get_cell_id */
  uint32_t cp, frame_type;
  float    M_norm_avg, M_ext_avg;
} mi355_sync_res_t;

int  mi355_sync_create(mi355_sync_t** q, const mi355_sync_cfg_t* cfg, int device);
void mi355_sync_destroy(mi355_sync_t* q);
/* srslte_sync_reset + srslte_sync_cfo_reset(q, 0): clears the correlation average, cfo_pss_mean and its is_set flag,
 * M_norm_avg / M_ext_avg; the CP goes back to cfg.cp, so a sequence after a reset repeats the first one. */
int mi355_sync_reset(mi355_sync_t* q);

/* MI355_SYNC_INDEPENDENT: every job is the first call on a freshly reset object; the object's state is neither read
 *   nor written.
 * MI355_SYNC_SEQUENCE: the jobs are successive calls on one object (three objects for N_ID_2_ALL).  Carried from call
 *   to call: the correlation average conv_output_avg, cfo_pss_mean with its is_set flag (and with it the 7 kHz rule
 *   of sync.c:729), M_norm_avg / M_ext_avg and the detected CP that places the next call's SSS.  The state persists
 *   across batch calls, so a batch of n equals n batches of 1. */
enum { MI355_SYNC_INDEPENDENT = 0, MI355_SYNC_SEQUENCE = 1 };

/* Synchronous: res[njobs * nhyp] is filled on return. */
int mi355_sync_find_batch(mi355_sync_t* q, const mi355_sync_job_t* jobs, uint32_t njobs, uint32_t mode,
                          mi355_sync_res_t* res, void* stream);

/* ---------------------------------------------------------------- cell search vote */

typedef struct {
  uint32_t cell_id, cp, frame_type;
  float    peak, mode, psr, cfo;
} mi355_cellsearch_res_t;

/* get_cell (ue_cell_search.c:192-253) over the n candidates found[] (FOUND results with a valid cell id; peak =
 * peak_abs, psr = peak_value, cfo = cfo_pss_mean): the most frequent cell id, a majority CP and frame type among its
 * candidates, the mean peak, mode = share of the winning id, psr and cfo of the last candidate. */
int mi355_cellsearch_pick(const mi355_sync_res_t* found, uint32_t n, mi355_cellsearch_res_t* out);

#ifdef __cplusplus
}
#endif
#endif
