/*
 * include/srsran_amd/csi.h -- C ABI of the UE's channel-state feedback on the MI355X: for batches of subframes whose
 * channel estimates are in HBM, the 1-layer and 2-layer PMI selection, the TM4 rank / PMI choice, the condition number
 * with the TM3 rank, and the wideband CQI.
 *
 *   mi355_ue_dl_csi_batch          what srslte_ue_dl_gen_cqi_periodic / _aperiodic (ue/ue_dl.c:886-1010) compute per
 *                                  TTI: select_ri_pmi / select_pmi (ue_dl.c:791-863) over srslte_pdsch_select_pmi
 *                                  (phch/pdsch.c:1260-1279) -> srslte_precoding_pmi_select (mimo/precoding.c:2786-2810)
 *                                  with its 1-layer (:2363-2478) and 2-layer (:2609-2759) SIMD paths;
 *                                  srslte_ue_dl_select_ri (ue_dl.c:866-884) over srslte_pdsch_compute_cn
 *                                  (pdsch.c:1281-1284) -> srslte_precoding_cn (precoding.c:2813-2854) ->
 *                                  srslte_mat_2x2_cn (utils/mat.c:127-159); srslte_cqi_from_snr (phch/cqi.c:589-602).
 *   mi355_cqi_from_snr             srslte_cqi_from_snr.
 *   mi355_cqi_hl_get_no_subbands   srslte_cqi_hl_get_no_subbands (cqi.c:608-634).
 *   mi355_csi_decide               the decisions of select_ri_pmi, srslte_ue_dl_select_ri and the CQI from the SINR
 *                                  lists and the condition number.
 *
 * Semantics: those of the reference's AVX2 build.  With N = 14 * 12 * nof_prb estimates per grid, the PMI selection
 * reads the samples j = 24 m for m < 8 G, G = (N - 192) / 192 + 1 (whole groups of eight: 40 samples at 6 PRB, 696 at
 * 100 PRB), the condition number every j = 24 m < N (42 and 700): the last samples of a grid enter cn only.
 * Numerics: the reference's formulas in float without FMA contraction, with exact divisions where the reference takes
 * _mm256_rcp_ps (relative error up to 1.5 * 2^-12, CPU-vendor specific) and a fixed summation tree of its own, so
 * results repeat bit for bit from run to run and agree with the reference within
 *   sinr_1l  1e-5 * mean ||H||_F^2 / noise      sinr_2l  1.5e-3 * (sinr_2l + 2)      cn  1e-3 dB      cn_count exact.
 * The decisions are taken on the host (mi355_csi_decide) with the host libm's log10f, as in the reference.
 * Deviation: exactly 2 CRS ports x 2 rx antennas, the only shape for which the reference computes all three quantities
 * (its select_ri_pmi silently does nothing below 2 ports, its srslte_precoding_cn errors for anything but 2x2);
 * mi355_ue_dl_csi_batch returns MI355_ERROR_INVALID_INPUTS for every other object.
 * Deviation: normal CP only.  The reference samples SRSLTE_NOF_RE(cell) estimates (pdsch.c:1266, 1283), 12 symbols
 * with the extended CP; the sample counts here are those of the 14-symbol grid, so an extended-CP object gets
 * MI355_ERROR_INVALID_INPUTS (as from mi355_ue_dl_decode_phich_batch) and its shorter grids are never read.
 * Out: periodic-report scheduling (srslte_cqi_periodic_*), srslte_uci_data_t packing, sub-band CQI (the reference
 * reports offset 0), 4-port cells, extended-CP cells.
 */
#ifndef SRSRAN_AMD_CSI_H
#define SRSRAN_AMD_CSI_H

#include <stddef.h>
#include <stdint.h>

#include "ue_dl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI355_CSI_PMI_PRECISION 24 /* PMI_SEL_PRECISION (precoding.c:2270): every 24th estimate is a sample */
#define MI355_CSI_RI_CN_DB 17.0f   /* srslte_ue_dl_select_ri: two layers below this condition number */

/* One subframe's feedback.  The first four members are what the kernel computes; mi355_csi_decide fills the rest. */
typedef struct {
  float    sinr_1l[4]; /* linear SINR per 1-layer codebook index (w = (1, {1, -1, j, -j}) / sqrt 2) */
  float    sinr_2l[2]; /* linear sum SINR of both layers per 2-layer codebook index (1, 2 of 36.211 Table 6.3.4.2.3-1) */
  float    cn;         /* mean condition number in dB over the counted samples, 0 when none was counted */
  uint32_t cn_count;   /* samples whose eigenvalue bounds were finite */
  uint32_t pmi_1l;     /* argmax of sinr_1l from max = 0 with a strict >: 0 when no entry is positive or one is NaN */
  uint32_t pmi_2l;     /* argmax of sinr_2l, likewise */
  uint32_t ri;         /* select_ri_pmi: layers - 1 */
  uint32_t pmi;        /* select_ri_pmi: the PMI of that rank */
  float    sinr_db;    /* select_ri_pmi: 10 log10f of that entry; -INFINITY when no rank was accepted */
  uint32_t ri_cn;      /* srslte_ue_dl_select_ri (TM3): cn < 17.0f ? 1 : 0 */
  uint32_t cqi;        /* srslte_cqi_from_snr(sinr_db + snr_to_cqi_offset) */
} mi355_csi_res_t;

/* ---------------------------------------------------------------- host functions (no GPU) */

/* srslte_cqi_from_snr: the highest CQI 1..15 whose threshold {1.95, 4, 6, 8, 10, 11.95, 14.05, 16, 17.9, 20.9, 22.5,
 * 24.75, 25.5, 27.30, 29} dB (as floats) snr_db reaches, 0 below the first and for NaN */
uint32_t mi355_cqi_from_snr(float snr_db);
/* srslte_cqi_hl_get_no_subbands: ceil(nof_prb / k) with the sub-band size k = 4 (7..26 PRB), 6 (..63), 8 (..110) of
 * 36.213 Table 7.2.1-3; 0 below 7 PRB and above 110 */
int mi355_cqi_hl_get_no_subbands(uint32_t nof_prb);
/* The decisions from r->sinr_1l, r->sinr_2l and r->cn as mi355_ue_dl_csi_batch (or the reference) left them; fills
 * pmi_1l, pmi_2l, ri, pmi, sinr_db, ri_cn and cqi.  select_ri_pmi: for ri = 0, 1 the candidate is
 * 10 log10f(list[argmax]); it replaces the choice when it exceeds the best so far by more than 0.1 dB (in double, as the
 * reference's `best + 0.1`) or exceeds 20 dB.  noise_estimate is the subframe's noise: the lists are already divided by
 * it and no decision of the reference reads it again, so it changes nothing here; it is part of the call because a
 * subframe's feedback is defined by (estimates, noise, offset). */
void mi355_csi_decide(float noise_estimate, float snr_to_cqi_offset, mi355_csi_res_t* r);

/* ---------------------------------------------------------------- GPU batch */

/* The feedback of nsf subframes whose channel estimates sfjobs[i].ce[port][rx] are in HBM as
 * mi355_chest_dl_estimate_batch or the batched decode calls left them, with chest[i].noise_estimate (not normal or
 * below 1e-9: 1e-9, precoding.c:2796).  Synchronous: res[nsf] is complete on return (mi355_csi_decide applied).
 * Under mi355_ue_dl_set_ce_rows(q, 1) only row 0 of an estimate is read: sample j at j % (12 nof_prb).
 * One wavefront per subframe, one launch per call; nsf = 0 returns 0 without a launch.
 * MI355_ERROR_INVALID_INPUTS unless q has 2 CRS ports, 2 rx antennas and the normal CP, and for a null estimate
 * pointer. */
int mi355_ue_dl_csi_batch(mi355_ue_dl_t* q, const mi355_dl_sf_job_t* sfjobs, const mi355_chest_dl_res_t* chest,
                          uint32_t nsf, float snr_to_cqi_offset, mi355_csi_res_t* res, void* stream);

#ifdef __cplusplus
}
#endif
#endif
