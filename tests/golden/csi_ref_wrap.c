/*
 * tests/golden/csi_ref_wrap.c -- the entry points tests/golden/make_golden_csi.py calls to record the reference's
 * channel-state feedback.  Compiled by that script, in a temporary directory, together with the reference's own
 * precoding.c, mat.c and cqi.c (read where the reference tree lies); nothing compiled is kept.
 *
 * Of the reference this file calls srslte_precoding_pmi_select, srslte_precoding_cn and srslte_cqi_from_snr only, so
 * the recorded sinr_1l, sinr_2l, pmi_1l, pmi_2l, cn and the SNR -> CQI mapping are reference output.  The rank choice
 * (ri, pmi, sinr_db) and ri_cn are not: select_ri_pmi and select_pmi are static functions of ue/ue_dl.c that need a
 * whole srslte_ue_dl_t, so csiwrap_decide below states their rule in this project's words around the reference's
 * srslte_precoding_pmi_select, compiled with the reference's flags so that log10f and the float / double comparisons
 * are the reference build's.  cqi is the reference's srslte_cqi_from_snr applied to that restated sinr_db.
 */
#include <math.h>
#include <stdint.h>

#include "srslte/phy/mimo/precoding.h"
#include "srslte/phy/phch/cqi.h"
#include "srslte/phy/utils/vector.h"

/* ce[port][rx] as (re, im) float pairs, nof_symbols estimates each -> the reference's h[SRSLTE_MAX_PORTS][SRSLTE_MAX_PORTS] */
static void set_h(cf_t* h[SRSLTE_MAX_PORTS][SRSLTE_MAX_PORTS], float* ce00, float* ce01, float* ce10, float* ce11)
{
  for (int p = 0; p < SRSLTE_MAX_PORTS; p++)
    for (int r = 0; r < SRSLTE_MAX_PORTS; r++) h[p][r] = NULL;
  h[0][0] = (cf_t*)ce00;
  h[0][1] = (cf_t*)ce01;
  h[1][0] = (cf_t*)ce10;
  h[1][1] = (cf_t*)ce11;
}

/* srslte_precoding_pmi_select for nof_layers = 1 (sinr[4]) or 2 (sinr[2]); pmi starts at 0 as in
 * srslte_pdsch_select_pmi (pdsch.c:1267) */
int csiwrap_pmi_select(float* ce00, float* ce01, float* ce10, float* ce11, uint32_t nof_symbols, float noise,
                       int nof_layers, uint32_t* pmi, float* sinr)
{
  cf_t* h[SRSLTE_MAX_PORTS][SRSLTE_MAX_PORTS];
  float list[SRSLTE_MAX_CODEBOOKS];
  set_h(h, ce00, ce01, ce10, ce11);
  *pmi    = 0;
  int ret = srslte_precoding_pmi_select(h, nof_symbols, noise, nof_layers, pmi, list);
  for (int i = 0; i < ret && i < SRSLTE_MAX_CODEBOOKS; i++) sinr[i] = list[i];
  return ret;
}

/* srslte_precoding_cn for 2 x 2 */
int csiwrap_cn(float* ce00, float* ce01, float* ce10, float* ce11, uint32_t nof_symbols, float* cn)
{
  cf_t* h[SRSLTE_MAX_PORTS][SRSLTE_MAX_PORTS];
  set_h(h, ce00, ce01, ce10, ce11);
  return srslte_precoding_cn(h, 2, 2, nof_symbols, cn);
}

/* The rank / PMI choice the UE reports in TM4, written out for the two ranks a 2 x 2 link has.  This is a restatement
 * of ours, not reference output: what it must agree with is the rule of ue_dl.c:819-863 -- the ranks are visited in
 * order from a best value of -INFINITY, and a rank takes over when its SINR in dB exceeds the best so far by more than
 * 0.1 (the sum formed in double) or exceeds 20 dB.  Visiting one layer first against -INFINITY, it is taken exactly
 * when its dB value is a number above -INFINITY; two layers are then measured against whatever one layer left.
 * The SINR lists, the argmaxes and the CQI are the reference's own (srslte_precoding_pmi_select, srslte_cqi_from_snr).
 * TM3's rank from the condition number (ue_dl.c:879) is the comparison with 17 dB. */
typedef struct {
  uint32_t pmi; /* srslte_precoding_pmi_select's argmax, 0 when it wrote none */
  float    db;  /* 10 log10f of that list entry */
} csiwrap_cand_t;

static int candidate(cf_t* h[SRSLTE_MAX_PORTS][SRSLTE_MAX_PORTS], uint32_t nof_symbols, float noise, int layers,
                     csiwrap_cand_t* c)
{
  float list[SRSLTE_MAX_CODEBOOKS];
  c->pmi = 0;
  if (srslte_precoding_pmi_select(h, nof_symbols, noise, layers, &c->pmi, list) < 0) return -1;
  c->db = srslte_convert_power_to_dB(list[c->pmi % SRSLTE_MAX_CODEBOOKS]);
  return 0;
}

int csiwrap_decide(float* ce00, float* ce01, float* ce10, float* ce11, uint32_t nof_symbols, float noise, float cn,
                   float snr_to_cqi_offset, uint32_t* ri, uint32_t* pmi, float* sinr_db, uint32_t* ri_cn, uint32_t* cqi)
{
  cf_t*          h[SRSLTE_MAX_PORTS][SRSLTE_MAX_PORTS];
  csiwrap_cand_t one, two;
  set_h(h, ce00, ce01, ce10, ce11);
  if (candidate(h, nof_symbols, noise, 1, &one) || candidate(h, nof_symbols, noise, 2, &two)) return -1;
  /* nothing chosen yet: rank 0, PMI 0, -INFINITY dB */
  *ri      = 0;
  *pmi     = 0;
  *sinr_db = -INFINITY;
  /* against -INFINITY the 0.1 dB margin changes nothing, and what exceeds 20 dB exceeds -INFINITY too */
  if (one.db > -INFINITY) {
    *pmi     = one.pmi;
    *sinr_db = one.db;
  }
  const double margin = (double)*sinr_db + 0.1;
  if ((double)two.db > margin || (double)two.db > 20.0) {
    *ri      = 1;
    *pmi     = two.pmi;
    *sinr_db = two.db;
  }
  *ri_cn = cn < 17.0f ? 1u : 0u;
  *cqi   = srslte_cqi_from_snr(*sinr_db + snr_to_cqi_offset);
  return 0;
}

uint32_t csiwrap_cqi_from_snr(float snr) { return srslte_cqi_from_snr(snr); }

/* the reference's ERROR / INFO macros end here once a log handler is registered (none is); phy_logger.c itself needs
 * the generated srslte/version.h */
#include "srslte/phy/utils/phy_logger.h"
void srslte_phy_log_print(phy_logger_level_t level, const char* format, ...)
{
  (void)level;
  (void)format;
}
