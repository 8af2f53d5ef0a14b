// srsran_amd/csrc/csi_host.cpp -- the host half of include/srsran_amd/csi.h: the SNR -> CQI table, the sub-band count
// and the decisions select_ri_pmi / srslte_ue_dl_select_ri take from the SINR lists and the condition number
// (ue/ue_dl.c:791-884), with the host libm's log10f as in the reference.
#include <cmath>
#include <stdint.h>

#include "../../include/srsran_amd/csi.h"

namespace {

// cqi.c:589
const float cqi_to_snr_table[15] = {1.95, 4, 6, 8, 10, 11.95, 14.05, 16, 17.9, 20.9, 22.5, 24.75, 25.5, 27.30, 29};

// srslte_precoding_pmi_select_{1,2}l: max from 0.0 with a strict > (a NaN entry exceeds nothing)
uint32_t argmax_from_zero(const float* list, uint32_t n)
{
  float    max = 0.0f;
  uint32_t at  = 0;
  for (uint32_t i = 0; i < n; i++)
    if (list[i] > max) {
      max = list[i];
      at  = i;
    }
  return at;
}

} // namespace

uint32_t mi355_cqi_from_snr(float snr_db)
{
  for (int cqi = 14; cqi >= 0; cqi--)
    if (snr_db >= cqi_to_snr_table[cqi]) return (uint32_t)cqi + 1;
  return 0;
}

int mi355_cqi_hl_get_no_subbands(uint32_t nof_prb)
{
  const int k = nof_prb < 7 ? 0 : nof_prb <= 26 ? 4 : nof_prb <= 63 ? 6 : nof_prb <= 110 ? 8 : -1;
  return k > 0 ? (int)ceil((float)nof_prb / k) : 0;
}

void mi355_csi_decide(float noise_estimate, float snr_to_cqi_offset, mi355_csi_res_t* r)
{
  (void)noise_estimate; // the lists are already divided by it (csi.h)
  if (!r) return;
  r->pmi_1l = argmax_from_zero(r->sinr_1l, 4);
  r->pmi_2l = argmax_from_zero(r->sinr_2l, 2);
  // select_ri_pmi (ue_dl.c:819-863)
  float    best_sinr_db = -INFINITY;
  uint32_t best_pmi = 0, best_ri = 0;
  for (uint32_t ri = 0; ri < 2; ri++) {
    const uint32_t pmi     = ri ? r->pmi_2l : r->pmi_1l;
    const float    sinr_db = 10.0f * log10f(ri ? r->sinr_2l[pmi] : r->sinr_1l[pmi]);
    if (sinr_db > best_sinr_db + 0.1 || sinr_db > 20.0) {
      best_sinr_db = sinr_db;
      best_pmi     = pmi;
      best_ri      = ri;
    }
  }
  r->ri      = best_ri;
  r->pmi     = best_pmi;
  r->sinr_db = best_sinr_db;
  r->ri_cn   = r->cn < MI355_CSI_RI_CN_DB ? 1u : 0u;
  r->cqi     = mi355_cqi_from_snr(best_sinr_db + snr_to_cqi_offset);
}
