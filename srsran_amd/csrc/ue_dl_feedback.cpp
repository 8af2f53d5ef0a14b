// srsran_amd/csrc/ue_dl_feedback.cpp -- what the UE sends back or acts on after a control-stage call: the UL grants
// (DCI format 0) its replay kept, PHICH decoding and the CSI feedback; and the control stage's inspection accessors.
#include <algorithm>
#include <cmath>

#include "../../include/srsran_amd/csi.h"
#include "../../include/srsran_amd/phich.h"
#include "csi_internal.h"
#include "ue_dl_object.h"

using namespace mi355;

extern "C" {

// srslte_ue_dl_find_ul_dci (ue_dl.c:613-641) over the lists the previous control-stage call's replay kept
int mi355_ue_dl_find_ul_dci_batch(mi355_ue_dl_t* q, const mi355_dl_sf_cfg_t* sfs, const mi355_ue_dl_cfg_t* cfgs,
                                  const uint16_t* rntis, uint32_t njobs, int32_t* nof_ul, mi355_dci_ul_t* dci_ul)
{
  if (!q || (njobs && (!sfs || !cfgs || !rntis || !nof_ul || !dci_ul))) return MI355_ERROR_INVALID_INPUTS;
  std::lock_guard<std::mutex> lock(q->mu);
  if (!njobs) return MI355_SUCCESS;
  if (!q->ctrl || njobs > q->ctrl->ul_cnt.size()) return MI355_ERROR_INVALID_INPUTS;
  for (uint32_t i = 0; i < njobs; i++) {
    nof_ul[i] = 0;
    if (!rntis[i]) continue; // (the list stays, as in the reference)
    const uint32_t n     = std::min<uint32_t>(MI355_MAX_DCI_MSG, q->ctrl->ul_cnt[i]);
    q->ctrl->ul_cnt[i]   = 0;
    mi355_dci_msg_t* pen = q->ctrl->ul_msgs.data() + (size_t)i * MI355_MAX_DCI_MSG;
    nof_ul[i]            = (int32_t)n;
    for (uint32_t k = 0; k < n; k++)
      if (mi355_dci_msg_unpack_pusch(&q->cell, &sfs[i], &cfgs[i].dci, &pen[k], &dci_ul[(size_t)i * MI355_MAX_DCI_MSG + k])) {
        nof_ul[i] = -1; // "Unpacking UL DCI"
        break;
      }
  }
  return MI355_SUCCESS;
}

// srslte_ue_dl_decode_phich (ue_dl.c:757-790) per job; jobs the reference's srslte_phich_decode refuses
// (phich.c:217-220) are answered on the host
int mi355_ue_dl_decode_phich_batch(mi355_ue_dl_t* q, const mi355_dl_sf_job_t* sfjobs, const mi355_dl_sf_cfg_t* sfs,
                                   const mi355_chest_dl_res_t* chest, uint32_t nsf, const mi355_phich_job_t* jobs,
                                   uint32_t njobs, mi355_phich_res_t* res, void* stream)
{
  if (!q || (njobs && (!jobs || !res)) || (njobs && nsf && (!sfjobs || !sfs || !chest))) return MI355_ERROR_INVALID_INPUTS;
  if (!njobs) return MI355_SUCCESS;
  if (q->cell.cp != MI355_CP_NORM) return MI355_ERROR_INVALID_INPUTS;
  std::lock_guard<std::mutex> lock(q->mu);
  CHECK_HIP(hipSetDevice(q->device));
  int r = ctrl_ready(q);
  if (r) return r;
  std::vector<PhichJob> dev;
  std::vector<uint32_t> which;
  dev.reserve(njobs), which.reserve(njobs);
  for (uint32_t i = 0; i < njobs; i++) {
    res[i] = mi355_phich_res_t{MI355_ERROR_INVALID_INPUTS, 0u, 0.f};
    mi355_phich_resource_t n{};
    if (jobs[i].sf >= nsf || mi355_phich_calc(&q->cell, &jobs[i].grant, &n) || n.ngroup >= q->ctrl->ngroups) continue;
    dev.push_back(PhichJob{jobs[i].sf, n.ngroup, n.nseq});
    which.push_back(i);
  }
  if (dev.empty()) return MI355_SUCCESS;
  std::vector<PhichOut> out(dev.size());
  // estimates written by the batched decode calls under set_ce_rows(1) have row 0 only
  if ((r = q->ctrl->phich(sfjobs, sfs, chest, nsf, dev.data(), (uint32_t)dev.size(), ce_row_arg(q, ce_row0_only(q)),
                          stream ? (hipStream_t)stream : q->own, out.data())))
    return r;
  for (size_t k = 0; k < dev.size(); k++) res[which[k]] = mi355_phich_res_t{MI355_SUCCESS, out[k].ack, out[k].distance};
  return MI355_SUCCESS;
}

// the per-TTI feedback of srslte_ue_dl_gen_cqi_periodic / _aperiodic (ue_dl.c:886-1010) per subframe: descriptors up,
// one csi_feedback launch, 32 bytes per subframe back, the decisions on the host
int mi355_ue_dl_csi_batch(mi355_ue_dl_t* q, const mi355_dl_sf_job_t* sfjobs, const mi355_chest_dl_res_t* chest,
                          uint32_t nsf, float snr_to_cqi_offset, mi355_csi_res_t* res, void* stream)
{
  if (!q || (nsf && (!sfjobs || !chest || !res))) return MI355_ERROR_INVALID_INPUTS;
  // the one shape for which the reference computes the SINR lists and the condition number (csi.h)
  if (q->cell.nof_ports != 2 || q->nof_rx != 2) return MI355_ERROR_INVALID_INPUTS;
  // the sample counts (csi_internal.h) are those of a 14-symbol grid: an extended-CP grid holds 12 symbols, and
  // sampling it as 14 would read past its end
  if (q->cell.cp != MI355_CP_NORM) return MI355_ERROR_INVALID_INPUTS;
  if (!nsf) return MI355_SUCCESS;
  std::lock_guard<std::mutex> lock(q->mu);
  CHECK_HIP(hipSetDevice(q->device));
  hipStream_t  s     = stream ? (hipStream_t)stream : q->own;
  const size_t b_job = staged_size((size_t)nsf * sizeof(CsiJob)), b_out = staged_size((size_t)nsf * sizeof(CsiOut));
  // Nothing of an earlier call on this object is in flight (every call ends with a wait), so an outgrown arena could
  // be freed -- but hipFree (SyncFree) waits for the whole device and would stall the other workers' streams.  Retire
  // keeps the outgrown buffers until destruction instead: 72 bytes per subframe, grown by a quarter each time
  CHECK_HIP(q->d_csi.reserve(b_job + b_out, b_job + b_out + (b_job + b_out) / 4, DevScratch::Retire));
  char* base = q->d_csi.base();
  CHECK_HIP(q->st_csi.reserve(b_job));
  auto* cj = (CsiJob*)q->st_csi.slot((size_t)nsf * sizeof(CsiJob));
  for (uint32_t i = 0; i < nsf; i++) {
    for (uint32_t p = 0; p < 2; p++)
      for (uint32_t r = 0; r < 2; r++) {
        if (!sfjobs[i].ce[p][r]) return MI355_ERROR_INVALID_INPUTS;
        cj[i].ce[p][r] = (const float2*)sfjobs[i].ce[p][r];
      }
    // srslte_precoding_pmi_select (precoding.c:2796): bound the noise estimate
    const float n = chest[i].noise_estimate;
    cj[i].noise   = (!std::isnormal(n) || n < 1e-9f) ? 1e-9f : n;
    cj[i].pad     = 0;
  }
  CHECK_HIP(q->st_csi.upload(base, s));
  CsiArgs a{};
  a.jobs   = (const CsiJob*)base;
  a.out    = (CsiOut*)(base + b_job);
  a.nsf    = nsf;
  a.n_cn   = csi_cn_samples(q->cell.nof_prb);
  a.groups = csi_pmi_groups(q->cell.nof_prb);
  // estimates written by the batched decode calls under set_ce_rows(1) have row 0 only
  a.ce_row = ce_row_arg(q, ce_row0_only(q));
  CHECK_HIP(csi_launch(a, s));
  CHECK_HIP(q->back_csi.reserve((size_t)nsf * sizeof(CsiOut)));
  CHECK_HIP(stage_copy(q->back_csi.host, a.out, (size_t)nsf * sizeof(CsiOut), s));
  CHECK_HIP(wait_stream(s));
  const CsiOut* o = (const CsiOut*)q->back_csi.host;
  for (uint32_t i = 0; i < nsf; i++) {
    mi355_csi_res_t& r = res[i];
    memset(&r, 0, sizeof(r));
    memcpy(r.sinr_1l, o[i].sinr_1l, sizeof(r.sinr_1l));
    memcpy(r.sinr_2l, o[i].sinr_2l, sizeof(r.sinr_2l));
    r.cn       = o[i].cn;
    r.cn_count = o[i].cn_count;
    mi355_csi_decide(chest[i].noise_estimate, snr_to_cqi_offset, &r);
  }
  return MI355_SUCCESS;
}

int mi355_ue_dl_ctrl_llr(mi355_ue_dl_t* q, uint32_t i, float* llr, uint32_t max_llr)
{
  if (!q || !llr) return MI355_ERROR_INVALID_INPUTS;
  std::lock_guard<std::mutex> lock(q->mu);
  if (!q->ctrl || i >= q->ctrl->last_n) return MI355_ERROR_INVALID_INPUTS;
  CHECK_HIP(hipSetDevice(q->device));
  uint32_t cfi = 0;
  CHECK_HIP(hipDeviceSynchronize());
  // the CFI array follows the LLRs in the arena (pdcch_runtime.cpp)
  const char* cfi_base = (const char*)(q->ctrl->last_llr) + staged_size((size_t)q->ctrl->last_n * q->ctrl->last_stride * 4);
  CHECK_HIP(hipMemcpy(&cfi, cfi_base + 4 * i, 4, hipMemcpyDeviceToHost));
  if (cfi < 1 || cfi > 3) return MI355_ERROR;
  const uint32_t n = std::min(8 * q->ctrl->regs.nregs[cfi - 1], max_llr);
  CHECK_HIP(hipMemcpy(llr, q->ctrl->last_llr + (size_t)i * q->ctrl->last_stride, n * 4, hipMemcpyDeviceToHost));
  return (int)n;
}

int mi355_ue_dl_ctrl_candidates(mi355_ue_dl_t* q, uint32_t i, uint32_t* out, uint32_t max_words)
{
  if (!q || !out) return MI355_ERROR_INVALID_INPUTS;
  std::lock_guard<std::mutex> lock(q->mu);
  if (!q->ctrl || i >= q->ctrl->last_n) return MI355_ERROR_INVALID_INPUTS;
  CHECK_HIP(hipSetDevice(q->device));
  const uint32_t words = std::min<uint32_t>(PDCCH_SLOTS * PDCCH_FMTS * sizeof(DciCand) / 4, max_words);
  CHECK_HIP(hipDeviceSynchronize());
  CHECK_HIP(hipMemcpy(out, q->ctrl->last_cand + (size_t)i * PDCCH_SLOTS * PDCCH_FMTS, words * 4, hipMemcpyDeviceToHost));
  return (int)words;
}

} // extern "C"
