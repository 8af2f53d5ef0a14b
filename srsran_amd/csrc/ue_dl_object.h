// srsran_amd/csrc/ue_dl_object.h -- the object behind include/srsran_amd/ue_dl.h and what its translation units share:
// ue_dl_front.cpp (OFDM / estimator plans, srslte_chest_dl_res_t), ue_dl_runtime.cpp (create / setters, the OFDM,
// estimation and decode entry points), ue_dl_find_decode.cpp (control-stage calls, find_and_decode) and
// ue_dl_feedback.cpp (UL DCI, PHICH, CSI, inspection).
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <mutex>
#include <string.h>
#include <vector>

#include "../../include/srsran_amd/pdcch.h"
#include "../../include/srsran_amd/pdsch.h"
#include "../../include/srsran_amd/ue_dl.h"
#include "device_mem.h"
#include "host_env.h"
#include "host_staging.h"
#include "pdcch_runtime.h"
#include "runtime_internal.h"
#include "ue_dl_internal.h"
#include "wiener_bank.h"

namespace mi355 {

// the values srslte_chest_dl_t carries from one subframe to the next (chest_dl.c: q->cfo, q->noise_estimate,
// q->sync_err)
struct ChestLink {
  float cfo = 0.f, sync = 0.f;
  float noise[MI355_MAX_RX_ANT][MI355_MAX_PORTS] = {};
};

// find_and_decode: one chunk's PDSCH jobs and the bookkeeping of its decode in flight
struct FdChunk {
  uint32_t                       b = 0, e = 0;
  std::vector<mi355_pdsch_job_t> jobs;
  std::vector<uint32_t>          which, rs_sb, rs_tbs;
  std::vector<mi355_pdsch_res_t> sub; // the chunk's results while its decode is in flight
  int                            r        = MI355_SUCCESS;
  bool                           launched = false; // collected even after a later error (its enqueued groups)
};

} // namespace mi355

struct mi355_ue_dl {
  mi355::WienerBank* wiener = nullptr; // WIENER estimator states per link (srslte_wiener_dl_t), built on first use
  int            device = 0;
  mi355_cell_t   cell{};
  uint32_t       nof_rx = 1;
  bool           std_rates = false;
  hipStream_t    own       = nullptr;
  mi355::OfdmArgs ofdm{};
  mi355::DevMem  tw, pilots; // float2
  mi355::DevMem  pss;        // float2: srslte_pss_generate(cell.id % 3)
  mi355_pdsch_t* pdsch  = nullptr;
  std::vector<mi355::ChestLink> links;
  mi355::DevScratch  scratch;
  mi355::HostStaging st_ofdm, st_chest, back; // pinned descriptor uploads / estimator read-back
  hipStream_t    side     = nullptr;          // estimator read-back + fill_res overlapping the PDSCH decode
  hipEvent_t     ev_chest = nullptr;
  mi355::CtrlState* ctrl  = nullptr;          // PCFICH / PDCCH stage, built on first use (ctrl_ready)
  mi355::DevScratch  d_csi;                   // CSI feedback: a call's descriptors | result records
  mi355::HostStaging st_csi, back_csi;
  std::vector<std::unique_ptr<mi355::PdschPending>> pend; // find_and_decode: per chunk, decodes left in flight
  uint32_t       chunks = 0;                              // find_and_decode chunk count (0: automatic)
  uint32_t       ce_rows = 0;                             // batched calls: 1 = AVERAGE estimate row 0 only (set_ce_rows)
  // find_and_decode's host arrays, kept from call to call: a batch's replay and grant building then write into
  // memory already mapped (1.5 MB of DCI messages and ~1 MB of job descriptors per 2,048 subframes otherwise newly
  // allocated, their first-touch page faults on the host's critical path between the chunks)
  std::vector<mi355_dci_msg_t> fd_msgs;
  std::vector<uint16_t>        fd_rntis;
  std::vector<mi355::FdChunk>  fd_ck;
  std::mutex     mu;
};

namespace mi355 {

// Two different facts let a reader of the estimates take row 0 (the first OFDM symbol's) for every symbol:
// the AVERAGE estimator writes the same estimate into every row, so a stage of the same call MAY read row 0 ...
inline bool ce_time_invariant(const mi355_chest_dl_cfg_t* cfg) { return cfg->estimator_alg == MI355_ESTIMATOR_ALG_AVERAGE; }
// ... and under set_ce_rows(1) the batched decode calls write row 0 only, so a later call on the object MUST
inline bool ce_row0_only(const mi355_ue_dl_t* q) { return q->ce_rows == 1; }
// the kernels' ce_row argument: the row length when they are to read row 0, 0 to read the estimates where they lie
inline uint32_t ce_row_arg(const mi355_ue_dl_t* q, bool row0) { return row0 ? 12 * q->cell.nof_prb : 0u; }

// The front end of a call, OFDM then estimation, as plans: build() validates the jobs, fills the descriptors (into
// the kernel arguments for srsUE's one-subframe calls, else into pinned staging, uploaded), lays out the scratch and
// launches nothing; launch(o, m, s) enqueues subframes [o, o + m).
struct OfdmPlan {
  bool            ranges = false; // set by the caller before build(): it launches subframe ranges
  OfdmArgs        a{};            // a.jobs: the uploaded table, or null with inl[] filled
  uint32_t        rx   = 1;
  size_t          used = 0;       // scratch bytes the table takes (the estimator's region starts behind them)
  int build(mi355_ue_dl_t* q, const mi355_dl_sf_job_t* jobs, uint32_t njobs, hipStream_t s);
  int launch(uint32_t o, uint32_t m, hipStream_t s) const;
};

struct ChestPlan {
  // set by the caller before build():
  bool row0       = false; // write row 0 only where the estimates are time-invariant (ce_row0_only)
  bool want_noise = false; // get_noise per job into d_noise for the equaliser / control stage
  bool ranges     = false; // the caller launches subframe ranges (chest_deferrable configurations only)
  // build():
  ChestArgs                   a{};
  const mi355_chest_dl_cfg_t* cfg   = nullptr;
  const mi355_dl_sf_job_t*    jobs  = nullptr;
  uint32_t                    njobs = 0;
  float *                     d_out = nullptr, *d_noise = nullptr; // [njobs][rx][port][CHEST_OUT] | [njobs]
  int build(mi355_ue_dl_t* q, const mi355_dl_sf_job_t* jobs, uint32_t njobs, const mi355_chest_dl_cfg_t* cfg,
            hipStream_t s, size_t offset);
  // ranges in order: a subframe 0/5 noise hold reads out_all of an earlier range only in chest_resolve
  int launch(uint32_t o, uint32_t m, hipStream_t s) const;
  // the whole batch in one pass, the only order for the configurations that are not chest_deferrable
  int launch_all(mi355_ue_dl_t* q, hipStream_t s) const;
};

// the estimator can run in consecutive subframe ranges unless a subframe's kernels depend on the estimate of an
// earlier subframe of the batch (the automatic Gauss sigma of the PSS noise, and WIENER, whose stage walks each
// link's subframes after the whole batch's estimates)
bool chest_deferrable(const mi355_chest_dl_cfg_t* cfg);

struct FrontPlan {
  OfdmPlan  ofdm;
  ChestPlan chest;
  // builds both plans, each stage's kernels enqueued as soon as its tables are up: subframes [0, m0) when
  // chest.ranges (the caller launches the later ranges with launch()), else the whole batch
  int start(mi355_ue_dl_t* q, const mi355_dl_sf_job_t* jobs, uint32_t njobs, const mi355_chest_dl_cfg_t* cfg,
            hipStream_t s, uint32_t m0);
  int launch(uint32_t o, uint32_t m, hipStream_t s) const
  {
    const int e = ofdm.launch(o, m, s);
    return e ? e : chest.launch(o, m, s);
  }
};

// srslte_chest_dl_res_t of a batch from the estimator's outputs: chest_finish synchronously; chest_finish_async
// overlapped with what follows -- the read-back runs on the side stream once the estimator has finished, and
// chest_fill_cb fills the results on the calling thread (as the DL-SCH's wait hook, after every decode kernel is
// enqueued, before the final wait; or called directly).
struct ChestFill {
  mi355_ue_dl_t*              q;
  const mi355_chest_dl_cfg_t* cfg;
  const float*                out;
  const mi355_dl_sf_job_t*    jobs;
  uint32_t                    njobs;
  mi355_chest_dl_res_t*       res;
  bool                        done;
};
void chest_fill_cb(void* p);
int  chest_finish_async(mi355_ue_dl_t* q, ChestFill* f, const float* d_out, hipStream_t s);
int  chest_finish(mi355_ue_dl_t* q, const mi355_chest_dl_cfg_t* cfg, const float* d_out, const mi355_dl_sf_job_t* jobs,
                  uint32_t njobs, mi355_chest_dl_res_t* res, hipStream_t s);

int ctrl_ready(mi355_ue_dl_t* q); // q->ctrl built (under q->mu)

// subframe i's PDSCH job, built in place (the descriptor is large: a batch's are written once, not copied): its
// grids and estimates, sfs[i], cfgs[i] and its two payload pointers
inline void pdsch_job_fill(mi355_pdsch_job_t& j, const mi355_ue_dl_t* q, const mi355_dl_sf_job_t* sfjobs,
                           const mi355_dl_sf_cfg_t* sfs, const mi355_pdsch_cfg_t* cfgs, uint8_t* const* payloads, uint32_t i)
{
  memset(&j, 0, sizeof(j));
  j.sf  = sfs[i];
  j.cfg = cfgs[i];
  for (uint32_t a = 0; a < q->nof_rx; a++) {
    j.sf_symbols[a] = sfjobs[i].sf_symbols[a];
    for (uint32_t p = 0; p < q->cell.nof_ports; p++) j.ce[p][a] = sfjobs[i].ce[p][a];
  }
  j.payload[0] = payloads[2 * i];
  j.payload[1] = payloads[2 * i + 1];
}

} // namespace mi355
