// srsran_amd/csrc/pdcch_runtime.h -- the control-channel stage owned by a mi355_ue_dl_t (pdcch_runtime.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <unordered_map>
#include <vector>

#include "device_mem.h"
#include "pdcch_internal.h"

namespace mi355 {

struct HostStaging;

struct CtrlState {
  mi355_cell_t cell{};
  uint32_t     nof_rx    = 1;
  RegMap       regs;
  DevMem       d_tab;               // REG map + scrambling words (uint32_t), resident
  uint32_t     seq_words = 0;
  DevScratch   d_buf;               // per-call arena: descriptors | LLRs | CFIs | correlations | candidates
  HostStaging* st        = nullptr;
  HostStaging* back      = nullptr;
  uint32_t     last_n = 0, last_stride = 0; // the previous call's arena layout (inspection accessors)
  float*       last_llr  = nullptr;
  DciCand*     last_cand = nullptr;
  std::unordered_map<uint64_t, BlindJob> plans; // search plan per (rnti, subframe, UE configuration)
  std::vector<BlindJob>                  plan_of; // this call's plan per subframe
  // the format-0 messages the previous call's replay kept per subframe (ue_dl.c:521-529), drained by mi355_ue_dl_find_ul_dci_batch
  std::vector<mi355_dci_msg_t> ul_msgs; // [n][MI355_MAX_DCI_MSG]
  std::vector<uint32_t>        ul_cnt;  // [n], every launch() starts them at 0
  // PHICH: phich_re[ngroups][12] | phich_seq[10] behind the PDCCH words in d_tab; a call's arena and stagings
  uint32_t     phich_tab = 0, ngroups = 0;
  DevScratch   d_phich;
  HostStaging* pst   = nullptr;
  HostStaging* pback = nullptr;

  // launch(): the arena layout and the per-chunk completion events of the pending call
  size_t                b_cfi_ = 0, b_corr_ = 0;
  std::vector<uint32_t> chunk_end;
  std::vector<hipEvent_t> ev;  // chunk c's read-back landed (on rb)
  std::vector<hipEvent_t> kev; // chunk c's kernels done (on the compute stream)
  hipStream_t             rb = nullptr; // read-back stream

  ~CtrlState();
  int init(const mi355_cell_t& c, uint32_t nof_rx);
  // PCFICH + PDCCH LLRs + blind decoding of n subframes on s, then the blind-search replay (synchronous).
  // Noise per subframe from host_noise[i] or, when host_noise is null, from device memory d_noise[i].
  // ce_row: 12 nof_prb where the kernels are to read row 0 of the estimates for every symbol, else 0
  int run(const mi355_dl_sf_job_t* sfjobs, const float* host_noise, const float* d_noise, const uint16_t* rntis,
          const mi355_ue_dl_cfg_t* cfgs, uint32_t n, uint32_t ce_row, hipStream_t s, mi355_ctrl_res_t* res,
          mi355_dci_msg_t* msgs);
  // run() in two halves: launch() enqueues the kernels and read-backs of n subframes in nchunks consecutive chunks
  // (one completion event each); finish(c) waits for chunk c only and replays its blind searches, so the host
  // works on chunk c while the GPU runs the later chunks (and whatever the caller enqueued after them)
  // split0: the first chunk's size with two chunks (0: n / 2)
  // front(o, m), when given, enqueues what chunk [o, o + m) needs first (its OFDM and estimation) ahead of its kernels
  int launch(const mi355_dl_sf_job_t* sfjobs, const float* host_noise, const float* d_noise, const uint16_t* rntis,
             const mi355_ue_dl_cfg_t* cfgs, uint32_t n, uint32_t nchunks, uint32_t ce_row, uint32_t split0,
             hipStream_t s, const std::function<int(uint32_t, uint32_t)>& front = nullptr);
  int finish(uint32_t chunk, const uint16_t* rntis, const mi355_ue_dl_cfg_t* cfgs, mi355_ctrl_res_t* res,
             mi355_dci_msg_t* msgs);
  // srslte_phich_decode for njobs (subframe, resource) pairs on s, synchronous: out[i] for every job.  The caller has
  // checked sf < nsf and ngroup < ngroups, nseq < 8 for every job.  Subframe i: grids / estimates of sfjobs[i],
  // scrambling of sfs[i].tti % 10, noise chest[i].noise_estimate.
  int phich(const mi355_dl_sf_job_t* sfjobs, const mi355_dl_sf_cfg_t* sfs, const mi355_chest_dl_res_t* chest,
            uint32_t nsf, const PhichJob* jobs, uint32_t njobs, uint32_t ce_row_phich, hipStream_t s, PhichOut* out);
};

} // namespace mi355
