// srsran_amd/csrc/pbch_runtime.cpp -- host runtime of the PBCH receiver: the cell's RE index table and scrambling
// sequence resident in HBM, per-call descriptor upload, the LLR and decode kernels, one read-back of the decode
// records, and the host replay of srslte_pbch_decode's sequential search over them (pbch.c:501-554): first hit in
// (nant, nb, dst, src) order, reset on success, history slide after four frames without one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string.h>
#include <vector>

#include "device_mem.h"
#include "host_staging.h"
#include "lte_common.h"
#include "pbch_internal.h"

using namespace mi355;

struct mi355_pbch {
  int          device = 0;
  mi355_cell_t cell{};
  uint32_t     nhyp = 1, ports[PBCH_HYPS] = {1, 2, 4};
  hipStream_t  own  = nullptr;
  std::mutex   mu;
  DevMem       d_tab;  // re[240] | seq[60]
  DevMem       d_hist; // [PBCH_HIST][480] LLRs of the frames in front of the next call, last hypothesis, newest last
  DevScratch   d_buf;  // per-call arena: descriptors | LLRs | decode records
  HostStaging  st, back;
  // srslte_pbch_t.frame_idx between calls (0 .. 3) and, for the frames still in the history, the decode records of
  // their own calls under the last hypothesis (windows of older frames alone are not decoded again), newest last
  uint32_t frame_idx = 0;
  PbchRec  hist_rec[PBCH_HIST][PBCH_WIN];
  // the previous call's arena (inspection accessor)
  uint32_t last_n   = 0;
  float*   last_llr = nullptr;
};

namespace {

// srslte_crc_mask (pbch.c:42-45) as the 16 parity bits, MSB first
uint32_t crc_mask(uint32_t nant) { return nant == 1 ? 0x0000u : nant == 2 ? 0xFFFFu : 0x5555u; }

// srslte_pbch_crc_check (pbch.c:378-397) on a decode record: the masked CRC passes and the payload is not all zero
bool rec_ok(const PbchRec& r, uint32_t nant) { return r.rem == crc_mask(nant) && (r.w0 >> 8) != 0; }

int run(mi355_pbch_t* q, const mi355_dl_sf_job_t* sfjobs, const mi355_chest_dl_res_t* chest, uint32_t n, uint32_t mode,
        mi355_pbch_res_t* res, hipStream_t s)
{
  const bool     seq    = mode == MI355_PBCH_SEQUENCE;
  const uint32_t nhyp   = q->nhyp;
  const size_t   b_jobs = staged_size((size_t)n * sizeof(PbchJob));
  const size_t   b_llr  = staged_size((size_t)n * nhyp * PBCH_NBITS * sizeof(float));
  const size_t   b_rec  = staged_size((size_t)n * nhyp * PBCH_WIN * sizeof(PbchRec));
  const size_t   need   = b_jobs + b_llr + b_rec;
  CHECK_HIP(q->d_buf.reserve(need, need + need / 4, DevScratch::SyncFree)); // grow-only
  char* base = q->d_buf.base();
  CHECK_HIP(q->st.reserve(b_jobs));
  auto* pj = (PbchJob*)q->st.slot((size_t)n * sizeof(PbchJob));
  for (uint32_t i = 0; i < n; i++) {
    PbchJob& J = pj[i];
    memset(&J, 0, sizeof(J));
    if (!sfjobs[i].sf_symbols[0]) return MI355_ERROR_INVALID_INPUTS;
    J.grid = (const float2*)sfjobs[i].sf_symbols[0];
    for (uint32_t p = 0; p < q->cell.nof_ports; p++) {
      if (!sfjobs[i].ce[p][0]) return MI355_ERROR_INVALID_INPUTS;
      J.ce[p] = (const float2*)sfjobs[i].ce[p][0];
    }
    J.noise  = chest[i].noise_estimate;
    J.navail = seq ? std::min<uint32_t>(PBCH_HIST, q->frame_idx + i) : 0u; // (as if no job of this call succeeded)
  }
  CHECK_HIP(q->st.upload(base, s));
  PbchArgs a{};
  a.jobs = (const PbchJob*)base;
  a.re   = q->d_tab.as<uint32_t>();
  a.seq  = a.re + PBCH_NRE;
  a.llr  = (float*)(base + b_jobs);
  a.hist = q->d_hist.as<float>();
  a.rec  = (PbchRec*)(base + b_jobs + b_llr);
  a.nhyp = nhyp;
  for (uint32_t h = 0; h < PBCH_HYPS; h++) a.ports[h] = q->ports[h];
  CHECK_HIP(pbch_launch_llr(a, n, s));
  CHECK_HIP(pbch_launch_decode(a, n, s));
  if (seq) CHECK_HIP(pbch_launch_save_hist(a, q->d_hist.as<float>(), n, s));
  // the one read-back of the call: every decode's record
  const size_t nrec = (size_t)n * nhyp * PBCH_WIN;
  CHECK_HIP(q->back.reserve(nrec * sizeof(PbchRec)));
  CHECK_HIP(stage_copy(q->back.host, a.rec, nrec * sizeof(PbchRec), s));
  q->last_n = n, q->last_llr = a.llr;
  CHECK_HIP(wait_stream(s));
  const PbchRec* R = (const PbchRec*)q->back.host;
  // the record of the window (nb + 1 frames, phase dst) that ends `back` frames in front of job i
  auto rec_of = [&](uint32_t i, uint32_t h, uint32_t back, uint32_t w) -> const PbchRec& {
    if (back == 0) return R[((size_t)i * nhyp + h) * PBCH_WIN + w];
    const int j = (int)i - (int)back; // an older frame's own call, under the last hypothesis
    return j >= 0 ? R[((size_t)j * nhyp + (nhyp - 1)) * PBCH_WIN + w] : q->hist_rec[(int)PBCH_HIST + j][w];
  };
  uint32_t fidx = q->frame_idx;
  for (uint32_t i = 0; i < n; i++) {
    mi355_pbch_res_t& o = res[i];
    memset(&o, 0, sizeof(o));
    const uint32_t f = seq ? ++fidx : 1u; // q->frame_idx++ (pbch.c:489)
    bool           hit = false;
    for (uint32_t h = 0; h < nhyp && !hit; h++)
      for (uint32_t nb = 0; nb < f && !hit; nb++)
        for (uint32_t dst = 0; dst < 4 - nb && !hit; dst++)
          for (uint32_t src = 0; src < f - nb && !hit; src++) {
            const PbchRec& r = rec_of(i, h, f - 1 - (src + nb), pbch_win(nb + 1, dst));
            if (!rec_ok(r, q->ports[h])) continue;
            hit            = true;
            o.ret          = 1;
            o.nof_tx_ports = q->ports[h];
            o.sfn_offset   = (int32_t)dst - (int32_t)src + (int32_t)f - 1;
            for (uint32_t b = 0; b < MI355_BCH_PAYLOAD_LEN; b++) o.bch_payload[b] = (uint8_t)((r.w0 >> (31 - b)) & 1u);
          }
    if (!seq) continue;
    if (hit)
      fidx = 0; // srslte_pbch_decode_reset
    else if (f == 4)
      fidx = 3; // the history slides by one frame
  }
  if (seq) {
    q->frame_idx = fidx;
    PbchRec keep[PBCH_HIST][PBCH_WIN];
    for (uint32_t k = 0; k < PBCH_HIST; k++) {
      const int j = (int)n - (int)PBCH_HIST + (int)k;
      if (j >= 0)
        memcpy(keep[k], &R[((size_t)j * nhyp + (nhyp - 1)) * PBCH_WIN], sizeof(keep[k]));
      else
        memcpy(keep[k], q->hist_rec[k + n], sizeof(keep[k]));
    }
    memcpy(q->hist_rec, keep, sizeof(keep));
  }
  return MI355_SUCCESS;
}

} // namespace

extern "C" {

int mi355_pbch_create(mi355_pbch_t** q, const mi355_cell_t* cell, int device)
{
  if (!q || !cell || cell->nof_prb < 6 || cell->nof_prb > MI355_MAX_PRB || cell->id > 503 || cell->cp != MI355_CP_NORM ||
      !(cell->nof_ports == 0 || cell->nof_ports == 1 || cell->nof_ports == 2 || cell->nof_ports == 4))
    return MI355_ERROR_INVALID_INPUTS;
  CHECK_HIP(hipSetDevice(device));
  auto* d   = new mi355_pbch;
  d->device = device;
  d->cell   = *cell;
  if (cell->nof_ports == 0) { // search_all_ports (pbch.c:244-249)
    d->cell.nof_ports = MI355_MAX_PORTS;
    d->nhyp           = PBCH_HYPS;
  } else {
    d->nhyp     = 1;
    d->ports[0] = cell->nof_ports;
  }
  for (auto& f : d->hist_rec)
    for (auto& r : f) r = PbchRec{0u, PBCH_REC_NONE};
  std::vector<uint32_t> tab = pbch_re(d->cell);
  std::vector<uint8_t>  c;
  gold_sequence(cell->id, 4 * PBCH_NBITS, c); // srslte_sequence_pbch (sequences.c:29-32)
  tab.resize(PBCH_NRE + 4 * PBCH_NBITS / 32, 0u);
  for (uint32_t j = 0; j < 4 * PBCH_NBITS; j++) tab[PBCH_NRE + j / 32] |= (uint32_t)c[j] << (j % 32);
  const std::vector<float> zero(PBCH_HIST * PBCH_NBITS, 0.f);
  if (hipStreamCreateWithFlags(&d->own, hipStreamNonBlocking) != hipSuccess || d->d_tab.upload(tab) != hipSuccess ||
      d->d_hist.upload(zero) != hipSuccess) {
    mi355_pbch_destroy(d);
    return MI355_ERROR;
  }
  *q = d;
  return MI355_SUCCESS;
}

void mi355_pbch_destroy(mi355_pbch_t* q)
{
  if (!q) return;
  (void)hipSetDevice(q->device);
  (void)hipDeviceSynchronize();
  if (q->own) (void)hipStreamDestroy(q->own);
  delete q;
}

void mi355_pbch_decode_reset(mi355_pbch_t* q)
{
  if (!q) return;
  std::lock_guard<std::mutex> lock(q->mu);
  q->frame_idx = 0;
}

int mi355_pbch_decode_batch(mi355_pbch_t* q, const mi355_dl_sf_job_t* sfjobs, const mi355_chest_dl_res_t* chest,
                            uint32_t njobs, uint32_t mode, mi355_pbch_res_t* res, void* stream)
{
  if (!q || mode > MI355_PBCH_SEQUENCE || (njobs && (!sfjobs || !chest || !res))) return MI355_ERROR_INVALID_INPUTS;
  if (!njobs) return MI355_SUCCESS;
  std::lock_guard<std::mutex> lock(q->mu);
  CHECK_HIP(hipSetDevice(q->device));
  return run(q, sfjobs, chest, njobs, mode, res, stream ? (hipStream_t)stream : q->own);
}

int mi355_pbch_llr(mi355_pbch_t* q, uint32_t i, uint32_t nant, float* llr480)
{
  if (!q || !llr480 || i >= q->last_n) return MI355_ERROR_INVALID_INPUTS;
  std::lock_guard<std::mutex> lock(q->mu);
  CHECK_HIP(hipSetDevice(q->device));
  uint32_t h = 0;
  while (h < q->nhyp && q->ports[h] != nant) h++;
  if (h == q->nhyp) return MI355_ERROR_INVALID_INPUTS;
  CHECK_HIP(hipDeviceSynchronize());
  CHECK_HIP(hipMemcpy(llr480, q->last_llr + ((size_t)i * q->nhyp + h) * PBCH_NBITS, PBCH_NBITS * sizeof(float),
                      hipMemcpyDeviceToHost));
  return (int)PBCH_NBITS;
}

} // extern "C"
