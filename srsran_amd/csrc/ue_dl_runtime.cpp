// srsran_amd/csrc/ue_dl_runtime.cpp -- host runtime behind include/srsran_amd/ue_dl.h: the srslte_ue_dl-level object
// owning the PDSCH receiver, and its OFDM, estimation and PDSCH decode entry points over batches of subframes.
#include <cmath>
#include <stdio.h>

#include "lte_common.h"
#include "sync_internal.h"
#include "ue_dl_object.h"

using namespace mi355;

static int set_dft(mi355_ue_dl_t* q)
{
  const uint32_t N = symbol_sz(q->cell.nof_prb, q->std_rates);
  OfdmArgs&      a = q->ofdm;
  if (!N || N > OFDM_MAX_N) return MI355_ERROR_INVALID_INPUTS;
  int ns = radix_plan(N, a.radix);
  if (ns < 0) return MI355_ERROR;
  a.nstages = (uint32_t)ns;
  a.N       = N;
  a.nre     = 12 * q->cell.nof_prb;
  a.nsymb   = q->cell.cp == MI355_CP_EXT ? 6 : 7;
  if (q->cell.cp == MI355_CP_EXT) {
    a.cp0 = a.cp1 = cp_len(N, 512);
  } else {
    a.cp0 = cp_len(N, 160);
    a.cp1 = cp_len(N, 144);
  }
  a.slot_sz = N * 15 / 2; // SRSLTE_SLOT_LEN
  std::vector<float2> tw(N);
  for (uint32_t m = 0; m < N; m++) {
    const double ang = -2.0 * M_PI * (double)m / (double)N;
    tw[m]            = make_float2((float)std::cos(ang), (float)std::sin(ang));
  }
  q->tw.reset();
  CHECK_HIP(q->tw.upload(tw));
  a.tw = q->tw.as<float2>();
  return MI355_SUCCESS;
}

extern "C" {

uint32_t mi355_symbol_sz(uint32_t nof_prb, int use_standard_rates) { return symbol_sz(nof_prb, use_standard_rates != 0); }

int mi355_ue_dl_create(mi355_ue_dl_t** q, const mi355_cell_t* cell, uint32_t nof_rx_antennas, int device)
{
  if (!q || !cell || cell->nof_prb == 0 || cell->nof_prb > MI355_MAX_PRB || nof_rx_antennas == 0 ||
      nof_rx_antennas > MI355_MAX_RX_ANT || !(cell->nof_ports == 1 || cell->nof_ports == 2 || cell->nof_ports == 4) ||
      cell->frame_type != MI355_FDD)
    return MI355_ERROR_INVALID_INPUTS;
  CHECK_HIP(hipSetDevice(device));
  auto* d   = new mi355_ue_dl;
  d->device = device;
  d->cell   = *cell;
  d->nof_rx = nof_rx_antennas;
  const std::vector<float2> pil = crs_table(*cell);
  // srslte_pss_generate (sync/pss.c:346-375) for N_id_2 = cell.id % 3
  std::vector<float2> pss(62);
  pss_sequence(cell->id % 3, pss.data());
  if (hipStreamCreateWithFlags(&d->own, hipStreamNonBlocking) != hipSuccess || set_dft(d) != MI355_SUCCESS ||
      d->pilots.upload(pil) != hipSuccess || d->pss.upload(pss) != hipSuccess ||
      mi355_pdsch_create(&d->pdsch, cell, nof_rx_antennas, device) != MI355_SUCCESS) {
    mi355_ue_dl_destroy(d);
    return MI355_ERROR;
  }
  *q = d;
  return MI355_SUCCESS;
}

void mi355_ue_dl_destroy(mi355_ue_dl_t* q)
{
  if (!q) return;
  (void)hipSetDevice(q->device);
  (void)hipDeviceSynchronize();
  mi355_pdsch_destroy(q->pdsch);
  if (q->own) (void)hipStreamDestroy(q->own);
  if (q->side) (void)hipStreamDestroy(q->side);
  if (q->ev_chest) (void)hipEventDestroy(q->ev_chest);
  delete q->ctrl;
  delete q->wiener;
  delete q;
}

int mi355_ue_dl_set_standard_rates(mi355_ue_dl_t* q, int enable)
{
  if (!q) return MI355_ERROR_INVALID_INPUTS;
  std::lock_guard<std::mutex> lock(q->mu);
  q->std_rates = enable != 0;
  return set_dft(q);
}

int mi355_ue_dl_set_chunks(mi355_ue_dl_t* q, uint32_t nof_chunks)
{
  if (!q || nof_chunks > 8) return MI355_ERROR_INVALID_INPUTS;
  std::lock_guard<std::mutex> lock(q->mu);
  q->chunks = nof_chunks;
  return MI355_SUCCESS;
}

void* mi355_ue_dl_get_stream(mi355_ue_dl_t* q) { return q ? (void*)q->own : nullptr; }

int mi355_ue_dl_set_ce_rows(mi355_ue_dl_t* q, uint32_t ce_rows)
{
  if (!q || ce_rows > 1) return MI355_ERROR_INVALID_INPUTS;
  std::lock_guard<std::mutex> lock(q->mu);
  q->ce_rows = ce_rows;
  return MI355_SUCCESS;
}

int mi355_ue_dl_reset_link(mi355_ue_dl_t* q, uint32_t link)
{
  if (!q || link >= MI355_MAX_LINKS) return MI355_ERROR_INVALID_INPUTS;
  std::lock_guard<std::mutex> lock(q->mu);
  if (link < q->links.size()) q->links[link] = ChestLink{};
  if (q->wiener && link < q->wiener->slabs.size() && q->wiener->slabs[link].p) return q->wiener->reset(link);
  return MI355_SUCCESS;
}

int mi355_ofdm_rx_batch(mi355_ue_dl_t* q, const mi355_dl_sf_job_t* jobs, uint32_t njobs, void* stream)
{
  if (!q || (njobs && !jobs)) return MI355_ERROR_INVALID_INPUTS;
  std::lock_guard<std::mutex> lock(q->mu);
  CHECK_HIP(hipSetDevice(q->device));
  hipStream_t s = stream ? (hipStream_t)stream : q->own;
  OfdmPlan    p;
  int         r = p.build(q, jobs, njobs, s);
  if (!r) r = p.launch(0, njobs, s);
  if (r) return r;
  CHECK_HIP(wait_stream(s));
  return MI355_SUCCESS;
}

int mi355_chest_dl_estimate_batch(mi355_ue_dl_t* q, const mi355_dl_sf_job_t* jobs, uint32_t njobs,
                                  const mi355_chest_dl_cfg_t* cfg, mi355_chest_dl_res_t* res, void* stream)
{
  if (!q || !res || (njobs && !jobs)) return MI355_ERROR_INVALID_INPUTS;
  std::lock_guard<std::mutex> lock(q->mu);
  CHECK_HIP(hipSetDevice(q->device));
  hipStream_t s = stream ? (hipStream_t)stream : q->own;
  ChestPlan   p;
  int         r = p.build(q, jobs, njobs, cfg, s, 0);
  if (!r) r = p.launch_all(q, s);
  return r ? r : chest_finish(q, cfg, p.d_out, jobs, njobs, res, s);
}

int mi355_ue_dl_decode_fft_estimate_batch(mi355_ue_dl_t* q, const mi355_dl_sf_job_t* jobs, uint32_t njobs,
                                          const mi355_chest_dl_cfg_t* cfg, mi355_chest_dl_res_t* res, void* stream)
{
  if (!q || !res || (njobs && !jobs)) return MI355_ERROR_INVALID_INPUTS;
  std::lock_guard<std::mutex> lock(q->mu);
  CHECK_HIP(hipSetDevice(q->device));
  hipStream_t s = stream ? (hipStream_t)stream : q->own;
  FrontPlan   p;
  const int   r = p.start(q, jobs, njobs, cfg, s, njobs);
  return r ? r : chest_finish(q, cfg, p.chest.d_out, jobs, njobs, res, s);
}

mi355_pdsch_t* mi355_ue_dl_pdsch(mi355_ue_dl_t* q) { return q ? q->pdsch : nullptr; }

int mi355_ue_dl_decode_batch(mi355_ue_dl_t* q, mi355_softbuffer_pool_t* pool, const mi355_dl_sf_job_t* sfjobs,
                             const mi355_dl_sf_cfg_t* sfs, const mi355_pdsch_cfg_t* cfgs,
                             const mi355_chest_dl_cfg_t* chest_cfg, mi355_chest_dl_res_t* chest,
                             uint8_t* const* payloads, uint32_t njobs, mi355_pdsch_res_t* res, void* stream)
{
  if (!q || !pool || !res || !chest || (njobs && (!sfjobs || !sfs || !cfgs || !payloads)))
    return MI355_ERROR_INVALID_INPUTS;
  std::lock_guard<std::mutex> lock(q->mu);
  const HostTime t0 = host_now();
  CHECK_HIP(hipSetDevice(q->device));
  hipStream_t s = stream ? (hipStream_t)stream : q->own;
  FrontPlan   fp;
  fp.chest.row0       = ce_row0_only(q);
  fp.chest.want_noise = true;
  int r = fp.start(q, sfjobs, njobs, chest_cfg, s, njobs);
  if (r) return r;
  // the PDSCH jobs are planned on the host while the GPU demodulates and estimates
  std::vector<mi355_pdsch_job_t> jobs(njobs);
  for (uint32_t i = 0; i < njobs; i++) pdsch_job_fill(jobs[i], q, sfjobs, sfs, cfgs, payloads, i);
  ChestFill fill{q, chest_cfg, nullptr, sfjobs, njobs, chest, false};
  if ((r = chest_finish_async(q, &fill, fp.chest.d_out, s))) return r;
  const HostTime t1 = host_now();
  r = pdsch_decode_batch_dev_noise(q->pdsch, pool, jobs.data(), njobs, res, s, fp.chest.d_noise,
                                   WaitHook{chest_fill_cb, &fill}, ce_time_invariant(chest_cfg));
  const HostTime t2 = host_now();
  CHECK_HIP(wait_stream(q->side));
  if (r) return r;
  if (!fill.done) chest_fill_cb(&fill); // no DL-SCH work in the batch: the hook did not run
  if (env_host_prof())
    fprintf(stderr, "[mi355 host] ue_dl_decode_batch: launch ofdm/chest + jobs %.1f us, pdsch+dlsch (incl. sync) %.1f us, "
                    "chest fill wait %.1f us\n", host_us(t0, t1), host_us(t1, t2), host_us(t2, host_now()));
  return r;
}

int mi355_ue_dl_decode_pdsch_batch(mi355_ue_dl_t* q, mi355_softbuffer_pool_t* pool, const mi355_dl_sf_job_t* sfjobs,
                                   const mi355_dl_sf_cfg_t* sfs, const mi355_pdsch_cfg_t* cfgs,
                                   const mi355_chest_dl_res_t* chest, uint8_t* const* payloads, uint32_t njobs,
                                   mi355_pdsch_res_t* res, void* stream)
{
  if (!q || !pool || !res || (njobs && (!sfjobs || !sfs || !cfgs || !chest || !payloads)))
    return MI355_ERROR_INVALID_INPUTS;
  std::vector<mi355_pdsch_job_t> jobs(njobs);
  for (uint32_t i = 0; i < njobs; i++) {
    pdsch_job_fill(jobs[i], q, sfjobs, sfs, cfgs, payloads, i);
    jobs[i].noise_estimate = chest[i].noise_estimate; // srslte_pdsch_decode(..., &q->chest_res, ...)
  }
  return mi355_pdsch_decode_batch(q->pdsch, pool, jobs.data(), njobs, res, stream);
}

} // extern "C"
