// srsran_amd/csrc/cell_meas_runtime.cpp -- host runtime of the neighbour-cell measurement: the cells' time-domain
// sequences generated on the GPU and resident in HBM, the per-call plan (cell_meas_plan.h), descriptor upload, the two
// launches of a run, one read-back of the per-job and per-subframe records and the host's decision on them.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <string.h>
#include <vector>

#include "cell_meas_internal.h"
#include "device_mem.h"
#include "host_staging.h"
#include "lte_common.h"
#include "sync_internal.h"
#include "ue_dl_internal.h"

using namespace mi355;

struct mi355_cell_meas {
  int                       device = 0;
  mi355_cell_meas_cfg_t     cfg{};
  uint32_t                  N = 0, cp0 = 0, cp1 = 0, sf_len = 0, ntiles = 0;
  hipStream_t               own = nullptr;
  std::mutex                mu;
  OfdmArgs                  ofdm{};
  DevMem                    d_tw, d_pss; // modulator twiddles [N] | PSS [3][62]
  DevMem                    d_seq;       // [cell][10][sf_len]
  std::vector<mi355_cell_t> cells;
  DevScratch                d_buf; // per-call arena: groups | jobs | partials | heads | subframe records
  HostStaging               st, back;
};

namespace {

constexpr size_t GRID_CHUNK_BYTES = 64u << 20; // resource grids held at a time while the sequences are built

int build_sequences(mi355_cell_meas_t* q, const mi355_cell_t* cells, uint32_t n)
{
  const uint32_t nre = 12 * q->cfg.nof_prb, nref = 2 * q->cfg.nof_prb, L = q->sf_len;
  const size_t   grid_b = (size_t)10 * 14 * nre * sizeof(float2);
  const uint32_t chunk  = (uint32_t)std::max<size_t>(1, std::min<size_t>(n, GRID_CHUNK_BYTES / grid_b));
  CHECK_HIP(q->d_seq.alloc((size_t)n * 10 * L * sizeof(float2)));
  DevMem d_grid, d_cells, d_pil, d_sss, d_jobs;
  CHECK_HIP(d_grid.alloc(chunk * grid_b));
  std::vector<CmCellDev> cd;
  std::vector<float2>    pil;
  std::vector<float>     sss;
  std::vector<OfdmJob>   oj;
  for (uint32_t c0 = 0; c0 < n; c0 += chunk) {
    const uint32_t nc = std::min(chunk, n - c0);
    cd.resize(nc), sss.resize((size_t)nc * 2 * 62), oj.resize((size_t)nc * 10);
    pil.clear();
    for (uint32_t i = 0; i < nc; i++) {
      const mi355_cell_t& c = cells[c0 + i];
      cd[i]                 = CmCellDev{c.id, c.nof_ports};
      const auto t          = crs_table(c); // [2][10][4 nref]
      pil.insert(pil.end(), t.begin(), t.end());
      if (mi355_sss_generate(c.id, &sss[(size_t)i * 124], &sss[(size_t)i * 124 + 62]) != MI355_SUCCESS)
        return MI355_ERROR;
      for (uint32_t sf = 0; sf < 10; sf++)
        oj[(size_t)i * 10 + sf] = OfdmJob{d_grid.as<float2>() + ((size_t)i * 10 + sf) * 14 * nre,
                                          q->d_seq.as<float2>() + ((size_t)(c0 + i) * 10 + sf) * L};
    }
    if (pil.size() != (size_t)nc * 2 * 10 * 4 * nref) return MI355_ERROR;
    CHECK_HIP(d_cells.upload(cd));
    CHECK_HIP(d_pil.upload(pil));
    CHECK_HIP(d_sss.upload(sss));
    CHECK_HIP(d_jobs.upload(oj));
    CmGridArgs g{};
    g.cells = d_cells.as<CmCellDev>(), g.pilots = d_pil.as<float2>(), g.pss = q->d_pss.as<float2>();
    g.sss = d_sss.as<float>(), g.grids = d_grid.as<float2>(), g.n = nc, g.nof_prb = q->cfg.nof_prb;
    CHECK_HIP(cm_launch_grid(g, q->own));
    OfdmArgs a = q->ofdm;
    a.jobs     = d_jobs.as<OfdmJob>();
    // set_cell :258-264: the unnormalised modulator, then 1 / nof_re of port 0 (4 symbols x 2 nof_prb)
    CHECK_HIP(ofdm_launch_tx(a, 1.0f / (float)(4 * nref), nc * 10, q->own));
    CHECK_HIP(wait_stream(q->own)); // the chunk's tables and grids are reused
  }
  return MI355_SUCCESS;
}

CmArgs base_args(const mi355_cell_meas_t* q)
{
  CmArgs a{};
  a.seq     = q->d_seq.as<float2>();
  a.nof_prb = q->cfg.nof_prb, a.N = q->N, a.cp0 = q->cp0, a.cp1 = q->cp1, a.sf_len = q->sf_len;
  a.ntiles = q->ntiles, a.max_nof_sf = q->cfg.max_nof_sf;
  return a;
}

int run(mi355_cell_meas_t* q, const mi355_cell_meas_job_t* jobs, uint32_t n, bool stage2, mi355_cell_meas_res_t* res,
        mi355_cell_meas_sf_t* sf_out, hipStream_t s)
{
  std::vector<CmGroup> groups;
  if (!cm_plan(jobs, n, q->sf_len, q->cfg.max_nof_sf, (uint32_t)q->cells.size(), groups))
    return MI355_ERROR_INVALID_INPUTS;
  const uint32_t M      = q->cfg.max_nof_sf;
  const size_t   b_grp  = staged_size(groups.size() * sizeof(CmGroup));
  const size_t   b_jobs = staged_size((size_t)n * sizeof(CmJobDev));
  const size_t   b_part = staged_size((size_t)n * CM_MAX_BLOCKS * q->ntiles * sizeof(CmPartial));
  const size_t   b_head = staged_size((size_t)n * sizeof(CmHead));
  const size_t   b_sf   = staged_size((size_t)n * M * sizeof(mi355_cell_meas_sf_t));
  const size_t   need   = b_grp + b_jobs + b_part + b_head + b_sf;
  CHECK_HIP(q->d_buf.reserve(need, need + need / 4, DevScratch::SyncFree)); // grow-only
  char* base = q->d_buf.base();
  CHECK_HIP(q->st.reserve(b_grp + b_jobs));
  memcpy(q->st.slot(groups.size() * sizeof(CmGroup)), groups.data(), groups.size() * sizeof(CmGroup));
  auto*    pj         = (CmJobDev*)q->st.slot((size_t)n * sizeof(CmJobDev));
  uint32_t max_blocks = 0;
  for (uint32_t i = 0; i < n; i++) pj[i] = CmJobDev{(const float2*)jobs[i].input, jobs[i].nsamples, jobs[i].cell};
  for (const CmGroup& g : groups) max_blocks = std::max(max_blocks, g.nblocks);
  CHECK_HIP(q->st.upload(base, s));
  CmArgs a  = base_args(q);
  a.groups  = (const CmGroup*)base;
  a.jobs    = (const CmJobDev*)(base + b_grp);
  a.part    = (CmPartial*)(base + b_grp + b_jobs);
  a.head    = (CmHead*)(base + b_grp + b_jobs + b_part);
  a.sf      = (mi355_cell_meas_sf_t*)(base + b_grp + b_jobs + b_part + b_head);
  a.njobs = n, a.ngroups = (uint32_t)groups.size(), a.max_blocks = max_blocks, a.stage2 = stage2;
  // the launches and the one read-back of the call; whatever fails, the stream is waited for before returning, so
  // that neither staging buffer is left in flight
  const size_t bytes = b_head + (stage2 ? b_sf : 0);
  hipError_t   e     = q->back.reserve(bytes);
  if (e == hipSuccess) e = cm_launch_corr(a, s);
  if (e == hipSuccess) e = cm_launch_measure(a, s);
  if (e == hipSuccess) e = stage_copy(q->back.host, a.head, bytes, s);
  const hipError_t w = wait_stream(s);
  CHECK_HIP(e);
  CHECK_HIP(w);
  const auto* head = (const CmHead*)q->back.host;
  const auto* sf   = (const mi355_cell_meas_sf_t*)(q->back.host + b_head);
  for (uint32_t i = 0; i < n; i++) {
    const CmHead&          H = head[i];
    mi355_cell_meas_res_t& r = res[i];
    memset(&r, 0, sizeof(r));
    r.peak_value = H.peak_value, r.rms_avg = H.rms_avg;
    r.stage1_peak = H.stage1_peak, r.stage1_found = H.stage1_found, r.peak_shifted = H.peak_shifted;
    if (!stage2) {
      r.peak_index = H.peak_idx < 0 ? MI355_CELL_MEAS_NOT_FOUND : (uint32_t)H.peak_idx;
      continue;
    }
    if (H.peak_idx < 0) {
      r.rsrp_dBfs = r.rssi_dBfs = r.rsrq_dB = r.cfo_Hz = NAN;
      r.peak_index                                     = MI355_CELL_MEAS_NOT_FOUND;
      continue;
    }
    const uint32_t cnt = std::min(H.sf_count, M);
    if (mi355_cell_meas_decide(sf + (size_t)i * M, cnt, q->cfg.nof_prb, (uint32_t)H.peak_idx, &r) != MI355_SUCCESS)
      return MI355_ERROR;
    if (sf_out) memcpy(sf_out + (size_t)i * M, sf + (size_t)i * M, cnt * sizeof(mi355_cell_meas_sf_t));
  }
  return MI355_SUCCESS;
}

} // namespace

extern "C" {

int mi355_cell_meas_create(mi355_cell_meas_t** q, const mi355_cell_meas_cfg_t* cfg, int device)
{
  if (!q || !cfg || cfg->nof_prb < 6 || cfg->nof_prb > 110 || cfg->max_nof_sf < 2 || cfg->max_nof_sf > 4096)
    return MI355_ERROR_INVALID_INPUTS;
  const uint32_t N = cm_symbol_sz(cfg->nof_prb);
  uint32_t       radix[OFDM_MAX_STAGES];
  const int      nst = radix_plan(N, radix);
  if (!N || N > OFDM_MAX_N || nst < 0) return MI355_ERROR_INVALID_INPUTS;
  CHECK_HIP(hipSetDevice(device));
  auto* d   = new mi355_cell_meas;
  d->device = device;
  d->cfg    = *cfg;
  d->N = N, d->cp0 = cp_len(N, 160), d->cp1 = cp_len(N, 144), d->sf_len = 15 * N, d->ntiles = cm_ntiles(15 * N);
  OfdmArgs& a = d->ofdm;
  a.N = N, a.nstages = (uint32_t)nst;
  memcpy(a.radix, radix, sizeof(radix));
  a.nre = 12 * cfg->nof_prb, a.nsymb = 7, a.cp0 = d->cp0, a.cp1 = d->cp1, a.slot_sz = N * 15 / 2;
  std::vector<float2> tw(N), pss(3 * MI355_PSS_LEN);
  for (uint32_t m = 0; m < N; m++) {
    const double ang = -2.0 * M_PI * (double)m / (double)N;
    tw[m]            = make_float2((float)std::cos(ang), (float)std::sin(ang));
  }
  for (uint32_t i = 0; i < 3; i++) pss_sequence(i, &pss[i * MI355_PSS_LEN]);
  if (hipStreamCreateWithFlags(&d->own, hipStreamNonBlocking) != hipSuccess || d->d_tw.upload(tw) != hipSuccess ||
      d->d_pss.upload(pss) != hipSuccess) {
    mi355_cell_meas_destroy(d);
    return MI355_ERROR;
  }
  a.tw = d->d_tw.as<float2>();
  *q   = d;
  return MI355_SUCCESS;
}

void mi355_cell_meas_destroy(mi355_cell_meas_t* q)
{
  if (!q) return;
  (void)hipSetDevice(q->device);
  (void)hipDeviceSynchronize();
  if (q->own) (void)hipStreamDestroy(q->own);
  delete q;
}

uint32_t mi355_cell_meas_sf_len(const mi355_cell_meas_t* q) { return q ? q->sf_len : 0; }

int mi355_cell_meas_set_cells(mi355_cell_meas_t* q, const mi355_cell_t* cells, uint32_t n)
{
  if (!q || !cells || !n || n > MI355_CELL_MEAS_MAX_CELLS) return MI355_ERROR_INVALID_INPUTS;
  for (uint32_t i = 0; i < n; i++) {
    const mi355_cell_t& c = cells[i];
    if (c.nof_prb != q->cfg.nof_prb || c.id > 503 || (c.nof_ports != 1 && c.nof_ports != 2 && c.nof_ports != 4) ||
        c.cp != MI355_CP_NORM || c.frame_type != MI355_FDD)
      return MI355_ERROR_INVALID_INPUTS;
  }
  std::lock_guard<std::mutex> lock(q->mu);
  CHECK_HIP(hipSetDevice(q->device));
  CHECK_HIP(hipDeviceSynchronize()); // nothing may still read the sequences that are replaced
  q->cells.clear();
  const int r = build_sequences(q, cells, n);
  if (r == MI355_SUCCESS) q->cells.assign(cells, cells + n);
  return r;
}

int mi355_cell_meas_sequence(mi355_cell_meas_t* q, uint32_t cell, uint32_t sf_idx, float* host_out)
{
  if (!q || !host_out || sf_idx > 9) return MI355_ERROR_INVALID_INPUTS;
  std::lock_guard<std::mutex> lock(q->mu);
  if (cell >= q->cells.size()) return MI355_ERROR_INVALID_INPUTS;
  CHECK_HIP(hipSetDevice(q->device));
  CHECK_HIP(hipMemcpy(host_out, q->d_seq.as<float2>() + ((size_t)cell * 10 + sf_idx) * q->sf_len,
                      (size_t)q->sf_len * sizeof(float2), hipMemcpyDeviceToHost));
  return MI355_SUCCESS;
}

int mi355_cell_meas_run_batch(mi355_cell_meas_t* q, const mi355_cell_meas_job_t* jobs, uint32_t njobs,
                              mi355_cell_meas_res_t* res, mi355_cell_meas_sf_t* sf_out, void* stream)
{
  if (!q || (njobs && (!jobs || !res))) return MI355_ERROR_INVALID_INPUTS;
  if (!njobs) return MI355_SUCCESS;
  std::lock_guard<std::mutex> lock(q->mu);
  CHECK_HIP(hipSetDevice(q->device));
  return run(q, jobs, njobs, true, res, sf_out, stream ? (hipStream_t)stream : q->own);
}

int mi355_cell_meas_find_peak_batch(mi355_cell_meas_t* q, const mi355_cell_meas_job_t* jobs, uint32_t njobs,
                                    mi355_cell_meas_res_t* res, void* stream)
{
  if (!q || (njobs && (!jobs || !res))) return MI355_ERROR_INVALID_INPUTS;
  if (!njobs) return MI355_SUCCESS;
  std::lock_guard<std::mutex> lock(q->mu);
  CHECK_HIP(hipSetDevice(q->device));
  return run(q, jobs, njobs, false, res, nullptr, stream ? (hipStream_t)stream : q->own);
}

int mi355_cell_meas_measure_sf_batch(mi355_cell_meas_t* q, const mi355_cell_meas_sf_job_t* jobs, uint32_t njobs,
                                     mi355_cell_meas_sf_t* out, void* stream)
{
  if (!q || (njobs && (!jobs || !out))) return MI355_ERROR_INVALID_INPUTS;
  if (!njobs) return MI355_SUCCESS;
  std::lock_guard<std::mutex> lock(q->mu);
  for (uint32_t i = 0; i < njobs; i++)
    if (!jobs[i].input || jobs[i].cell >= q->cells.size()) return MI355_ERROR_INVALID_INPUTS;
  CHECK_HIP(hipSetDevice(q->device));
  hipStream_t  s      = stream ? (hipStream_t)stream : q->own;
  const size_t b_jobs = staged_size((size_t)njobs * sizeof(CmSfJobDev));
  const size_t b_out  = staged_size((size_t)njobs * sizeof(mi355_cell_meas_sf_t));
  CHECK_HIP(q->d_buf.reserve(b_jobs + b_out, b_jobs + b_out, DevScratch::SyncFree));
  char* base = q->d_buf.base();
  CHECK_HIP(q->st.reserve(b_jobs));
  auto* pj = (CmSfJobDev*)q->st.slot((size_t)njobs * sizeof(CmSfJobDev));
  for (uint32_t i = 0; i < njobs; i++) pj[i] = CmSfJobDev{(const float2*)jobs[i].input, jobs[i].cell, jobs[i].sf_idx};
  CHECK_HIP(q->st.upload(base, s));
  const CmArgs a     = base_args(q);
  auto*        d_out = (mi355_cell_meas_sf_t*)(base + b_jobs);
  const size_t bytes = (size_t)njobs * sizeof(mi355_cell_meas_sf_t);
  hipError_t   e     = q->back.reserve(bytes);
  if (e == hipSuccess) e = cm_launch_measure_sf(a, (const CmSfJobDev*)base, njobs, d_out, s);
  if (e == hipSuccess) e = stage_copy(q->back.host, d_out, bytes, s);
  const hipError_t w = wait_stream(s);
  CHECK_HIP(e);
  CHECK_HIP(w);
  memcpy(out, q->back.host, bytes);
  return MI355_SUCCESS;
}

} // extern "C"
