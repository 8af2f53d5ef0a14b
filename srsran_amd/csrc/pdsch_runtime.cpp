// srsran_amd/csrc/pdsch_runtime.cpp -- host runtime behind include/srsran_amd/pdsch.h.
//
// A batch of srslte_pdsch_decode calls (pdsch.c:907-1072) runs as
//   kernel A (RE gather + rho_b + equaliser + layer demap + CSI max)   one launch for the whole batch
//   kernel B (demapper + descrambler + CSI weighting)                  one launch for every codeword
//   DL-SCH batch decode (dlsch_runtime.cpp)                            rate dematch, turbo, CRCs
// The host only plans: extraction maps are built once per (grant allocation, cfi, subframe) and cached in
// HBM (pdsch_maps.cpp), job / codeword descriptors and block tables are uploaded with one copy each
// (pdsch_frontend.cpp).  Here: create / destroy, the setters and debug entry points, the planning of one job, and the
// decode: plan jobs, plan pdsch_eq_rm (pdsch_eqrm.cpp), front end, group the TBs by iteration count, decode the groups.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <stdio.h>
#include <vector>

#include "host_env.h"
#include "lte_common.h"
#include "pdsch_object.h"
#include "pdsch_plan.h"
#include "pdsch_re_map.h"

using namespace mi355;

// host planning of one job; returns <0 when srslte_pdsch_decode would fail before decoding
static int plan_job(mi355_pdsch_t* q, const mi355_pdsch_job_t& j, const mi355_pdsch_res_t* res, JobPlan& P)
{
  const mi355_pdsch_cfg_t&   cfg = j.cfg;
  const mi355_pdsch_grant_t& g   = cfg.grant;
  const mi355_cell_t&        c   = q->cell;
  PdschJobDev&               D   = P.dev;
  const uint32_t sch = g.tx_scheme, L = g.nof_layers, np = c.nof_ports, nrx = q->nof_rx;
  uint32_t       cb  = 0;
  int            rr  = pdsch_admit(j.sf.cfi, sch, np, nrx, L, g.nof_tb, g.pmi, &cb);
  if (rr) return rr;
  for (uint32_t r = 0; r < nrx; r++) {
    if (!j.sf_symbols[r]) return MI355_ERROR_INVALID_INPUTS;
    for (uint32_t p = 0; p < np; p++)
      if (!j.ce[p][r]) return MI355_ERROR_INVALID_INPUTS;
  }
  MapEntry me;
  if ((rr = get_map(q, g, j.sf.cfi, j.sf.tti % 10, &me))) return rr;
  const uint32_t nre = me.n;
  D.map              = me.d;
  D.imap             = me.inv();
  D.g0               = me.g0;
  D.cols             = me.cols();
  D.ncols            = me.ncols;
  if (nre != g.nof_re) return MI355_ERROR; // "Error expecting %d symbols but got %d" (pdsch.c:949-960)
  PdschPower pw;
  if ((rr = pdsch_power(cfg, np, c.cp, g.nof_symb_slot[0] ? g.nof_symb_slot[0] : nsymb_of(c), &pw))) return rr;
  for (uint32_t r = 0; r < nrx; r++) {
    D.y[r] = (const float2*)j.sf_symbols[r];
    for (uint32_t p = 0; p < np; p++) D.h[p][r] = (const float2*)j.ce[p][r];
  }
  D.nof_re     = nre;
  D.nof_rx     = nrx;
  D.nof_ports  = np;
  D.nof_layers = L;
  D.scheme     = sch;
  D.cb         = cb;
  D.row        = 12 * c.nof_prb;
  D.row_magic  = (uint32_t)((1ull << 32) / D.row + 1);
  D.rhob_mask  = pw.rhob_mask;
  D.rhob_inv   = pw.rhob_inv;
  D.scaling    = pw.scaling;
  D.noise      = cfg.decoder_type == MI355_MIMO_DECODER_ZF ? 0.0f : j.noise_estimate;
  // single-RE schemes walk the grid span of the allocation (inverse map), SFBC the RE pairs / quads
  D.units      = sch == MI355_TXSCHEME_DIVERSITY ? (np == 2 ? (nre + 1) / 2 : (nre + 3) / 4) : me.g1 - me.g0;
  for (uint32_t t = 0; t < 2; t++) {
    const mi355_ra_tb_t& tb = g.tb[t];
    P.decode[t]             = tb.enabled && !(res && res[t].crc);
    if (!P.decode[t]) continue;
    P.cw_of_tb[t] = tb.cw_idx;
    if (tb.cw_idx > 1 || mod_bits(tb.mod) == 0 || tb.nof_bits != nre * mod_bits(tb.mod) ||
        tb.nof_bits > PDSCH_GOLD_MAX || cfg.softbuffer[t] == UINT32_MAX || !j.payload[t])
      return MI355_ERROR_INVALID_INPUTS;
  }
  return MI355_SUCCESS;
}

// trim_maps, then plan_job for every job (res: nullable, 2 per job; d_noise: nullable) and the row-invariant
// estimates' consequences (mi355_pdsch_set_ce_invariant): row 0 read, and the fused equaliser where the csi depends on
// the subcarrier only (CDD alternates its precoder per RE, SFBC pairs REs)
static int plan_jobs(mi355_pdsch_t* q, const mi355_pdsch_job_t* jobs, const mi355_pdsch_res_t* res, const float* d_noise,
                     bool ce_invariant, std::vector<JobPlan>& plans)
{
  int r = trim_maps(q);
  if (r) return r;
  for (size_t i = 0; i < plans.size(); i++) {
    JobPlan& P = plans[i];
    if ((r = plan_job(q, jobs[i], res ? &res[2 * i] : nullptr, P))) return r;
    // noise estimate left in device memory by the channel estimator (ZF ignores it, pdsch.c:934)
    if (d_noise && jobs[i].cfg.decoder_type != MI355_MIMO_DECODER_ZF) P.dev.noise_dev = d_noise + i;
    P.dev.h_invariant = ce_invariant ? 1u : 0u;
    P.dev.fused       = !q->llr8 && ce_invariant &&
                          (P.dev.scheme == MI355_TXSCHEME_PORT0 || P.dev.scheme == MI355_TXSCHEME_SPATIALMUX) ? 1u : 0u;
  }
  return MI355_SUCCESS;
}

extern "C" {

uint32_t mi355_pdsch_re_map(const mi355_cell_t* cell, const mi355_pdsch_grant_t* grant, uint32_t cfi, uint32_t sf_idx,
                            uint32_t* idx)
{
  if (!cell || !grant || cell->nof_prb == 0 || cell->nof_prb > MI355_MAX_PRB) return 0;
  return walk_map(*cell, *grant, cfi, sf_idx % 10, [&](uint32_t k, uint32_t p) {
    if (idx) idx[k] = p;
  });
}

int mi355_pdsch_create(mi355_pdsch_t** q, const mi355_cell_t* cell, uint32_t nof_rx_antennas, int device)
{
  if (!q || !cell || cell->nof_prb == 0 || cell->nof_prb > MI355_MAX_PRB || nof_rx_antennas == 0 ||
      nof_rx_antennas > MI355_MAX_RX_ANT || !(cell->nof_ports == 1 || cell->nof_ports == 2 || cell->nof_ports == 4))
    return MI355_ERROR_INVALID_INPUTS;
  CHECK_HIP(hipSetDevice(device));
  auto* d   = new mi355_pdsch;
  d->device = device;
  d->cell   = *cell;
  d->nof_rx = nof_rx_antennas;
  const std::vector<uint32_t> g = gold_table(PDSCH_GOLD_MAX);
  if (hipStreamCreateWithFlags(&d->own, hipStreamNonBlocking) != hipSuccess ||
      mi355_dlsch_create(&d->dlsch, device) != MI355_SUCCESS ||
      d->gold.upload(g) != hipSuccess) {
    mi355_pdsch_destroy(d);
    return MI355_ERROR;
  }
  *q = d;
  return MI355_SUCCESS;
}

void mi355_pdsch_destroy(mi355_pdsch_t* q)
{
  if (!q) return;
  (void)hipSetDevice(q->device);
  (void)hipDeviceSynchronize();
  if (q->fe_done) (void)hipEventDestroy(q->fe_done);
  mi355_dlsch_destroy(q->dlsch);
  if (q->own) (void)hipStreamDestroy(q->own);
  delete q;
}

mi355_dlsch_t* mi355_pdsch_dlsch(mi355_pdsch_t* q) { return q ? q->dlsch : nullptr; }

int mi355_pdsch_set_llr_8bit(mi355_pdsch_t* q, int enable)
{
  if (!q) return MI355_ERROR_INVALID_INPUTS;
  std::lock_guard<std::mutex> lk(q->mu);
  q->llr8 = enable != 0;
  return MI355_SUCCESS;
}

int mi355_pdsch_set_ce_invariant(mi355_pdsch_t* q, int enable)
{
  if (!q) return MI355_ERROR_INVALID_INPUTS;
  std::lock_guard<std::mutex> lk(q->mu);
  q->ce_inv = enable != 0;
  return MI355_SUCCESS;
}

int mi355_pdsch_frontend(mi355_pdsch_t* q, const mi355_pdsch_job_t* jobs, uint32_t njobs, void* stream)
{
  if (!q || (njobs && !jobs)) return MI355_ERROR_INVALID_INPUTS;
  std::lock_guard<std::mutex> lock(q->mu);
  CHECK_HIP(hipSetDevice(q->device));
  hipStream_t          s = stream ? (hipStream_t)stream : q->own;
  std::vector<JobPlan> plans(njobs);
  int                  r = plan_jobs(q, jobs, nullptr, nullptr, q->ce_inv, plans);
  if (r || (r = run_frontend(q, jobs, plans, s))) return r;
  CHECK_HIP(wait_stream(s));
  q->last = plans;
  return MI355_SUCCESS;
}

int mi355_pdsch_debug_stage(mi355_pdsch_t* q, uint32_t job, uint32_t cw, const float** d, const float** csi,
                            const int16_t** e)
{
  if (!q || job >= q->last.size() || cw > 1) return MI355_ERROR_INVALID_INPUTS;
  if (q->e_pending) { // (debug path) the LLRs of the last batch, which pdsch_eq_rm kept in LDS only
    CHECK_HIP(hipSetDevice(q->device));
    CHECK_HIP(hipDeviceSynchronize()); // (the batch's stream may be the caller's, gone by now)
    CHECK_HIP(pdsch_launch_fused(q->last_jobs_dev, q->last_njobs, q->last_max_fpairs, q->last_fkeys.data(),
                                 (uint32_t)q->last_fkeys.size(), q->own));
    CHECK_HIP(hipStreamSynchronize(q->own));
    q->e_pending = false;
  }
  const JobPlan& P = q->last[job];
  if (d) *d = (const float*)(q->d_arena + P.d_off[cw]);
  if (csi) *csi = q->csi_arena + P.d_off[cw];
  if (e) {
    *e = nullptr;
    for (uint32_t t = 0; t < 2; t++)
      if (P.decode[t] && P.cw_of_tb[t] == cw)
        *e = q->llr8 ? (const int16_t*)((const int8_t*)q->e_arena + P.e_off[t]) : q->e_arena + P.e_off[t];
  }
  return MI355_SUCCESS;
}

int mi355_pdsch_debug_set_cache_limits(mi355_pdsch_t* q, uint32_t max_maps, uint32_t max_scr)
{
  if (!q) return MI355_ERROR_INVALID_INPUTS;
  std::lock_guard<std::mutex> lk(q->mu);
  if (max_maps) q->max_maps = max_maps;
  if (max_scr) q->max_scr = max_scr;
  return MI355_SUCCESS;
}

int mi355_pdsch_debug_job_map(mi355_pdsch_t* q, uint32_t job, const uint16_t** d_map, uint32_t* n)
{
  if (!q || job >= q->last.size() || !d_map || !n) return MI355_ERROR_INVALID_INPUTS;
  *d_map = q->last[job].dev.map;
  *n     = q->last[job].dev.nof_re;
  return MI355_SUCCESS;
}

int mi355_pdsch_decode_batch(mi355_pdsch_t*           q,
                             mi355_softbuffer_pool_t* pool,
                             const mi355_pdsch_job_t* jobs,
                             uint32_t                 njobs,
                             mi355_pdsch_res_t*       res,
                             void*                    stream)
{
  return mi355::pdsch_decode_batch_dev_noise(q, pool, jobs, njobs, res, stream, nullptr, mi355::WaitHook{},
                                             q && q->ce_inv);
}

int mi355_pdsch_decode_launch(mi355_pdsch_t* q, mi355_softbuffer_pool_t* pool, const mi355_pdsch_job_t* jobs,
                              uint32_t njobs, mi355_pdsch_res_t* res, void* stream)
{
  if (!q) return MI355_ERROR_INVALID_INPUTS;
  if (q->api_armed) return MI355_ERROR; // the previous launch was not collected
  if (!q->api_pend) q->api_pend.reset(new mi355::PdschPending);
  const int r = mi355::pdsch_decode_batch_dev_noise(q, pool, jobs, njobs, res, stream, nullptr, mi355::WaitHook{},
                                                    q->ce_inv, q->api_pend.get());
  q->api_armed = true; // collected even after an error (whatever groups were enqueued)
  return r;
}

int mi355_pdsch_decode_collect(mi355_pdsch_t* q)
{
  if (!q) return MI355_ERROR_INVALID_INPUTS;
  if (!q->api_armed) return MI355_SUCCESS;
  q->api_armed = false;
  return q->api_pend->collect();
}

} // extern "C"

// srslte_pdsch_codeword_decode's result fields (pdsch.c:862-871) from one DL-SCH batch's per-TB returns
static void fill_results(mi355_pdsch_res_t* res, const std::vector<std::pair<uint32_t, uint32_t>>& who,
                         const std::vector<int32_t>& ret, const std::vector<float>& avg)
{
  for (size_t k = 0; k < who.size(); k++) {
    mi355_pdsch_res_t& o   = res[2 * who[k].first + who[k].second];
    o.crc                  = ret[k] == 0;
    o.ret                  = ret[k] == MI355_ERROR_INVALID_INPUTS ? MI355_ERROR : MI355_SUCCESS;
    o.avg_iterations_block = avg[k];
  }
}

// DL-SCH: one batch per max-iterations setting (srslte_sch_set_max_noi persists across jobs and calls,
// pdsch.c:930-932), decoded in ascending order of the setting
struct ItsGroup {
  std::vector<std::pair<uint32_t, uint32_t>> who; // (job, tb)
  std::vector<mi355_dlsch_tb_t>              tbs;
};

static void group_tbs(mi355_pdsch_t* q, const mi355_pdsch_job_t* jobs, uint32_t njobs, const std::vector<JobPlan>& plan,
                      std::map<uint32_t, ItsGroup>& groups)
{
  for (uint32_t i = 0; i < njobs; i++) {
    const mi355_pdsch_cfg_t& cfg = jobs[i].cfg;
    if (cfg.max_nof_iterations) q->max_its = cfg.max_nof_iterations;
    for (uint32_t t = 0; t < 2; t++) {
      if (!plan[i].decode[t]) continue;
      const mi355_ra_tb_t& tb = cfg.grant.tb[t];
      const uint32_t       Nl = cfg.grant.nof_layers != cfg.grant.nof_tb ? 2 : 1; // sch.c:584-588
      mi355_dlsch_tb_t     d{};
      d.tbs         = (uint32_t)std::max(0, tb.tbs);
      d.nof_e_bits  = tb.nof_bits;
      d.Qm          = mod_bits(tb.mod) * Nl;
      d.rv          = tb.rv;
      d.softbuffer  = cfg.softbuffer[t];
      d.e_offset    = plan[i].e_off[t];
      d.data_offset = (uint64_t)(uintptr_t)jobs[i].payload[t]; // absolute (d_data == NULL)
      groups[q->max_its].who.push_back({i, t});
      groups[q->max_its].tbs.push_back(d);
    }
  }
}

// pend: the results stay in flight, the arrays live in the pending object until collect(); else res is filled here.
// The hook goes to the first group only.
static int decode_groups(mi355_pdsch_t* q, mi355_softbuffer_pool_t* pool, std::map<uint32_t, ItsGroup>& groups,
                         mi355_pdsch_res_t* res, hipStream_t s, WaitHook hook, PdschPending* pend, bool after_s, bool eqrm)
{
  if (pend) {
    pend->used = 0;
    pend->res  = res;
  }
  for (auto& kv : groups) {
    ItsGroup&            G = kv.second;
    std::vector<int32_t> ret_local, *ret = &ret_local;
    std::vector<float>   avg_local, *avg = &avg_local;
    DlschPending*        dp = nullptr;
    if (pend) {
      const uint32_t g = pend->used; // counted once its decode is enqueued
      if (pend->groups.size() <= g) {
        pend->groups.emplace_back(new DlschPending);
        pend->ret.emplace_back();
        pend->avg.emplace_back();
        pend->who.emplace_back();
      }
      dp = pend->groups[g].get(), ret = &pend->ret[g], avg = &pend->avg[g];
      pend->who[g] = G.who;
    }
    ret->assign(G.tbs.size(), 0);
    avg->assign(G.tbs.size(), 0.f);
    int r = mi355_dlsch_set_max_iterations(q->dlsch, kv.first);
    if (r) return r;
    // with results left in flight, a later iteration-count batch shares the DL-SCH descriptor scratch with the
    // earlier ones still queued on s: its upload waits for their epilogue (done_ev)
    const bool after = after_s || (pend && pend->used > 0);
    r = dlsch_decode_dev_hook(q->dlsch, pool, q->e_arena, G.tbs.data(), (uint32_t)G.tbs.size(), nullptr, ret->data(),
                              avg->data(), s, hook, q->llr8, dp, after, eqrm);
    hook = WaitHook{}; // once
    if (r) return r;
    if (pend)
      pend->used++;
    else
      fill_results(res, G.who, *ret, *avg);
  }
  return MI355_SUCCESS;
}

int mi355::pdsch_decode_batch_dev_noise(mi355_pdsch_t* q, mi355_softbuffer_pool_t* pool, const mi355_pdsch_job_t* jobs,
                                        uint32_t njobs, mi355_pdsch_res_t* res, void* stream, const float* d_noise,
                                        WaitHook hook, bool ce_invariant, PdschPending* pend, bool after_s)
{
  if (!q || !pool || !res || (njobs && !jobs)) return MI355_ERROR_INVALID_INPUTS;
  std::lock_guard<std::mutex> lock(q->mu);
  const HostTime t0 = host_now();
  CHECK_HIP(hipSetDevice(q->device));
  hipStream_t          s = stream ? (hipStream_t)stream : q->own;
  std::vector<JobPlan> plans(njobs);
  int                  r = plan_jobs(q, jobs, res, d_noise, ce_invariant, plans);
  if (r) return r;
  EqRmPlan       er;
  const bool     eqrm = plan_eq_rm(q, pool, jobs, plans, er);
  const HostTime t1   = host_now();
  if ((r = run_frontend(q, jobs, plans, s, after_s, eqrm ? &er : nullptr))) return r;
  if (env_host_prof()) {
    fprintf(stderr, "[mi355 host] pdsch: plan %.1f us, frontend launch %.1f us\n", host_us(t0, t1),
            host_us(t1, host_now()));
  }
  q->last.swap(plans);
  std::map<uint32_t, ItsGroup> groups;
  group_tbs(q, jobs, njobs, q->last, groups);
  return decode_groups(q, pool, groups, res, s, hook, pend, after_s, eqrm);
}

int mi355::PdschPending::collect()
{
  int r = MI355_SUCCESS;
  for (uint32_t g = 0; g < used; g++) {
    const int e = groups[g]->collect();
    if (e) {
      r = e;
      continue;
    }
    fill_results(res, who[g], ret[g], avg[g]);
  }
  used = 0;
  return r;
}
