// srsran_amd/csrc/pdsch_eqrm.cpp -- host plan of pdsch_eq_rm (pdsch_internal.h): which batches take it (the job-shape
// rule is pdsch_plan.h's), the DL-SCH's rate-dematching tables of their code blocks, and its phase counters.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <mutex>

#include "host_env.h"
#include "pdsch_object.h"
#include "pdsch_plan.h"

using namespace mi355;

namespace {
std::atomic<unsigned long long*> g_eqrm_prof{nullptr};
unsigned long long*              g_eqrm_prof_mem = nullptr;
std::mutex                       g_eqrm_prof_mu;
} // namespace

// measurement: enable = 1 arms pdsch_eq_rm's phase counters (zeroed), 0 disarms; out (nullable, 4 u64): workgroups and
// the sums of their prologue, equaliser and rate-dematching shader cycles since arming (include/srsran_amd/pdsch.h)
extern "C" int mi355_pdsch_eqrm_profile(int enable, uint64_t* out)
{
  std::lock_guard<std::mutex> lk(g_eqrm_prof_mu);
  if (out && g_eqrm_prof.load()) {
    if (hipDeviceSynchronize() != hipSuccess) return MI355_ERROR;
    if (hipMemcpy(out, g_eqrm_prof_mem, 4 * 8, hipMemcpyDeviceToHost) != hipSuccess) return MI355_ERROR;
  }
  if (enable) {
    if (!g_eqrm_prof_mem && hipMalloc(&g_eqrm_prof_mem, 4 * 8) != hipSuccess) return MI355_ERROR;
    if (hipMemset(g_eqrm_prof_mem, 0, 4 * 8) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return MI355_ERROR;
    g_eqrm_prof.store(g_eqrm_prof_mem);
  } else {
    g_eqrm_prof.store(nullptr);
  }
  return MI355_SUCCESS;
}

// pdsch_eq_rm for the whole batch when every job qualifies: fused (port 0 / spatial multiplexing, row-invariant
// estimates), 16-bit LLRs, and the job shape of eqrm_job_shape (pdsch_plan.h).  MI355_NO_EQRM (A/B, tests): never.
bool mi355::plan_eq_rm(mi355_pdsch_t* q, mi355_softbuffer_pool_t* pool, const mi355_pdsch_job_t* jobs,
                       const std::vector<JobPlan>& plans, EqRmPlan& er)
{
  if (env_no_eqrm() || q->llr8 || !pool || plans.empty()) return false;
  const SoftbufferView v = softbuffer_view(pool);
  er.rj.assign(plans.size(), EqRmJob{});
  er.max_c = er.img = er.cimg = 0;
  const bool compact = env_eqrm_compact() && rm_sparse_writes();
  struct CKey {
    uint32_t        key = UINT32_MAX, E = 0, nq = 0, qoff = 0;
    const uint16_t* tab = nullptr;
  } ck[4]; // the last compact tables looked up (a batch has few (K, rv, E))
  // a batch has few distinct TB sizes and (K, rv): segmentation and table look-ups of the previous TB are reused
  SegCache        seg;
  uint32_t        tab_key[2] = {UINT32_MAX, UINT32_MAX};
  const uint16_t* tab[2]     = {nullptr, nullptr};
  auto inv_of = [&](uint32_t K, uint32_t rv, const uint16_t** out) {
    const uint32_t key = K << 2 | rv;
    for (int k = 0; k < 2; k++)
      if (tab_key[k] == key) return *out = tab[k], 0;
    const int e = dlsch_rm_inv(q->dlsch, K, rv, out);
    tab_key[1] = tab_key[0], tab[1] = tab[0], tab_key[0] = key, tab[0] = *out;
    return e;
  };
  for (size_t i = 0; i < plans.size(); i++) {
    const JobPlan&           P   = plans[i];
    const mi355_pdsch_cfg_t& cfg = jobs[i].cfg;
    if (!P.dev.fused) return false;
    EqRmTb tbs[2];
    for (uint32_t t = 0; t < 2; t++) {
      const mi355_ra_tb_t& tb = cfg.grant.tb[t];
      tbs[t] = EqRmTb{tb.tbs, tb.nof_bits, mod_bits(tb.mod), tb.rv, cfg.softbuffer[t]};
    }
    EqRmShape S;
    if (!eqrm_job_shape(tbs, P.decode, v.max_cb, v.nof_sb, seg, &S)) return false;
    EqRmJob& R    = er.rj[i];
    uint32_t cimg = 0;
    R.C = S.C, R.Qm = S.Qm, R.Gp = S.Gp;
    for (uint32_t t = 0; t < 2; t++) {
      if (!P.decode[t]) continue;
      EqRmLayer& L = R.layer[P.cw_of_tb[t] & 1];
      L.C1         = S.C1;
      L.slot0      = tbs[t].softbuffer * v.max_cb;
      for (uint32_t kx = 0; kx < 2; kx++) {
        const uint32_t K = kx ? S.K2 : S.K1;
        if (!S.used[kx]) continue;
        if (inv_of(K, tbs[t].rv, &L.inv[kx])) return false;
        L.N[kx]      = 3 * K + 12;
        L.buflen[kx] = dlsch_rm_buflen(K);
      }
      if (!compact || &L != &R.layer[0]) continue;
      for (uint32_t kx = 0; kx < 2; kx++) {
        const uint32_t K = kx ? S.K2 : S.K1;
        for (uint32_t ev = 0; ev < (S.used[kx] ? S.nE : 0); ev++) {
          const uint32_t E = S.E[ev], key = K << 2 | tbs[t].rv;
          CKey*          hit = nullptr;
          for (auto& c : ck)
            if (c.key == key && c.E == E) hit = &c;
          if (!hit) {
            for (int k = 3; k > 0; k--) ck[k] = ck[k - 1];
            hit = &ck[0];
            if (dlsch_rm_compact(q->dlsch, K, tbs[t].rv, E, &hit->tab, &hit->nq, &hit->qoff)) return false;
            hit->key = key, hit->E = E;
          }
          R.cmp[kx][ev] = hit->tab, R.cnq[kx][ev] = hit->nq, R.cqoff[kx][ev] = hit->qoff;
          cimg          = std::max(cimg, 8 * hit->nq);
        }
      }
    }
    // the compact image serves two layers only (pdsch_eq_rm's cm: both fresh, one table): a one-layer job (SISO,
    // transmit diversity, a single TB) keeps the circular-order image, and its compact size must not set the
    // workgroup's LDS -- at QPSK K = 5312 it is 1.8x the circular image and halved the occupancy (SISO -9 %, r06u)
    if (S.nt < 2) {
      for (auto& row : R.cmp) row[0] = row[1] = nullptr;
    } else {
      er.cimg = std::max(er.cimg, cimg);
    }
    er.max_c = std::max(er.max_c, R.C);
    er.img   = std::max(er.img, S.n_max);
  }
  er.pool      = EqRmPool{v.buf, v.stride, v.cb_crc, v.fresh, rm_sparse_writes() ? 1 : 0};
  er.pool.diag = env_eqrm_diag();
  er.pool.prof = g_eqrm_prof.load();
  return er.max_c > 0;
}
