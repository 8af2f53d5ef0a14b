// srsran_amd/csrc/pdsch_frontend.cpp -- the PDSCH front end of one call over planned jobs, as named steps over one
// call struct: codeword descriptors and arena offsets, the device scratch (FrontLayout, pdsch_plan.h), the device
// pointers, one upload, and the launches
//   equalize -> scr_pack -> eq_rm | fused -> llr                       (pdsch_kernels.hip)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <stdio.h>
#include <vector>

#include "host_env.h"
#include "pdsch_object.h"
#include "pdsch_plan.h"

using namespace mi355;

namespace {

struct FrontCall {
  mi355_pdsch_t*           q;
  const mi355_pdsch_job_t* jobs;
  std::vector<JobPlan>&    plans;
  hipStream_t              s;
  bool                     after_s;
  const EqRmPlan*          er;
  uint32_t                 njobs;
  size_t                   nd = 0, ne = 0, nwt = 0; // elements of d / csi and of e, bytes of wtab
  uint32_t                 max_units = 0, max_pairs = 0, max_fpairs = 0, nparts = 0;
  std::vector<PdschCwDev>  cws;
  std::vector<uint32_t>    new_ci; // descrambling sequences to generate: c_init and destination
  std::vector<uint32_t*>   new_dst;
  std::vector<PdschJobDev> hj;
  std::vector<uint32_t>    fkeys; // (qm0, qm1) pairs of the fused jobs: one kernel instantiation each
  FrontLayout              lay{};
  char*                    base = nullptr;
  template <class T> const T* dev(size_t off) const { return (const T*)(base + off); }
};

// eq_rm's two-layer jobs: the per-subcarrier MMSE matrices (PdschJobDev.wtab)
size_t wtab_bytes(const FrontCall& c, const JobPlan& P)
{
  const bool two = c.er && P.dev.fused && P.dev.nof_layers == 2 && P.decode[0] && P.decode[1];
  return two ? ((size_t)P.dev.row * 48 + 255) / 256 * 256 : 0;
}

// step 1: arena offsets of every job, and the codewords to decode with their descrambling sequences
int collect_codewords(FrontCall& c)
{
  mi355_pdsch_t*  q        = c.q;
  uint32_t        last_ci  = 0;
  const uint32_t* last_scr = nullptr;
  int             r        = trim_scr(q, c.s);
  if (r) return r;
  c.cws.reserve(2 * c.njobs);
  for (uint32_t i = 0; i < c.njobs; i++) {
    JobPlan& P = c.plans[i];
    for (uint32_t cw = 0; cw < 2; cw++) {
      P.d_off[cw] = c.nd;
      c.nd += (P.dev.nof_re + 63) / 64 * 64;
    }
    if (P.dev.fused) {
      c.max_fpairs = std::max(c.max_fpairs, (P.dev.nof_re + 1) / 2);
    } else {
      c.max_units = std::max(c.max_units, P.dev.units);
    }
    c.nwt += wtab_bytes(c, P);
    for (uint32_t t = 0; t < 2; t++) {
      if (!P.decode[t]) continue;
      const mi355_ra_tb_t& tb = c.jobs[i].cfg.grant.tb[t];
      P.e_off[t]              = c.ne;
      c.ne += (tb.nof_bits + 63) / 64 * 64;
      PdschCwDev w{};
      w.nof_re     = P.dev.nof_re;
      w.nof_bits   = tb.nof_bits;
      w.qm         = mod_bits(tb.mod);
      w.c_init     = pdsch_c_init(c.jobs[i].cfg.rnti, tb.cw_idx, c.jobs[i].sf.tti, q->cell.id);
      w.csi_enable = c.jobs[i].cfg.csi_enable ? 1u : 0u;
      w.pairs      = (w.nof_re + 1) / 2;
      w.fused      = P.dev.fused;
      if (!w.fused) c.max_pairs = std::max(c.max_pairs, w.pairs);
      if (w.c_init != last_ci || !last_scr) {
        uint32_t* d     = nullptr;
        bool      fresh = false; // filled by pdsch_launch_scr_pack below
        if ((r = get_scr(q, w.c_init, &d, &fresh))) return r;
        if (fresh) {
          c.new_ci.push_back(w.c_init);
          c.new_dst.push_back(d);
        }
        last_ci  = w.c_init;
        last_scr = d;
      }
      w.scr = last_scr;
      c.cws.push_back(w);
    }
  }
  c.nparts = (c.max_units + EQ_BLOCK_ITEMS - 1) / EQ_BLOCK_ITEMS; // equaliser blocks per job
  return MI355_SUCCESS;
}

// step 2: the layout, the device scratch and the pinned staging behind its staged part
int reserve_scratch(FrontCall& c)
{
  mi355_pdsch_t* q = c.q;
  c.lay = front_layout(c.njobs, c.cws.size(), c.new_ci.size(), c.nd, c.ne, c.nparts, c.nwt, c.er != nullptr,
                       sizeof(PdschJobDev), sizeof(PdschCwDev), sizeof(EqRmJob));
  // the old scratch may still be read by this object's batch in flight: retired, not freed (no device-wide wait)
  CHECK_HIP(q->scratch.reserve(c.lay.total, c.lay.total + c.lay.total / 4 + 4096, DevScratch::Retire));
  c.base       = q->scratch.base();
  q->d_arena   = (float2*)(c.base + c.lay.d);
  q->csi_arena = (float*)(c.base + c.lay.csi);
  q->e_arena   = (int16_t*)(c.base + c.lay.e);
  CHECK_HIP(q->stage.reserve(c.lay.staged));
  return MI355_SUCCESS;
}

// step 3: every device pointer of the job descriptors and of their codewords', in one pass (codewords in job order)
void patch_pointers(FrontCall& c)
{
  mi355_pdsch_t* q      = c.q;
  uint32_t*      d_cmax = (uint32_t*)(c.base + c.lay.cmax);
  uint32_t*      d_cfin = (uint32_t*)(c.base + c.lay.cfin);
  char*          d_wt   = c.base + c.lay.wtab;
  size_t         k      = 0;
  c.hj.resize(c.njobs);
  for (uint32_t i = 0; i < c.njobs; i++) {
    JobPlan& P        = c.plans[i];
    uint32_t qm[2]    = {0, 0};
    P.dev.cw[0]       = P.dev.cw[1] = nullptr;
    P.dev.cmax        = d_cmax + (size_t)2 * c.nparts * i;
    P.dev.cmax_stride = c.nparts;
    P.dev.wtab        = wtab_bytes(c, P) ? (float4*)d_wt : nullptr;
    d_wt += wtab_bytes(c, P);
    for (uint32_t cw = 0; cw < 2; cw++) {
      P.dev.d[cw]   = q->d_arena + P.d_off[cw];
      P.dev.csi[cw] = q->csi_arena + P.d_off[cw];
    }
    for (uint32_t t = 0; t < 2; t++) {
      if (!P.decode[t]) continue;
      const uint32_t cw = P.cw_of_tb[t];
      PdschCwDev&    w  = c.cws[k];
      P.dev.cw[cw & 1]  = c.dev<PdschCwDev>(c.lay.cws) + k; // the layer (codeword) feeding this TB
      qm[cw & 1]        = w.qm;
      w.d               = P.dev.d[cw];
      w.csi             = P.dev.csi[cw];
      w.cmax            = P.dev.cmax + (size_t)cw * c.nparts;
      w.nparts          = (P.dev.units + EQ_BLOCK_ITEMS - 1) / EQ_BLOCK_ITEMS;
      w.cmax_final      = d_cfin + k;
      w.e               = q->e_arena + P.e_off[t];
      if (q->llr8) {
        w.llr8  = 1;
        w.e8    = (int8_t*)q->e_arena + P.e_off[t];
        w.k8[0] = (float)(-20 * M_SQRT2);
        w.k8[1] = 2 * 30 / sqrtf(10);
        w.k8[2] = 8.0f / sqrtf(170.0f);
        w.k8[3] = 4.0f / sqrtf(170.0f);
        w.k8[4] = 2.0f / sqrtf(170.0f);
      }
      k++;
    }
    P.dev.fused_key = qm[0] * 16 + qm[1];
    if (P.dev.fused && std::find(c.fkeys.begin(), c.fkeys.end(), P.dev.fused_key) == c.fkeys.end())
      c.fkeys.push_back(P.dev.fused_key);
    c.hj[i] = P.dev;
  }
}

// step 4: the staged part in FrontLayout's order, and its one upload
int stage_and_upload(FrontCall& c, HostTime* t_put)
{
  mi355_pdsch_t* q = c.q;
  q->stage.put(c.hj.data(), c.njobs * sizeof(PdschJobDev));
  q->stage.put(c.cws.data(), c.cws.size() * sizeof(PdschCwDev));
  q->stage.put(c.new_ci.data(), c.new_ci.size() * 4);
  q->stage.put(c.new_dst.data(), c.new_dst.size() * 8);
  if (c.er) q->stage.put(c.er->rj.data(), c.njobs * sizeof(EqRmJob));
  *t_put = host_now();
  // after_s: the previous batch may still be in flight; its front end (the only reader of the descriptors) is done
  // at fe_done
  CHECK_HIP(q->stage.upload(c.base, c.s, c.after_s, c.after_s && q->fe_armed ? q->fe_done : nullptr));
  return MI355_SUCCESS;
}

// step 5: the launches, and fe_done behind the last of them; t[0..4]: the host clock after each
int launch(FrontCall& c, HostTime t[5])
{
  mi355_pdsch_t*     q    = c.q;
  const PdschJobDev* jobs = c.dev<PdschJobDev>(c.lay.jobs);
  const uint32_t     nkeys = (uint32_t)c.fkeys.size();
  CHECK_HIP(pdsch_launch_equalize(jobs, c.njobs, c.max_units, c.s));
  t[0] = host_now();
  CHECK_HIP(pdsch_launch_scr_pack(c.dev<uint32_t>(c.lay.nci), (uint32_t* const*)(c.base + c.lay.ndst),
                                  (uint32_t)c.new_ci.size(), q->gold.as<uint32_t>(), PDSCH_GOLD_MAX / 32, c.s));
  t[1]         = host_now();
  q->e_pending = c.er != nullptr;
  if (c.er) {
    CHECK_HIP(pdsch_launch_eq_rm(jobs, c.dev<EqRmJob>(c.lay.rj), c.njobs, c.er->max_c, c.er->img, c.er->cimg,
                                 c.fkeys.data(), nkeys, c.er->pool, c.s));
    q->last_jobs_dev = jobs, q->last_njobs = c.njobs, q->last_max_fpairs = c.max_fpairs;
    q->last_fkeys = c.fkeys;
  } else {
    CHECK_HIP(pdsch_launch_fused(jobs, c.njobs, c.max_fpairs, c.fkeys.data(), nkeys, c.s));
  }
  t[2] = host_now();
  CHECK_HIP(pdsch_launch_llr(c.dev<PdschCwDev>(c.lay.cws), (uint32_t)c.cws.size(), c.max_pairs, c.s));
  t[3] = host_now();
  if (!q->fe_done) CHECK_HIP(hipEventCreateWithFlags(&q->fe_done, hipEventDisableTiming));
  CHECK_HIP(hipEventRecord(q->fe_done, c.s));
  q->fe_armed = true;
  t[4]        = host_now();
  return MI355_SUCCESS;
}

} // namespace

int mi355::run_frontend(mi355_pdsch_t* q, const mi355_pdsch_job_t* jobs, std::vector<JobPlan>& plans, hipStream_t s,
                        bool after_s, const EqRmPlan* er)
{
  const HostTime t_in = host_now();
  FrontCall      c{q, jobs, plans, s, after_s, er, (uint32_t)plans.size()};
  int            r;
  if ((r = collect_codewords(c)) || (r = reserve_scratch(c))) return r;
  patch_pointers(c);
  const HostTime ta = host_now();
  HostTime       tb, tl[5];
  if ((r = stage_and_upload(c, &tb))) return r;
  const HostTime tc = host_now();
  if ((r = launch(c, tl))) return r;
  if (env_host_prof()) {
    fprintf(stderr, "[mi355 host] pdsch frontend: tables %.1f us, put %.1f us, upload %.1f us, launches %.1f us "
                    "(equalize %.1f, scr %.1f, fused %.1f, llr %.1f, event %.1f)\n",
            host_us(t_in, ta), host_us(ta, tb), host_us(tb, tc), host_us(tc, tl[4]), host_us(tc, tl[0]),
            host_us(tl[0], tl[1]), host_us(tl[1], tl[2]), host_us(tl[2], tl[3]), host_us(tl[3], tl[4]));
  }
  return MI355_SUCCESS;
}
