// srsran_amd/csrc/ue_dl_front.cpp -- the front end of every mi355_ue_dl_* call: the OFDM and estimator plans
// (ue_dl_object.h) and srslte_chest_dl_res_t from the estimator's outputs.
#include <algorithm>
#include <cmath>

#include "lte_common.h"
#include "ue_dl_object.h"

namespace mi355 {

namespace {

float to_db(float v) { return 10.0f * log10f(v); }
float to_dbm(float v) { return to_db(v) + 30.0f; }

int get_scratch(mi355_ue_dl_t* q, size_t bytes, char** p)
{
  // may still be read by this object's batch in flight: retired, not freed (no device-wide wait)
  CHECK_HIP(q->scratch.reserve(bytes, bytes + bytes / 4 + 4096, DevScratch::Retire));
  *p = q->scratch.base();
  return MI355_SUCCESS;
}

// the automatic Gauss sigma of a subframe reads the PSS estimate of the link's previous subframe 0/5, which itself
// comes after that subframe's interpolation
bool pss_auto_sigma(const mi355_chest_dl_cfg_t* cfg)
{
  return cfg->noise_alg == MI355_NOISE_ALG_PSS && cfg->filter_type == MI355_CHEST_FILTER_GAUSS && cfg->filter_coef[0] <= 0;
}

} // namespace

int OfdmPlan::build(mi355_ue_dl_t* q, const mi355_dl_sf_job_t* jobs, uint32_t njobs, hipStream_t s)
{
  const size_t nj = (size_t)njobs * q->nof_rx;
  a  = q->ofdm;
  rx = q->nof_rx;
  // srsUE's one-subframe calls: jobs in the kernel arguments (not for range launches, which address the table)
  const bool inl = nj <= OFDM_INLINE_JOBS && !ranges && env_inline_jobs();
  OfdmJob*   oj  = a.inl;
  if (!inl) {
    CHECK_HIP(q->st_ofdm.reserve(nj * sizeof(OfdmJob)));
    oj = (OfdmJob*)q->st_ofdm.slot(nj * sizeof(OfdmJob));
  }
  for (uint32_t i = 0; i < njobs; i++) {
    for (uint32_t r = 0; r < rx; r++) {
      if (!jobs[i].in_buffer[r] || !jobs[i].sf_symbols[r]) return MI355_ERROR_INVALID_INPUTS;
      oj[(size_t)i * rx + r] = OfdmJob{(const float2*)jobs[i].in_buffer[r], (float2*)jobs[i].sf_symbols[r]};
    }
  }
  a.jobs = nullptr;
  used   = 0;
  if (inl) return MI355_SUCCESS;
  char* base = nullptr;
  int   r    = get_scratch(q, nj * sizeof(OfdmJob) + 256, &base);
  if (r) return r;
  CHECK_HIP(q->st_ofdm.upload(base, s));
  a.jobs = (const OfdmJob*)base;
  used   = (nj * sizeof(OfdmJob) + 255) / 256 * 256;
  return MI355_SUCCESS;
}

int OfdmPlan::launch(uint32_t o, uint32_t m, hipStream_t s) const
{
  const size_t b = (size_t)o * rx, e = (size_t)(o + m) * rx;
  if (!a.jobs) { // in the kernel arguments: the whole (one-subframe) call
    CHECK_HIP(ofdm_launch_rx(a, (uint32_t)(e - b), s));
    return MI355_SUCCESS;
  }
  OfdmArgs x = a;
  for (size_t off = b; off < e; off += 65535) { // grid.y is limited to 65535: launch in chunks
    x.jobs = a.jobs + off;
    CHECK_HIP(ofdm_launch_rx(x, (uint32_t)std::min<size_t>(65535, e - off), s));
  }
  return MI355_SUCCESS;
}

// fill_res (chest_dl.c:944-972) for one job from its per (rx, port) outputs v[(rx * P + port) * CHEST_OUT], then the
// link's state moves on to this subframe (jobs are filled in batch order)
static void fill_res(mi355_ue_dl_t* q, const mi355_chest_dl_cfg_t* cfg, const float* v, const mi355_dl_sf_job_t& job,
                     mi355_chest_dl_res_t* res)
{
  const uint32_t P = q->cell.nof_ports, R = q->nof_rx, nprb = q->cell.nof_prb;
  ChestLink&     L = q->links[job.link];
  float          noise[4][4] = {}, rsrp[4][4] = {}, rssi[4][4] = {}, rsrp_corr[4][4] = {};
  const uint32_t npil[4] = {8 * nprb, 8 * nprb, 4 * nprb, 4 * nprb};
  for (uint32_t a = 0; a < R; a++) {
    for (uint32_t p = 0; p < P; p++) {
      const float* o = &v[(a * P + p) * CHEST_OUT];
      noise[a][p]    = o[CHEST_O_NF];
      rsrp[a][p]     = o[CHEST_O_RSRP];
      rssi[a][p]     = o[CHEST_O_RSSI];
      L.noise[a][p]  = noise[a][p];
      if (cfg->rsrp_neighbour) { // estimate_port :797-800
        const float re = o[CHEST_O_PE_RE], im = o[CHEST_O_PE_IM];
        const double e  = std::sqrt((double)(re / npil[p]) * (re / npil[p]) + (double)(im / npil[p]) * (im / npil[p]));
        rsrp_corr[a][p] = (float)(e * e);
      }
    }
  }
  const uint32_t sf = job.tti % 10;
  if (cfg->cfo_estimate_enable && ((1u << sf) & cfg->cfo_estimate_sf_mask)) // :635-637
    L.cfo = v[((R - 1) * P + (P - 1)) * CHEST_OUT + CHEST_O_CFO];
  if (cfg->sync_error_enable) L.sync = v[CHEST_O_SYNC]; // sync_err[0][0]
  memset(res, 0, sizeof(*res));
  res->nof_re = 2 * (q->cell.cp == MI355_CP_EXT ? 6 : 7) * 12 * nprb;
  // get_noise
  float n = 0;
  for (uint32_t a = 0; a < R; a++) {
    float acc = 0;
    for (uint32_t p = 0; p < P; p++) acc += noise[a][p];
    n += acc / P;
  }
  n /= R;
  auto rsrp_port = [&](uint32_t port) {
    float sum = 0;
    for (uint32_t j = 0; j < R; j++) sum += rsrp[j][port];
    return sum / R;
  };
  // get_rsrp: the reference iterates its "port" argument over the rx antenna count (chest_dl.c:897-905)
  float rs = -1e9f;
  for (uint32_t i = 0; i < R; i++) rs = std::max(rs, rsrp_port(i));
  float neigh = -1e9f;
  for (uint32_t i = 0; i < R; i++) {
    float sum = 0;
    for (uint32_t j = 0; j < P; j++) sum += rsrp_corr[i][j];
    neigh = std::max(neigh, sum / P);
  }
  float rq = 0, ri = 0;
  for (uint32_t a = 0; a < R; a++) {
    rq += nprb * rsrp[a][0] / rssi[a][0];
    ri += 4 * rssi[a][0] / nprb / 12;
  }
  rq /= R;
  ri /= R;
  res->noise_estimate     = n;
  res->noise_estimate_dbm = to_dbm(n);
  res->cfo                = L.cfo;
  res->rsrp               = rs;
  res->rsrp_dbm           = to_dbm(rs);
  res->rsrp_neigh         = neigh;
  res->rsrq               = rq;
  res->rsrq_db            = to_db(rq);
  res->snr_db             = to_db(rs / n);
  res->rssi_dbm           = to_dbm(ri);
  res->sync_error         = L.sync;
  for (uint32_t p = 0; p < P; p++) {
    res->rsrp_port_dbm[p] = to_dbm(rsrp_port(p));
    for (uint32_t a = 0; a < R; a++) {
      res->snr_ant_port_db[a][p]   = to_db(rsrp[a][p] / noise[a][p]);
      res->rsrp_ant_port_dbm[a][p] = to_dbm(rsrp[a][p]);
      res->rsrq_ant_port_db[a][p]  = to_db(nprb * rsrp[a][p] / rssi[a][p]);
    }
  }
}

static int chest_check_cfg(const mi355_ue_dl_t* q, const mi355_chest_dl_cfg_t* cfg)
{
  if (!cfg) return MI355_ERROR_INVALID_INPUTS;
  if (cfg->estimator_alg > MI355_ESTIMATOR_ALG_WIENER || cfg->noise_alg > MI355_NOISE_ALG_EMPTY ||
      cfg->filter_type > MI355_CHEST_FILTER_NONE)
    return MI355_ERROR;
  // WIENER (chest_dl.c:648-676): the reference allocates its states for 2 ports (chest_dl.c:147) and its ready path
  // skips the PSS / EMPTY noise update; supported with REFS noise, 1-2 ports, 1-2 rx, >= 6 PRB, normal CP
  if (cfg->estimator_alg == MI355_ESTIMATOR_ALG_WIENER &&
      (cfg->noise_alg != MI355_NOISE_ALG_REFS || q->cell.nof_ports > WNR_MAX_TX || q->nof_rx > WNR_MAX_RX ||
       q->cell.nof_prb < 6 || q->cell.cp != MI355_CP_NORM))
    return MI355_ERROR;
  return MI355_SUCCESS;
}

bool chest_deferrable(const mi355_chest_dl_cfg_t* cfg)
{
  return cfg && cfg->estimator_alg != MI355_ESTIMATOR_ALG_WIENER && !pss_auto_sigma(cfg);
}

// the estimator's tables (sync-error stage, estimation, noise resolution and, when wanted, the per-job get_noise);
// the scratch region starts after `offset` bytes (the OFDM job table may live before it)
int ChestPlan::build(mi355_ue_dl_t* q, const mi355_dl_sf_job_t* jobs_, uint32_t njobs_, const mi355_chest_dl_cfg_t* cfg_,
                     hipStream_t s, size_t offset)
{
  int r = chest_check_cfg(q, cfg_);
  if (r) return r;
  cfg = cfg_, jobs = jobs_, njobs = njobs_;
  const uint32_t P = q->cell.nof_ports, R = q->nof_rx;
  const bool     wiener = cfg->estimator_alg == MI355_ESTIMATOR_ALG_WIENER;
  if (wiener && !q->wiener) {
    auto* b = new WienerBank();
    if ((r = b->init(q->device, q->cell.nof_prb, P, R))) {
      delete b;
      return r;
    }
    q->wiener = b;
  }
  const size_t   ncj = (size_t)njobs * P * R;
  uint32_t       maxl = 0;
  for (uint32_t i = 0; i < njobs; i++) {
    if (jobs[i].link >= MI355_MAX_LINKS) return MI355_ERROR_INVALID_INPUTS;
    maxl = std::max(maxl, jobs[i].link);
  }
  if (njobs && q->links.size() <= maxl) q->links.resize((size_t)maxl + 1);
  // srsUE's one-subframe calls: the (job, rx, port) entries travel in the kernel arguments, no descriptor upload
  // (not for range launches, the Wiener stage or the PSS automatic-sigma order, which address the array)
  const bool inl = ncj <= CHEST_INLINE_JOBS && !ranges && !wiener && !pss_auto_sigma(cfg) && env_inline_jobs();
  ChestJob*  cj  = a.inl;
  if (!inl) {
    CHECK_HIP(q->st_chest.reserve(ncj * sizeof(ChestJob)));
    cj = (ChestJob*)q->st_chest.slot(ncj * sizeof(ChestJob));
  }
  const size_t nout = ncj * CHEST_OUT;
  char*        base = nullptr;
  const size_t jb   = (ncj * sizeof(ChestJob) + 255) / 256 * 256;
  const size_t ob   = (nout * 4 + 255) / 256 * 256;
  const size_t nb   = ((size_t)njobs * 4 + 255) / 256 * 256;
  const size_t pb   = wiener ? ncj * 4 * 2 * q->cell.nof_prb * sizeof(float2) : 0; // LS pilots for the Wiener stage
  if ((r = get_scratch(q, offset + jb + ob + nb + pb + 256, &base))) return r;
  base += offset;
  d_out   = (float*)(base + jb);
  d_noise = (float*)(base + jb + ob);
  const bool sf05_alg = cfg->noise_alg != MI355_NOISE_ALG_REFS; // PSS / EMPTY: state updated in subframes 0 and 5
  std::vector<int32_t> last05(sf05_alg ? (size_t)maxl + 1 : 0, -1);
  size_t               k = 0;
  for (uint32_t i = 0; i < njobs; i++) {
    const uint32_t sf   = jobs[i].tti % 10;
    const bool     is05 = sf05_alg && (sf == 0 || sf == 5);
    const bool     cfo  = cfg->cfo_estimate_enable && ((1u << sf) & cfg->cfo_estimate_sf_mask);
    const ChestLink& L  = q->links[jobs[i].link];
    const int32_t  src  = sf05_alg ? last05[jobs[i].link] : -1;
    for (uint32_t a = 0; a < R; a++) {
      for (uint32_t p = 0; p < P; p++) {
        if (!jobs[i].sf_symbols[a] || !jobs[i].ce[p][a]) return MI355_ERROR_INVALID_INPUTS;
        ChestJob& J  = cj[k++];
        J.grid       = (float2*)jobs[i].sf_symbols[a];
        J.ce         = (float2*)jobs[i].ce[p][a];
        J.out        = d_out + (((size_t)i * R + a) * P + p) * CHEST_OUT;
        J.sf         = sf;
        J.port       = p;
        J.flags      = (is05 ? CHEST_F_NOISE_SF05 : 0u) | (cfo && a == R - 1 && p == P - 1 ? CHEST_F_CFO : 0u);
        J.src        = src >= 0 ? (int32_t)((((size_t)src * R + a) * P + p) * CHEST_OUT) : -1;
        J.noise_prev = L.noise[a][p];
      }
    }
    if (is05) last05[jobs[i].link] = (int32_t)i;
  }
  a.jobs = nullptr;
  if (!inl) {
    CHECK_HIP(q->st_chest.upload(base, s));
    a.jobs = (const ChestJob*)base;
  }
  a.pilots      = q->pilots.as<float2>();
  a.pss         = q->pss.as<float2>();
  a.out_all     = d_out;
  a.nof_prb     = q->cell.nof_prb;
  a.cell_id     = q->cell.id;
  a.nsymb       = q->cell.cp == MI355_CP_EXT ? 6 : 7;
  a.nof_ports   = P;
  a.nof_rx      = R;
  a.filter_type = cfg->filter_type;
  a.alg         = wiener ? MI355_ESTIMATOR_ALG_AVERAGE : cfg->estimator_alg; // WIENER falls back to AVERAGE until ready
  a.pe_out      = wiener ? (float2*)(base + jb + ob + nb) : nullptr;
  a.noise_alg   = cfg->noise_alg;
  a.coef0       = cfg->filter_coef[0];
  a.coef1       = cfg->filter_coef[1];
  a.symbol_sz   = q->ofdm.N;
  a.cfo_n       = (float)q->ofdm.N;
  a.cfo_ns      = (float)a.nsymb;
  a.cfo_ng      = (float)cp_len(q->ofdm.N, 144); // SRSLTE_CP_LEN_NORM(1, n)
  a.sync_k      = (float)q->ofdm.N / 6.0f;
  a.ce_rows     = row0 && ce_time_invariant(cfg) ? 1u : 2 * a.nsymb;
  return ranges && !chest_deferrable(cfg) ? MI355_ERROR : MI355_SUCCESS;
}

int ChestPlan::launch(uint32_t o, uint32_t m, hipStream_t s) const
{
  const uint32_t RP = a.nof_rx * a.nof_ports;
  ChestArgs      x  = a;
  if (a.jobs) x.jobs = a.jobs + (size_t)o * RP;
  CHECK_HIP(chest_launch_pre(x, m, cfg->sync_error_enable != 0, cfg->noise_alg == MI355_NOISE_ALG_EMPTY, s));
  if (pss_auto_sigma(cfg)) { // (not deferrable: the whole batch) up to and including each subframe 0/5 in turn
    uint32_t b = o;
    for (uint32_t i = o; i < o + m; i++) {
      const uint32_t sf = jobs[i].tti % 10;
      if (sf == 0 || sf == 5 || i + 1 == o + m) {
        ChestArgs cs = a;
        cs.jobs      = a.jobs + (size_t)b * RP;
        CHECK_HIP(chest_launch(cs, (i + 1 - b) * RP, s));
        b = i + 1;
      }
    }
  } else {
    CHECK_HIP(chest_launch(x, m * RP, s));
  }
  CHECK_HIP(chest_launch_resolve(x, m, want_noise ? d_noise + o : nullptr, s));
  return MI355_SUCCESS;
}

int ChestPlan::launch_all(mi355_ue_dl_t* q, hipStream_t s) const
{
  int r = launch(0, njobs, s);
  if (r || cfg->estimator_alg != MI355_ESTIMATOR_ALG_WIENER) return r;
  // srslte_wiener_dl_run for m = 0..17 of every (rx, port) with this subframe's REFS noise and RSRP; the Wiener rows
  // replace the AVERAGE estimate where the link was ready (chest_dl.c:648-676)
  const uint32_t         P = a.nof_ports, R = a.nof_rx;
  std::vector<WienerJob> wj(njobs);
  std::vector<uint32_t>  wl(njobs);
  const size_t           nref = 2 * q->cell.nof_prb;
  for (uint32_t i = 0; i < njobs; i++) {
    WienerJob& J = wj[i];
    memset(&J, 0, sizeof(J));
    J.pilots    = a.pe_out + (size_t)i * R * P * 4 * nref;
    J.chest_out = d_out + (size_t)i * R * P * CHEST_OUT;
    for (uint32_t x = 0; x < R; x++)
      for (uint32_t p = 0; p < P; p++) J.ce[p][x] = (float2*)jobs[i].ce[p][x];
    wl[i] = jobs[i].link;
  }
  const uint32_t shift[WNR_MAX_TX] = {q->cell.id % 6, (3 + q->cell.id % 6) % 6}; // srslte_refsignal_cs_fidx(cell, 0, p, 0)
  return q->wiener->launch(wj.data(), wl.data(), njobs, shift, false, CHEST_OUT, CHEST_O_NOISE, CHEST_O_RSRP, s);
}

int FrontPlan::start(mi355_ue_dl_t* q, const mi355_dl_sf_job_t* jobs, uint32_t njobs, const mi355_chest_dl_cfg_t* cfg,
                     hipStream_t s, uint32_t m0)
{
  const bool ranges = ofdm.ranges = chest.ranges;
  int        r      = ofdm.build(q, jobs, njobs, s);
  if (!r) r = ofdm.launch(0, ranges ? m0 : njobs, s);
  if (!r) r = chest.build(q, jobs, njobs, cfg, s, ofdm.used);
  if (!r) r = ranges ? chest.launch(0, m0, s) : chest.launch_all(q, s);
  return r;
}

int chest_finish(mi355_ue_dl_t* q, const mi355_chest_dl_cfg_t* cfg, const float* d_out, const mi355_dl_sf_job_t* jobs,
                 uint32_t njobs, mi355_chest_dl_res_t* res, hipStream_t s)
{
  const uint32_t     P = q->cell.nof_ports, R = q->nof_rx;
  const size_t       nout = (size_t)njobs * P * R * CHEST_OUT;
  CHECK_HIP(q->back.reserve(nout * 4));
  const float* out = (const float*)q->back.host;
  CHECK_HIP(stage_copy(q->back.host, d_out, nout * 4, s));
  CHECK_HIP(wait_stream(s));
  for (uint32_t i = 0; i < njobs; i++) fill_res(q, cfg, &out[(size_t)i * R * P * CHEST_OUT], jobs[i], &res[i]);
  return MI355_SUCCESS;
}

void chest_fill_cb(void* p)
{
  ChestFill* f = (ChestFill*)p;
  if (f->done || wait_stream(f->q->side) != hipSuccess) return; // the read-back has landed
  const uint32_t k = f->q->cell.nof_ports * f->q->nof_rx * CHEST_OUT;
  for (uint32_t i = 0; i < f->njobs; i++) fill_res(f->q, f->cfg, &f->out[(size_t)i * k], f->jobs[i], &f->res[i]);
  f->done = true;
}

int chest_finish_async(mi355_ue_dl_t* q, ChestFill* f, const float* d_out, hipStream_t s)
{
  if (!q->side) CHECK_HIP(hipStreamCreateWithFlags(&q->side, hipStreamNonBlocking));
  if (!q->ev_chest) CHECK_HIP(hipEventCreateWithFlags(&q->ev_chest, hipEventDisableTiming));
  const size_t nout = (size_t)f->njobs * q->cell.nof_ports * q->nof_rx * CHEST_OUT;
  CHECK_HIP(q->back.reserve(nout * 4));
  f->out = (const float*)q->back.host;
  CHECK_HIP(hipEventRecord(q->ev_chest, s));
  CHECK_HIP(hipStreamWaitEvent(q->side, q->ev_chest, 0));
  CHECK_HIP(stage_copy(q->back.host, d_out, nout * 4, q->side));
  return MI355_SUCCESS;
}

} // namespace mi355
