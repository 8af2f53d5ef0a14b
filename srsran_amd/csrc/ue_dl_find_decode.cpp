// srsran_amd/csrc/ue_dl_find_decode.cpp -- the mi355_ue_dl_* calls through the control-channel stage:
// srslte_ue_dl_find_dl_dci on given estimates, estimation + search in one call, and find_and_decode (estimation,
// search, grants and the PDSCH decode, pipelined over chunks of the batch).
#include <atomic>
#include <cmath>
#include <stdio.h>

#include "../../include/srsran_amd/tdec.h"
#include "host_parallel.h"
#include "ue_dl_object.h"

using namespace mi355;

int mi355::ctrl_ready(mi355_ue_dl_t* q)
{
  if (q->ctrl) return MI355_SUCCESS;
  auto* c = new CtrlState;
  int   r = c->init(q->cell, q->nof_rx);
  if (r) {
    delete c;
    return r;
  }
  q->ctrl = c;
  return MI355_SUCCESS;
}

// search results -> srslte_dci_dl_t (srslte_dci_msg_unpack_pdsch with the UE's DCI configuration, ue_dl.c:722-728)
static int unpack_all(mi355_ue_dl_t* q, const mi355_dl_sf_cfg_t* sfs, const mi355_ue_dl_cfg_t* cfgs, uint32_t n,
                      mi355_ctrl_res_t* ctrl, mi355_dci_msg_t* msgs, mi355_dci_dl_t* dci, uint32_t first = 0)
{
  host_parallel_for(n - first, 128, [&](uint32_t b, uint32_t e) {
    for (uint32_t i = first + b; i < first + e; i++) {
      for (int k = 0; k < ctrl[i].nof_dci; k++) {
        mi355_dci_msg_t& m = msgs[(size_t)i * MI355_MAX_DCI_MSG + k];
        if (mi355_dci_msg_unpack_pdsch(&q->cell, &sfs[i], &cfgs[i].dci, &m, &dci[(size_t)i * MI355_MAX_DCI_MSG + k]))
          ctrl[i].nof_dci = -1; // "Error unpacking DL DCI" (ue_dl.c:724-727)
        if (ctrl[i].nof_dci < 0) break;
      }
    }
  });
  return MI355_SUCCESS;
}

// the replay writes every message it reports: stale contents of earlier calls are never read
static mi355_dci_msg_t* fd_msgs(mi355_ue_dl_t* q, uint32_t njobs)
{
  if (q->fd_msgs.size() < (size_t)njobs * MI355_MAX_DCI_MSG) q->fd_msgs.resize((size_t)njobs * MI355_MAX_DCI_MSG);
  return q->fd_msgs.data();
}

// test hook: the next n control stages of combined calls fail after their estimation (the drop-in's recovery path)
static std::atomic<int> g_fail_ctrl{0};

// One find_and_decode call: its arguments, and what its steps hand on
struct FdCall {
  mi355_ue_dl_t*              q;
  mi355_softbuffer_pool_t*    pool;
  const mi355_dl_sf_job_t*    sfjobs;
  mi355_dl_sf_cfg_t*          sfs;
  const mi355_ue_dl_cfg_t*    ue_cfgs;
  mi355_pdsch_cfg_t*          cfgs;
  const mi355_chest_dl_cfg_t* chest_cfg;
  mi355_chest_dl_res_t*       chest;
  uint8_t* const*             payloads;
  uint32_t                    njobs;
  mi355_ctrl_res_t*           ctrl;
  mi355_dci_dl_t*             dci;
  mi355_pdsch_res_t*          res;
  hipStream_t                 s;
  uint32_t                    nchunks, split0, end0; // chunk count; two chunks' first size (0: half); chunk 0's end
  const uint16_t*             rntis;   // q->fd_rntis
  mi355_dci_msg_t*            msgs;    // q->fd_msgs
  const float*                d_noise; // the estimator's per-subframe noise on the device
  ChestFill*                  fill;
};

// Two chunks: the host replays chunk 0's blind searches and builds its grants while the GPU decodes chunk 1's
// control channels, and does chunk 1's while the GPU decodes chunk 0's PDSCH, so the GPU never waits for the
// host's sequential find -> grant order.  Every subframe's outcome is the same as in one chunk: subframes are
// independent.  (mi355_ue_dl_set_chunks, or MI355_UEDL_CHUNKS when it is not set, overrides the choice, and
// MI355_UEDL_SPLIT0 the first of two chunks' share: tests, A/B timing)
static void fd_split(FdCall& f)
{
  const uint32_t forced = f.q->chunks ? f.q->chunks : env_uedl_chunks();
  f.nchunks = forced ? std::max(1u, std::min(forced, f.njobs)) : (f.njobs >= 256 ? 2u : 1u);
  f.split0  = f.nchunks == 2 ? (uint32_t)((uint64_t)f.njobs * env_uedl_split0() / 100) : 0u;
  f.end0    = f.split0 ? f.split0 : (uint32_t)((uint64_t)f.njobs / f.nchunks); // CtrlState::launch's first boundary
}

// srslte_ue_dl_decode_fft_estimate: OFDM + estimation; the noise estimate stays on the device for the control
// channels, the host fills srslte_chest_dl_res_t while the control kernels run.  Where the estimator can run in
// ranges, OFDM and estimation of chunk c are launched right in front of chunk c's control kernels, so the host
// replays chunk 0's blind searches while the GPU demodulates, estimates and searches chunk 1 (chunk 0's are
// launched here, as soon as their tables are up, so the GPU works while the host builds the rest)
static int fd_launch_front(FdCall& f, FrontPlan& fp)
{
  mi355_ue_dl_t* q    = f.q;
  fp.chest.ranges     = chest_deferrable(f.chest_cfg) && f.njobs > 0;
  fp.chest.row0       = ce_row0_only(q);
  fp.chest.want_noise = true;
  int r = fp.start(q, f.sfjobs, f.njobs, f.chest_cfg, f.s, f.end0);
  if (r) return r;
  if (!fp.chest.ranges && (r = chest_finish_async(q, f.fill, fp.chest.d_out, f.s))) return r;
  q->fd_rntis.resize(f.njobs);
  for (uint32_t i = 0; i < f.njobs; i++) q->fd_rntis[i] = f.cfgs[i].rnti;
  f.rntis = q->fd_rntis.data(), f.msgs = fd_msgs(q, f.njobs), f.d_noise = fp.chest.d_noise;
  return MI355_SUCCESS;
}

// the control kernels of every chunk, each later chunk's front end launched right in front of its own.  On a
// failure srslte_chest_dl_res_t is filled where the whole estimation was launched (no ranges), else left unfilled
static int fd_launch_ctrl(const FdCall& f, const FrontPlan& fp)
{
  mi355_ue_dl_t* q      = f.q;
  const bool     ranges = fp.chest.ranges;
  std::function<int(uint32_t, uint32_t)> front; // chunk 0's front end is already launched
  if (ranges) front = [&](uint32_t o, uint32_t m) { return o ? fp.launch(o, m, f.s) : (int)MI355_SUCCESS; };
  // AVERAGE estimates are time-invariant: the control channels read row 0 (the only one written with ce_rows = 1)
  int r = q->ctrl->launch(f.sfjobs, nullptr, f.d_noise, f.rntis, f.ue_cfgs, f.njobs, f.nchunks,
                          ce_row_arg(q, ce_time_invariant(f.chest_cfg)), f.split0, f.s, front);
  if (r) {
    if (ranges) (void)hipStreamSynchronize(f.s);
    else chest_fill_cb(f.fill);
    return r;
  }
  return ranges ? chest_finish_async(q, f.fill, fp.chest.d_out, f.s) : MI355_SUCCESS;
}

static void fd_reset_chunks(mi355_ue_dl_t* q, uint32_t nchunks)
{
  if (q->fd_ck.size() < nchunks) q->fd_ck.resize(nchunks);
  for (uint32_t c = 0; c < nchunks; c++) { // (capacity kept)
    FdChunk& C = q->fd_ck[c];
    C.jobs.clear(), C.which.clear(), C.rs_sb.clear(), C.rs_tbs.clear(), C.sub.clear();
    C.r = MI355_SUCCESS, C.launched = false;
  }
}

// srslte_ue_dl_find_dl_dci + DCI -> grant, RV from the SFN for format 1C, softbuffer reset list (ue_dl.c:1494-1535)
// and the PDSCH jobs of chunk c, once its control read-back has landed
static void fd_prepare_chunk(const FdCall& f, uint32_t c)
{
  mi355_ue_dl_t* q = f.q;
  FdChunk&       C = q->fd_ck[c];
  C.b              = c ? q->ctrl->chunk_end[c - 1] : 0;
  C.e              = q->ctrl->chunk_end[c];
  if ((C.r = q->ctrl->finish(c, f.rntis, f.ue_cfgs, f.ctrl, f.msgs))) return;
  for (uint32_t i = C.b; i < C.e; i++) f.sfs[i].cfi = f.ctrl[i].cfi;
  if ((C.r = unpack_all(q, f.sfs, f.ue_cfgs, C.e, f.ctrl, f.msgs, f.dci, C.b))) return;
  host_parallel_for(C.e - C.b, 128, [&](uint32_t lo, uint32_t hi) { // grants: independent per subframe
    for (uint32_t i = C.b + lo; i < C.b + hi; i++) {
      if (f.ctrl[i].nof_dci != 1) continue; // the reference decodes only when exactly one DCI was found
      const mi355_dci_dl_t& d = f.dci[(size_t)i * MI355_MAX_DCI_MSG];
      if (mi355_ra_dl_dci_to_grant(&q->cell, &f.sfs[i], f.ue_cfgs[i].tm, f.ue_cfgs[i].use_tbs_index_alt, &d,
                                   &f.cfgs[i].grant)) {
        f.ctrl[i].nof_dci = -1; // "Error unpacking DCI"
        continue;
      }
      for (int tb = 0; tb < MI355_MAX_CODEWORDS; tb++) {
        mi355_ra_tb_t& t = f.cfgs[i].grant.tb[tb];
        if (t.enabled && (int32_t)t.rv < 0) {
          const uint32_t k = ((f.sfs[i].tti / 10) / 2) % 4;
          t.rv             = ((uint32_t)ceilf(1.5f * k)) % 4;
        }
      }
    }
  });
  for (uint32_t i = C.b; i < C.e; i++) {
    if (f.ctrl[i].nof_dci != 1) continue;
    for (int tb = 0; tb < MI355_MAX_CODEWORDS; tb++) {
      const mi355_ra_tb_t& t = f.cfgs[i].grant.tb[tb];
      if (!t.enabled) continue;
      C.rs_sb.push_back(f.cfgs[i].softbuffer[tb]);
      C.rs_tbs.push_back((uint32_t)t.tbs);
    }
    for (int tb = 0; tb < 2; tb++) f.res[2 * i + tb].crc = 0;
    C.jobs.emplace_back();
    pdsch_job_fill(C.jobs.back(), q, f.sfjobs, f.sfs, f.cfgs, f.payloads, i);
    C.which.push_back(i);
  }
}

// Chunk c's PDSCH + DL-SCH are enqueued with their results left in flight; chunk c+1's replay and grants then run
// on the host while the GPU decodes chunk c, and chunk c+1's decode is enqueued right behind it (its descriptor
// uploads ordered after chunk c's kernels), so the GPU goes from chunk to chunk without waiting for a read-back.
static int fd_enqueue_chunk(const FdCall& f, uint32_t c)
{
  mi355_ue_dl_t* q = f.q;
  FdChunk&       C = q->fd_ck[c];
  // every subframe of the chunk decodes (the usual case): the equaliser reads the device noise estimates;
  // otherwise the host values of srslte_chest_dl_res_t are needed first
  const bool all = C.jobs.size() == C.e - C.b;
  if (!all) {
    chest_fill_cb(f.fill);
    for (size_t k = 0; k < C.jobs.size(); k++) C.jobs[k].noise_estimate = f.chest[C.which[k]].noise_estimate;
  }
  if (C.jobs.empty()) return MI355_SUCCESS;
  int r = mi355_softbuffer_reset_tbs_batch(f.pool, C.rs_sb.data(), C.rs_tbs.data(), (uint32_t)C.rs_sb.size(), f.s);
  if (r) return r;
  C.sub.resize(2 * C.jobs.size());
  for (size_t k = 0; k < C.jobs.size(); k++) C.sub[2 * k] = f.res[2 * C.which[k]], C.sub[2 * k + 1] = f.res[2 * C.which[k] + 1];
  C.launched = true;
  return pdsch_decode_batch_dev_noise(q->pdsch, f.pool, C.jobs.data(), (uint32_t)C.jobs.size(), C.sub.data(), f.s,
                                      all ? f.d_noise + C.b : nullptr, WaitHook{}, ce_time_invariant(f.chest_cfg),
                                      q->pend[c].get(), c > 0);
}

// waits for every launched chunk's decode and moves its results to res[]; the first error, r's included
static int fd_collect(const FdCall& f, int r)
{
  for (uint32_t c = 0; c < f.nchunks; c++) {
    FdChunk& C = f.q->fd_ck[c];
    if (!C.launched) continue;
    const int e = f.q->pend[c]->collect();
    if (e && !r) r = e;
    for (size_t k = 0; k < C.jobs.size(); k++)
      f.res[2 * C.which[k]] = C.sub[2 * k], f.res[2 * C.which[k] + 1] = C.sub[2 * k + 1];
  }
  return r;
}

extern "C" {

int mi355_ue_dl_find_dl_dci_batch(mi355_ue_dl_t* q, const mi355_dl_sf_job_t* sfjobs, mi355_dl_sf_cfg_t* sfs,
                                  const mi355_ue_dl_cfg_t* cfgs, const uint16_t* rntis,
                                  const mi355_chest_dl_res_t* chest, uint32_t njobs, mi355_ctrl_res_t* ctrl,
                                  mi355_dci_dl_t* dci, void* stream)
{
  if (!q || (njobs && (!sfjobs || !sfs || !cfgs || !rntis || !chest || !ctrl || !dci))) return MI355_ERROR_INVALID_INPUTS;
  std::lock_guard<std::mutex> lock(q->mu);
  CHECK_HIP(hipSetDevice(q->device));
  int r = ctrl_ready(q);
  if (r) return r;
  std::vector<float>           noise(njobs);
  // uninitialised: the replay writes every message it reports (1.5 MB of zeroing per 2,048 subframes otherwise)
  std::unique_ptr<mi355_dci_msg_t[]> msgs(new mi355_dci_msg_t[(size_t)njobs * MI355_MAX_DCI_MSG]);
  for (uint32_t i = 0; i < njobs; i++) noise[i] = chest[i].noise_estimate;
  // the caller's estimates, read where they lie
  if ((r = q->ctrl->run(sfjobs, noise.data(), nullptr, rntis, cfgs, njobs, ce_row_arg(q, false),
                        stream ? (hipStream_t)stream : q->own, ctrl, msgs.get())))
    return r;
  for (uint32_t i = 0; i < njobs; i++) sfs[i].cfi = ctrl[i].cfi;
  return unpack_all(q, sfs, cfgs, njobs, ctrl, msgs.get(), dci);
}

int mi355_debug_fail_ctrl_stages(int n)
{
  return g_fail_ctrl.exchange(n < 0 ? 0 : n);
}

int mi355_ue_dl_fft_estimate_find_dci_batch(mi355_ue_dl_t* q, const mi355_dl_sf_job_t* sfjobs, mi355_dl_sf_cfg_t* sfs,
                                            const mi355_ue_dl_cfg_t* cfgs, const uint16_t* rntis,
                                            const mi355_chest_dl_cfg_t* chest_cfg, mi355_chest_dl_res_t* chest,
                                            uint32_t njobs, mi355_ctrl_res_t* ctrl, mi355_dci_dl_t* dci,
                                            mi355_hook_fn after_estimate, void* hook_arg, void* stream)
{
  if (!q || !chest_cfg || (njobs && (!sfjobs || !sfs || !cfgs || !rntis || !chest || !ctrl || !dci)))
    return MI355_ERROR_INVALID_INPUTS;
  std::lock_guard<std::mutex> lock(q->mu);
  CHECK_HIP(hipSetDevice(q->device));
  hipStream_t s = stream ? (hipStream_t)stream : q->own;
  int         r = ctrl_ready(q);
  if (r) return r;
  FrontPlan fp;
  fp.chest.want_noise = true;
  if ((r = fp.start(q, sfjobs, njobs, chest_cfg, s, njobs))) return r;
  // the estimator's results go back on the side stream while the control channels run
  ChestFill fill{q, chest_cfg, nullptr, sfjobs, njobs, chest, false};
  if ((r = chest_finish_async(q, &fill, fp.chest.d_out, s))) return r;
  if (after_estimate) after_estimate(hook_arg);
  mi355_dci_msg_t* const msgs = fd_msgs(q, njobs);
  // every row of the estimates is written here: read where they lie
  r = q->ctrl->run(sfjobs, nullptr, fp.chest.d_noise, rntis, cfgs, njobs, ce_row_arg(q, false), s, ctrl, msgs);
  if (!r && g_fail_ctrl.load() > 0 && g_fail_ctrl.fetch_sub(1) > 0) r = MI355_ERROR;
  chest_fill_cb(&fill); // (also after a failed control stage: the estimation itself succeeded)
  if (!fill.done) return MI355_ERROR;
  if (r) return MI355_ERROR_SECOND_STAGE; // chest[] is valid: the caller retries the control stage only
  for (uint32_t i = 0; i < njobs; i++) sfs[i].cfi = ctrl[i].cfi;
  return unpack_all(q, sfs, cfgs, njobs, ctrl, msgs, dci) == MI355_SUCCESS ? MI355_SUCCESS : MI355_ERROR_SECOND_STAGE;
}

int mi355_ue_dl_find_and_decode_batch(mi355_ue_dl_t* q, mi355_softbuffer_pool_t* pool, const mi355_dl_sf_job_t* sfjobs,
                                      mi355_dl_sf_cfg_t* sfs, const mi355_ue_dl_cfg_t* ue_cfgs, mi355_pdsch_cfg_t* cfgs,
                                      const mi355_chest_dl_cfg_t* chest_cfg, mi355_chest_dl_res_t* chest,
                                      uint8_t* const* payloads, uint32_t njobs, mi355_ctrl_res_t* ctrl,
                                      mi355_dci_dl_t* dci, mi355_pdsch_res_t* res, void* stream)
{
  if (!q || !pool || !res || !chest || !ctrl || !dci ||
      (njobs && (!sfjobs || !sfs || !ue_cfgs || !cfgs || !payloads || !chest_cfg)))
    return MI355_ERROR_INVALID_INPUTS;
  std::lock_guard<std::mutex> lock(q->mu);
  const HostTime t0 = host_now();
  CHECK_HIP(hipSetDevice(q->device));
  hipStream_t s = stream ? (hipStream_t)stream : q->own;
  int         r = ctrl_ready(q);
  if (r) return r;
  ChestFill fill{q, chest_cfg, nullptr, sfjobs, njobs, chest, false};
  FdCall    f{q, pool, sfjobs, sfs, ue_cfgs, cfgs, chest_cfg, chest, payloads, njobs, ctrl, dci, res, s};
  f.fill = &fill;
  fd_split(f);
  FrontPlan fp;
  if ((r = fd_launch_front(f, fp))) return r;
  const HostTime t1 = host_now();
  if ((r = fd_launch_ctrl(f, fp))) return r;
  const HostTime t1c = host_now();
  fd_reset_chunks(q, f.nchunks);
  const HostTime t2a = host_now();
  fd_prepare_chunk(f, 0);
  const HostTime t2 = host_now();
  if (q->fd_ck[0].r) {
    chest_fill_cb(&fill);
    return q->fd_ck[0].r;
  }
  while (q->pend.size() < f.nchunks) q->pend.emplace_back(new PdschPending);
  for (uint32_t c = 0; c < f.nchunks && !r; c++) {
    if (c) fd_prepare_chunk(f, c);
    r = q->fd_ck[c].r ? q->fd_ck[c].r : fd_enqueue_chunk(f, c);
  }
  if (!fill.done) chest_fill_cb(&fill); // srslte_chest_dl_res_t on the host while the GPU decodes
  r = fd_collect(f, r);
  CHECK_HIP(wait_stream(q->side));
  if (!fill.done) chest_fill_cb(&fill);
  if (env_host_prof())
    fprintf(stderr, "[mi355 host] find_and_decode: launch ofdm/chest %.1f us, control launch %.1f us, chunk 0 "
                    "replay/grants %.1f us (wait included), pdsch+dlsch (chunk 1 host work hidden) %.1f us\n",
            host_us(t0, t1), host_us(t1, t1c), host_us(t2a, t2), host_us(t2, host_now()));
  return r;
}

} // extern "C"
