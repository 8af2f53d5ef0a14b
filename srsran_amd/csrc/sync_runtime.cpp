// srsran_amd/csrc/sync_runtime.cpp -- host runtime of the cell search: the time-domain PSS replicas, the DFT twiddles
// and the SSS tables resident in HBM, the object's state between the calls of a sequence (correlation average and the
// scalar averages, device resident and scanned there), per-call descriptor upload, the four launches (five for a
// SEQUENCE) and one read-back of the result records.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <string.h>
#include <vector>

#include "device_mem.h"
#include "host_staging.h"
#include "sync_internal.h"

using namespace mi355;

struct mi355_sync {
  int              device = 0;
  mi355_sync_cfg_t cfg{};
  uint32_t         nhyp = 1, hyp0 = 0, L = 0;
  hipStream_t      own = nullptr;
  std::mutex       mu;
  DevMem           d_pss, d_tw, d_sss; // replicas [3][fft] | twiddles [fft] | SssTables
  DevMem           d_avg, d_state;     // conv_output_avg [nhyp][L] | SyncState [nhyp]
  DevScratch       d_buf;              // per-call arena: descriptors | averages | scan records | results
  HostStaging      st, back;
};

namespace {

// srslte_pss_init_N_id_2 (pss.c:34-63): the 62 values around DC, the unnormalised inverse DFT scaled by 1 / sqrt(N),
// conjugated and scaled by 1 / 62.  The sum is formed in double and rounded once.
std::vector<float2> pss_replicas(uint32_t N)
{
  std::vector<float2> out(3 * (size_t)N);
  for (uint32_t id2 = 0; id2 < 3; id2++) {
    float2 f[MI355_PSS_LEN];
    pss_sequence(id2, f);
    const float norm = 1.0 / sqrtf((float)N);
    for (uint32_t n = 0; n < N; n++) {
      double re = 0, im = 0;
      for (uint32_t j = 0; j < MI355_PSS_LEN; j++) {
        const double ang = 2.0 * M_PI * (double)(((int64_t)central_bin(j) * n) % (int64_t)N) / (double)N;
        const double c = std::cos(ang), s = std::sin(ang);
        re += f[j].x * c - f[j].y * s;
        im += f[j].x * s + f[j].y * c;
      }
      const float tr = (float)re * norm, ti = (float)im * norm;
      out[(size_t)id2 * N + n] = make_float2(tr * (float)(1.0 / MI355_PSS_LEN), -ti * (float)(1.0 / MI355_PSS_LEN));
    }
  }
  return out;
}

int run(mi355_sync_t* q, const mi355_sync_job_t* jobs, uint32_t n, uint32_t mode, mi355_sync_res_t* res, hipStream_t s)
{
  const uint32_t nhyp   = q->nhyp;
  const size_t   b_jobs = staged_size((size_t)n * sizeof(SyncJob));
  const size_t   b_avg  = staged_size((size_t)n * nhyp * q->L * sizeof(float));
  const size_t   b_rec  = staged_size((size_t)n * nhyp * sizeof(SyncRec));
  const size_t   b_res  = staged_size((size_t)n * nhyp * sizeof(mi355_sync_res_t));
  const size_t   need   = b_jobs + b_avg + b_rec + b_res;
  CHECK_HIP(q->d_buf.reserve(need, need + need / 4, DevScratch::SyncFree)); // grow-only
  char* base = q->d_buf.base();
  CHECK_HIP(q->st.reserve(b_jobs));
  auto* pj = (SyncJob*)q->st.slot((size_t)n * sizeof(SyncJob));
  for (uint32_t i = 0; i < n; i++) {
    if (!jobs[i].input) return MI355_ERROR_INVALID_INPUTS;
    pj[i] = SyncJob{(const float2*)jobs[i].input, jobs[i].find_offset, 0u};
  }
  CHECK_HIP(q->st.upload(base, s));
  SyncArgs a{};
  a.jobs      = (const SyncJob*)base;
  a.pss_time  = q->d_pss.as<float2>();
  a.tw        = q->d_tw.as<float2>();
  a.sss       = q->d_sss.as<SssTables>();
  a.avg       = (float*)(base + b_jobs);
  a.avg_state = q->d_avg.as<float>();
  a.state     = q->d_state.as<SyncState>();
  a.rec       = (SyncRec*)(base + b_jobs + b_avg);
  a.res       = (mi355_sync_res_t*)(base + b_jobs + b_avg + b_rec);
  a.njobs = n, a.nhyp = nhyp, a.hyp0 = q->hyp0;
  a.fft = q->cfg.fft_size, a.N = q->cfg.max_offset, a.L = q->L;
  a.shortwin = a.N < a.fft;
  a.nout     = a.shortwin ? a.N - 1 : a.N + a.fft - 2;
  a.seq      = mode == MI355_SYNC_SEQUENCE;
  a.cfg      = q->cfg;
  // the launches and the one read-back of the call; whatever fails, the stream is waited for before returning, so
  // that neither staging buffer is left in flight
  const size_t bytes = (size_t)n * nhyp * sizeof(mi355_sync_res_t);
  hipError_t   e     = q->back.reserve(bytes);
  if (e == hipSuccess) e = sync_launch_corr(a, s);
  if (e == hipSuccess && a.seq) e = sync_launch_ema_scan(a, s);
  if (e == hipSuccess) e = sync_launch_peak(a, s);
  if (e == hipSuccess) e = sync_launch_scan(a, s);
  if (e == hipSuccess) e = sync_launch_sss(a, s);
  if (e == hipSuccess) e = stage_copy(q->back.host, a.res, bytes, s);
  const hipError_t w = wait_stream(s);
  CHECK_HIP(e);
  CHECK_HIP(w);
  memcpy(res, q->back.host, bytes);
  return MI355_SUCCESS;
}

int clear_state(mi355_sync_t* q)
{
  CHECK_HIP(sync_launch_clear(q->d_avg.as<float>(), (size_t)q->nhyp * q->L, q->d_state.as<SyncState>(), q->nhyp,
                              q->cfg.cp, q->own));
  CHECK_HIP(wait_stream(q->own));
  return MI355_SUCCESS;
}

} // namespace

extern "C" {

int mi355_sync_create(mi355_sync_t** q, const mi355_sync_cfg_t* cfg, int device)
{
  if (!q || !cfg || cfg->fft_size < 64 || cfg->fft_size > SYNC_MAX_FFT || cfg->fft_size % 64 || cfg->max_offset < 2 ||
      cfg->max_offset > (1u << 24) || cfg->n_id_2 > MI355_SYNC_N_ID_2_ALL || cfg->sss_alg > MI355_SSS_DIFF ||
      cfg->cp > MI355_CP_EXT || cfg->frame_type > MI355_TDD || cfg->unsupported)
    return MI355_ERROR_INVALID_INPUTS;
  CHECK_HIP(hipSetDevice(device));
  auto* d   = new mi355_sync;
  d->device = device;
  d->cfg    = *cfg;
  d->nhyp   = cfg->n_id_2 == MI355_SYNC_N_ID_2_ALL ? SYNC_HYPS : 1u;
  d->hyp0   = cfg->n_id_2 == MI355_SYNC_N_ID_2_ALL ? 0u : cfg->n_id_2;
  d->L      = cfg->max_offset + cfg->fft_size + 1; // the reference's buffer_size (pss.c:116)
  const uint32_t      N = cfg->fft_size;
  std::vector<float2> tw(N);
  for (uint32_t m = 0; m < N; m++) {
    const double ang = -2.0 * M_PI * (double)m / (double)N;
    tw[m]            = make_float2((float)std::cos(ang), (float)std::sin(ang));
  }
  std::vector<SssTables> tab(1);
  sss_tables(tab.data());
  if (hipStreamCreateWithFlags(&d->own, hipStreamNonBlocking) != hipSuccess ||
      d->d_pss.upload(pss_replicas(N)) != hipSuccess || d->d_tw.upload(tw) != hipSuccess ||
      d->d_sss.upload(tab) != hipSuccess || d->d_avg.alloc((size_t)d->nhyp * d->L * sizeof(float)) != hipSuccess ||
      d->d_state.alloc(SYNC_HYPS * sizeof(SyncState)) != hipSuccess || clear_state(d) != MI355_SUCCESS) {
    mi355_sync_destroy(d);
    return MI355_ERROR;
  }
  *q = d;
  return MI355_SUCCESS;
}

void mi355_sync_destroy(mi355_sync_t* q)
{
  if (!q) return;
  (void)hipSetDevice(q->device);
  (void)hipDeviceSynchronize();
  if (q->own) (void)hipStreamDestroy(q->own);
  delete q;
}

int mi355_sync_reset(mi355_sync_t* q)
{
  if (!q) return MI355_ERROR_INVALID_INPUTS;
  std::lock_guard<std::mutex> lock(q->mu);
  CHECK_HIP(hipSetDevice(q->device));
  CHECK_HIP(hipDeviceSynchronize()); // a caller's stream may still be reading the state
  return clear_state(q);
}

int mi355_sync_find_batch(mi355_sync_t* q, const mi355_sync_job_t* jobs, uint32_t njobs, uint32_t mode,
                          mi355_sync_res_t* res, void* stream)
{
  if (!q || mode > MI355_SYNC_SEQUENCE || (njobs && (!jobs || !res))) return MI355_ERROR_INVALID_INPUTS;
  if (!njobs) return MI355_SUCCESS;
  std::lock_guard<std::mutex> lock(q->mu);
  CHECK_HIP(hipSetDevice(q->device));
  return run(q, jobs, njobs, mode, res, stream ? (hipStream_t)stream : q->own);
}

} // extern "C"
