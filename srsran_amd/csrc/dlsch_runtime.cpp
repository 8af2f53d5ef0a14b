// srsran_amd/csrc/dlsch_runtime.cpp -- host runtime behind include/srsran_amd/dlsch.h: the decoder object and the decode.
// (The softbuffer pool: softbuffer_pool.cpp; the device tables: dlsch_tables.cpp; the host planning: dlsch_plan.h.)
//
// One call decodes a batch of transport blocks:
//   prologue (TB-CRC bytes zeroed, CBs decoded in an earlier transmission restored)
//   -> rate dematching of every code block into its softbuffer (one launch per K)
//   -> for h in 0 .. max_its-1: MAP half-iteration (finished CBs skipped) -> decision bytes -> CRC check
//   -> epilogue (TB CRC24A, softbuffer data of CRC-ok CBs saved when the TB fails).
// Code blocks are grouped by K (one decoder workspace per K); within a group every CB advances one
// half-iteration per launch, so CRC early stopping is a per-CB skip flag, not a per-CB loop.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <string.h>
#include <vector>

#include "dlsch_object.h"
#include "dlsch_tables.h"
#include "host_env.h"
#include "runtime_internal.h"
#include "tdec8_internal.h"
#include "tdec_internal.h"

using namespace mi355;

// the latency path's limit (process-wide): calls with up to 256 code blocks (srsUE's per-TTI calls carry 1-32; one
// code block per CU, so 256 fill the chip once) decode on tdec_win_lat.  Measured crossover (profiles/r04/
// lat_path_crossover.jsonl, host time per call): the latency path is faster from 16 to 384 code blocks (263 vs 494 us
// at 16, 765 vs 979 at 256); batch workloads of thousands stay on the throughput kernel.  MI355_DLSCH_LAT_CBS overrides
// (0: off); -1: not read yet.
static std::atomic<int> g_lat_cbs{-1};
// device counters of tdec_win_lat's phases (mi355_dlsch_latency_profile): allocated once and never freed, so a decode on
// another thread that snapshotted the pointer before a disarm still writes valid memory; armed = the pointer published
static std::atomic<uint64_t*> g_lat_prof{nullptr};
static uint64_t*              g_lat_prof_mem = nullptr;
static std::mutex             g_lat_prof_mu;
static int lat_cbs_now()
{
  int v = g_lat_cbs.load();
  if (v < 0) {
    v = env_dlsch_lat_cbs();
    g_lat_cbs.store(v);
  }
  return v;
}

// measurement: enable = 1 arms the latency kernel's phase counters (zeroed), 0 disarms; out (nullable, 11 u64): the sums
// since arming (include/srsran_amd/dlsch.h)
extern "C" int mi355_dlsch_latency_profile(int enable, uint64_t* out)
{
  std::lock_guard<std::mutex> lk(g_lat_prof_mu);
  if (out && g_lat_prof.load()) {
    if (hipDeviceSynchronize() != hipSuccess) return MI355_ERROR;
    if (hipMemcpy(out, g_lat_prof_mem, 11 * 8, hipMemcpyDeviceToHost) != hipSuccess) return MI355_ERROR;
  }
  if (enable) {
    if (!g_lat_prof_mem && hipMalloc(&g_lat_prof_mem, 11 * 8) != hipSuccess) return MI355_ERROR;
    if (hipMemset(g_lat_prof_mem, 0, 11 * 8) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return MI355_ERROR;
    g_lat_prof.store(g_lat_prof_mem);
  } else {
    g_lat_prof.store(nullptr);
  }
  return MI355_SUCCESS;
}

extern "C" int mi355_dlsch_set_latency_path(int max_cbs)
{
  const int old = lat_cbs_now();
  if (max_cbs >= 0) g_lat_cbs.store(max_cbs);
  return old;
}

bool mi355::rm_sparse_writes() { return env_rm_sparse() && !env_no_rowmask(); }

extern "C" {

int mi355_dlsch_create(mi355_dlsch_t** q, int device)
{
  if (!q) return MI355_ERROR_INVALID_INPUTS;
  CHECK_HIP(hipSetDevice(device));
  auto* d   = new mi355_dlsch;
  d->device = device;
  const CrcTable t[2] = {make_crc_table(CRC24A_POLY), make_crc_table(CRC24B_POLY)};
  if (hipStreamCreateWithFlags(&d->own, hipStreamNonBlocking) != hipSuccess ||
      d->crc.upload(t, sizeof(t)) != hipSuccess) {
    mi355_dlsch_destroy(d);
    return MI355_ERROR;
  }
  *q = d;
  return MI355_SUCCESS;
}

void mi355_dlsch_destroy(mi355_dlsch_t* q)
{
  if (!q) return;
  (void)hipSetDevice(q->device);
  (void)hipDeviceSynchronize();
  for (auto& kv : q->dec) mi355_tdec_batch_destroy(kv.second);
  for (auto& kv : q->dec8) mi355_tdec8_destroy(kv.second);
  for (int k = 0; k < 2; k++)
    if (q->done_ev[k]) (void)hipEventDestroy(q->done_ev[k]);
  if (q->own) (void)hipStreamDestroy(q->own);
  delete q;
}

int mi355_dlsch_set_max_iterations(mi355_dlsch_t* q, uint32_t max_iterations)
{
  if (!q || max_iterations == 0) return MI355_ERROR_INVALID_INPUTS;
  q->max_its = max_iterations;
  return MI355_SUCCESS;
}

void mi355_dlsch_set_profiling(mi355_dlsch_t* q, int enable)
{
  if (!q) return;
  q->prof = enable != 0;
  for (auto& kv : q->dec) mi355_tdec_batch_set_profiling(kv.second, enable);
}

int mi355_dlsch_kernel_stats(mi355_dlsch_t* q, double* ms, uint32_t* launches)
{
  if (!q) return MI355_ERROR_INVALID_INPUTS;
  double   tot = 0;
  uint32_t n   = 0;
  for (auto& kv : q->dec) {
    double   m = 0;
    uint32_t l = 0;
    int      r = mi355_tdec_batch_kernel_stats(kv.second, &m, &l);
    if (r) return r;
    tot += m;
    n += l;
  }
  if (ms) *ms = tot;
  if (launches) *launches = n;
  return MI355_SUCCESS;
}

int mi355_dlsch_decode_dev(mi355_dlsch_t*           q,
                           mi355_softbuffer_pool_t* pool,
                           const int16_t*           d_e_bits,
                           const mi355_dlsch_tb_t*  tbs,
                           uint32_t                 ntb,
                           uint8_t*                 d_data,
                           int32_t*                 ret,
                           float*                   avg_iterations,
                           void*                    stream)
{
  return mi355::dlsch_decode_dev_hook(q, pool, d_e_bits, tbs, ntb, d_data, ret, avg_iterations, stream, mi355::WaitHook{});
}

int mi355_dlsch_decode8_dev(mi355_dlsch_t* q, mi355_softbuffer_pool_t* pool, const int8_t* d_e_bits,
                            const mi355_dlsch_tb_t* tbs, uint32_t ntb, uint8_t* d_data, int32_t* ret,
                            float* avg_iterations, void* stream)
{
  return mi355::dlsch_decode_dev_hook(q, pool, d_e_bits, tbs, ntb, d_data, ret, avg_iterations, stream,
                                      mi355::WaitHook{}, true);
}

} // extern "C"

// ---------------------------------------------------------------- results: ret | avg from the pinned read-back

// Speculative half-iterations (TdecRun::spec): half-iteration h does not write the next one's input (DEC1: the
// extrinsic E, DEC2: the a-priori A1 -- 12 KB of a K = 6144 code block's ~100 KB of traffic); the code blocks its
// check leaves unfinished run it again (TdecRun::redo).  It pays where at most ~10 % of the code blocks entering h
// fail there (each such block costs a whole half-iteration more), which is judged from the previous batch: its per-TB
// average half-iteration counts (a TB whose blocks all stopped at h averages h + 1).  The last allowed half-iteration
// never needs that input and is always speculative.
static uint32_t spec_policy(const float* avg, const int32_t* ret, uint32_t ntb, uint32_t max_its)
{
  uint32_t mask = 0;
  for (uint32_t h = 0; h + 1 < max_its; h++) {
    uint32_t run = 0, fail = 0;
    for (uint32_t t = 0; t < ntb; t++) {
      if (ret[t] != MI355_SUCCESS && ret[t] != MI355_ERROR) continue; // not decoded
      const float a = avg[t];
      if (!(a > 0.f)) continue;
      run += a > (float)h + 0.5f;
      fail += a > (float)h + 1.5f;
    }
    if (run && fail * 10 <= run) mask |= 1u << h;
  }
  return mask;
}

static size_t rnd256(size_t b) { return (b + 255) / 256 * 256; }
static size_t back_bytes(uint32_t ntb) { return rnd256(ntb * 4) + ntb * 4; } // ret at 0 | avg at rnd256(ntb * 4)

// the call's results from the read-back bytes: ret (the TBs the planner rejected marked), avg (nullable), and the
// decoder's speculation policy refreshed from them
template <class Invalid>
static void take_results(const char* host, uint32_t ntb, Invalid invalid, int32_t* ret, float* avg,
                         std::atomic<uint32_t>* spec_mask, uint32_t max_its)
{
  const char* havg = host + rnd256(ntb * 4);
  memcpy(ret, host, ntb * 4);
  for (uint32_t t = 0; t < ntb; t++) {
    if (invalid(t)) ret[t] = MI355_ERROR_INVALID_INPUTS;
  }
  if (avg) memcpy(avg, havg, ntb * 4);
  if (spec_mask) spec_mask->store(spec_policy((const float*)havg, ret, ntb, max_its));
}

mi355::DlschPending::~DlschPending()
{
  if (armed && ev) (void)hipEventSynchronize(ev);
  if (ev) (void)hipEventDestroy(ev);
  if (host) (void)hipHostFree(host);
}

int mi355::DlschPending::collect()
{
  if (!armed) return MI355_SUCCESS;
  armed = false;
  CHECK_HIP(wait_event(ev));
  take_results(host, ntb, [&](uint32_t t) { return invalid[t] != 0; }, ret, avg, spec_mask, max_its);
  return MI355_SUCCESS;
}

// ---------------------------------------------------------------- one decode call

namespace {

// the call's device scratch, in this order, every part rounded to 256 bytes
struct CallScratch {
  char*     base   = nullptr;
  TbDesc*   d_tb   = nullptr; // staged (one pinned upload): tb | running flags (zeros)
  uint32_t* d_run  = nullptr; // running flags per half-iteration, max_its + 1
  size_t    staged = 0;       // bytes of the staged part
  CbDesc*   d_cb   = nullptr; // per code block (K-grouped, DlschGroup::off): expanded by the prologue
  uint32_t* d_slot = nullptr;
  uint32_t* d_its  = nullptr;
  uint8_t*  d_done = nullptr;
  uint8_t*  d_dec  = nullptr; // decision bytes (DlschGroup::doff)
  int32_t*  d_ret  = nullptr; // per TB: ret | avg read back with one copy
  float*    d_avg  = nullptr;
};

struct Live { // a group ready to decode
  uint32_t            K, off, n;
  uint8_t*            dec;
  const uint32_t*     scale;
  mi355_tdec_batch_t* td  = nullptr; // the 16-bit decoder, or
  mi355_tdec8_t*      t8  = nullptr; // int8 LLRs with an 8-bit window decoder
  bool                lat = false;   // decoded by the latency launch
};

struct Call {
  mi355_dlsch_t*           q;
  mi355_softbuffer_pool_t* pool;
  const void*              d_e_bits;
  uint8_t*                 d_data;
  uint32_t                 ntb;
  hipStream_t              s;
  bool                     llr8, after_s, rm_done;
  uint32_t                 slot = 0; // of q->scratch / done_ev
  CallScratch              m;
  const CrcTable*          crc = nullptr; // [0] CRC24A, [1] CRC24B
  DlschTbArgs              ta{};
  std::vector<Live>        live;
};

} // namespace

// 1. plan: q->plan, and the TB CRC scale tables of the TBs to decode
static int plan_call(Call& c, const mi355_dlsch_tb_t* tbs)
{
  plan_tbs(c.q->plan, tbs, c.ntb, c.pool->nof_sb, c.pool->max_cb, c.llr8);
  for (TbDesc& d : c.q->plan.tbd) {
    if (!d.C) continue;
    if (int e = dlsch_tb_crc_scales(c.q, d.tbs / 8, &d.crc_scale)) return e;
  }
  return MI355_SUCCESS;
}

// 2. scratch: the next of the object's two slots, grown where needed, carved
static int carve_scratch(Call& c)
{
  mi355_dlsch_t*   q  = c.q;
  const DlschPlan& pl = q->plan;
  const size_t     ncb = pl.total_cb;
  // (one rnd256(ncb * 4) more than the carves below take)
  const size_t need = rnd256(c.ntb * sizeof(TbDesc)) + rnd256(4 * (q->max_its + 1)) + rnd256(ncb * sizeof(CbDesc)) +
                      3 * rnd256(ncb * 4) + rnd256(ncb) + rnd256(pl.dec_bytes) + 2 * rnd256(c.ntb * 4);
  c.slot = q->par;
  q->par ^= 1u;
  // an outgrown buffer may still be read by this object's batch in flight: retired, not freed
  bool grew = false;
  CHECK_HIP(q->scratch[c.slot].reserve(need, need + need / 4 + 4096, DevScratch::Retire, &grew));
  if (grew) q->done_armed[c.slot] = false;
  char* p     = q->scratch[c.slot].base();
  auto  carve = [&](size_t b) {
    char* at = p;
    p += rnd256(b);
    return at;
  };
  CallScratch& m = c.m;
  m.base   = p;
  m.d_tb   = (TbDesc*)carve(c.ntb * sizeof(TbDesc));
  m.d_run  = (uint32_t*)carve(4 * (q->max_its + 1));
  m.staged = (size_t)(p - m.base);
  m.d_cb   = (CbDesc*)carve(ncb * sizeof(CbDesc));
  m.d_slot = (uint32_t*)carve(ncb * 4);
  m.d_its  = (uint32_t*)carve(ncb * 4);
  m.d_done = (uint8_t*)carve(ncb);
  m.d_dec  = (uint8_t*)carve(pl.dec_bytes);
  m.d_ret  = (int32_t*)carve(c.ntb * 4);
  m.d_avg  = (float*)carve(c.ntb * 4);
  return MI355_SUCCESS;
}

// 3. upload of the staged part
static int upload_staged(Call& c)
{
  mi355_dlsch_t* q = c.q;
  CHECK_HIP(q->stage.reserve(c.m.staged));
  q->stage.put(q->plan.tbd.data(), c.ntb * sizeof(TbDesc));
  q->stage.zeros(4 * (q->max_its + 1));
  // the batch that last used this slot may still be in flight (after_s): its epilogue, the last reader of the staged
  // part, is done at done_ev[slot]; a slot never used (or just reallocated) needs no wait
  CHECK_HIP(q->stage.upload(c.m.base, c.s, false, c.after_s && q->done_armed[c.slot] ? q->done_ev[c.slot] : nullptr));
  return MI355_SUCCESS;
}

// 4. prologue (its argument block serves the epilogue too)
static int launch_prologue(Call& c)
{
  c.crc = c.q->crc.as<CrcTable>();
  DlschTbArgs& ta = c.ta;
  ta.tb      = c.m.d_tb;
  ta.ntb     = (int)c.ntb;
  ta.data    = c.d_data;
  ta.sb_crc  = c.pool->cb_crc;
  ta.sb_data = c.pool->data;
  ta.ret     = c.m.d_ret;
  ta.crc24a  = &c.crc[0];
  ta.desc    = c.m.d_cb;
  ta.slot    = c.m.d_slot;
  ta.its     = c.m.d_its;
  ta.done    = c.m.d_done;
  ta.running = c.m.d_run;
  ta.avg     = c.m.d_avg;
  CHECK_HIP(dlsch_launch_prologue(ta, c.s));
  return MI355_SUCCESS;
}

// the inverse tables of the redundancy versions present in g
template <class Table> static int rm_inv_tables(const DlschGroup& g, const uint16_t* (&inv)[4], Table table)
{
  for (uint32_t rv = 0; rv < 4; rv++) {
    inv[rv] = nullptr;
    if (!((g.rvmask >> rv) & 1u)) continue;
    if (int r = table(rv, &inv[rv])) return r;
  }
  return MI355_SUCCESS;
}

// 5. group set-up: the group's rate dematching (int16: skipped under rm_done), its decoder workspace and CRC scales
static int setup_group(Call& c, const DlschGroup& g)
{
  mi355_dlsch_t*           q    = c.q;
  mi355_softbuffer_pool_t* pool = c.pool;
  const uint32_t           K = g.K, nsb8 = c.llr8 ? tdec_subblocks_8bit(K) : 0;
  int                      r = 0;
  if (c.llr8) {
    DlschRm8Args ra{};
    ra.desc   = c.m.d_cb + g.off;
    ra.ncb    = (int)g.n;
    ra.N      = 3 * K + 12;
    ra.buflen = rm_buflen_nsb(K, nsb8);
    if ((r = rm_inv_tables(g, ra.inv, [&](uint32_t rv, const uint16_t** o) { return dlsch_rm8_inv(q, K, rv, o); }))) return r;
    ra.e         = (const int8_t*)c.d_e_bits;
    ra.sb        = (int8_t*)pool->buf;
    ra.sb_stride = SB_STRIDE * sizeof(int16_t);
    ra.sb_crc    = pool->cb_crc;
    ra.fresh     = pool->fresh;
    ra.conv      = nsb8 ? nullptr : pool->buf + SB_CONV8;
    CHECK_HIP(dlsch_launch_rm8(ra, c.s));
  } else {
    DlschRmArgs ra{};
    ra.desc   = c.m.d_cb + g.off;
    ra.ncb    = (int)g.n;
    ra.N      = 3 * K + 12;
    ra.buflen = rm_buflen(K);
    if ((r = rm_inv_tables(g, ra.inv, [&](uint32_t rv, const uint16_t** o) { return dlsch_rm16_inv(q, K, rv, o); }))) return r;
    ra.fresh     = pool->fresh;
    ra.e         = (const int16_t*)c.d_e_bits;
    ra.sb        = pool->buf;
    ra.sb_stride = SB_STRIDE;
    ra.sb_crc    = pool->cb_crc;
    ra.fold2     = g.fold2;
    ra.sparse    = rm_sparse_writes() ? 1 : 0;
    if (!c.rm_done) CHECK_HIP(dlsch_launch_rm(ra, c.s));
  }
  Live lv{K, g.off, g.n, c.m.d_dec + g.doff, nullptr};
  if ((r = dlsch_crc_scales(q, K, &lv.scale))) return r;
  if (nsb8) { // int8 LLRs of a window size: the 8-bit decoder; every other group the 16-bit one
    auto it = q->dec8.find(K);
    if (it == q->dec8.end()) {
      mi355_tdec8_t* t8 = nullptr;
      if ((r = mi355_tdec8_create(&t8, q->device))) return r;
      it = q->dec8.emplace(K, t8).first;
    }
    lv.t8 = it->second;
  } else {
    auto it = q->dec.find(K);
    if (it == q->dec.end()) {
      mi355_tdec_batch_t* td = nullptr;
      if ((r = mi355_tdec_batch_create(&td, q->device))) return r;
      mi355_tdec_batch_set_profiling(td, q->prof);
      it = q->dec.emplace(K, td).first;
    }
    lv.td = it->second;
  }
  c.live.push_back(lv);
  return MI355_SUCCESS;
}

// the CRC check of group lv after half-iteration h
static DlschCheckArgs check_args(const Call& c, const Live& lv, uint32_t h)
{
  DlschCheckArgs a{};
  a.desc       = c.m.d_cb + lv.off;
  a.ncb        = (int)lv.n;
  a.K          = lv.K;
  a.h          = h;
  a.max_its    = c.q->max_its;
  a.dec        = lv.dec;
  a.dec_stride = lv.K / 8;
  a.data       = c.d_data;
  a.done       = c.m.d_done + lv.off;
  a.remaining  = c.m.d_run + h;
  a.next       = c.m.d_run + h + 1;
  a.its        = c.m.d_its + lv.off;
  a.sb_crc     = c.pool->cb_crc;
  a.crc24a     = &c.crc[0];
  a.crc24b     = &c.crc[1];
  a.scale      = lv.scale;
  return a;
}

// 6. latency path: a small call decodes each window-decoder group in one launch (tdec_win_lat.hip)
static int launch_latency(Call& c)
{
  if (c.llr8 || c.q->plan.total_cb > (size_t)lat_cbs_now()) return MI355_SUCCESS;
  for (Live& lv : c.live) {
    const uint32_t nsb = mi355_tdec_autoimp_get_subblocks(lv.K);
    if (lv.t8 || nsb == 0 || tdec_lat_lds((int)lv.K, (int)nsb) > 160 * 1024 - 64) continue;
    TdecLatArgs la{};
    la.in        = c.pool->buf;
    la.in_stride = SB_STRIDE;
    la.in_idx    = c.m.d_slot + lv.off;
    if (int r = mi355_tdec_win_tables(lv.td, lv.K, &la.dstE, &la.dstA)) return r;
    la.done    = c.m.d_done + lv.off;
    la.chk     = check_args(c, lv, 0);
    la.prof    = g_lat_prof.load();
    la.ncb     = (int)lv.n;
    la.K       = (int)lv.K;
    la.rowmask = nsb == 16 && !env_no_rowmask();
    la.bwave   = env_lat_waves4() ? 2 : 1;
    la.owaves  = la.bwave == 1 && env_lat_owaves() ? 1 : 0;
    CHECK_HIP(tdec_lat_launch((int)nsb, la, c.s));
    lv.lat = true;
  }
  return MI355_SUCCESS;
}

// after a speculative half-iteration rq: the same again without decisions, writing the next one's input (the a-priori)
// for the code blocks still running at `remaining` (a no-op when none is)
static TdecRun redo_of(TdecRun rq, const uint32_t* remaining)
{
  rq.remaining  = remaining;
  rq.chk        = nullptr;
  rq.chk_fused  = nullptr;
  rq.spec       = false;
  rq.spec_taken = nullptr;
  rq.redo       = true;
  return rq;
}

// 7. half-iteration h of one group: tdec8 or window half-iteration, the check unless fused, the redo when the
// speculation was taken and another half-iteration follows
static int halfit_group(Call& c, const Live& lv, uint32_t h, bool spec)
{
  const DlschCheckArgs ca = check_args(c, lv, h);
  if (lv.t8) {
    T8Batch b{};
    b.in        = (int8_t*)c.pool->buf;
    b.in_stride = SB_STRIDE * sizeof(int16_t);
    b.slot      = c.m.d_slot + lv.off;
    b.done      = c.m.d_done + lv.off;
    b.running   = c.m.d_run + h;
    b.K         = lv.K;
    b.ncb       = lv.n;
    if (int r = tdec8_halfit_batch(lv.t8, b, h, lv.dec, lv.K / 8, c.s)) return r;
    CHECK_HIP(dlsch_launch_check(ca, c.s));
    return MI355_SUCCESS;
  }
  bool    fused = false, taken = false; // fused: the window decoder's decision-byte launch ran the check in its epilogue
  TdecRun rq{};
  rq.in         = c.llr8 ? c.pool->buf + SB_CONV8 : c.pool->buf;
  rq.in_stride  = SB_STRIDE;
  rq.in_idx     = c.m.d_slot + lv.off;
  rq.done       = c.m.d_done + lv.off;
  rq.remaining  = c.m.d_run + h;
  rq.n          = lv.n;
  rq.K          = lv.K;
  rq.h0         = h;
  rq.h1         = h + 1;
  rq.out        = lv.dec;
  rq.out_stride = lv.K / 8;
  rq.stream     = c.s;
  rq.chk        = &ca;
  rq.chk_fused  = &fused;
  rq.spec       = spec;
  rq.spec_taken = &taken;
  rq.rowmask    = !c.llr8 && !env_no_rowmask(); // every 16-bit rate dematcher leaves the slots' parity-row bitmaps
  if (int r = mi355_tdec_run_internal(lv.td, rq)) return r;
  if (!fused) CHECK_HIP(dlsch_launch_check(ca, c.s));
  if (taken && h + 1 < c.q->max_its) return mi355_tdec_run_internal(lv.td, redo_of(rq, c.m.d_run + h + 1));
  return MI355_SUCCESS;
}

static int run_halfits(Call& c)
{
  mi355_dlsch_t* q         = c.q;
  const uint32_t spec_mask = env_tdec_spec() ? q->spec_mask.load() : 0u;
  for (uint32_t h = 0; h < q->max_its; h++) {
    const bool spec = h + 1 == q->max_its || ((spec_mask >> h) & 1u);
    for (const Live& lv : c.live) {
      if (lv.lat) continue;
      if (int r = halfit_group(c, lv, h, spec)) return r;
    }
  }
  return MI355_SUCCESS;
}

// 8. epilogue; done_ev[slot]: the last reader of the slot's staged part has run
static int launch_epilogue(Call& c)
{
  mi355_dlsch_t* q = c.q;
  CHECK_HIP(dlsch_launch_epilogue(c.ta, c.s));
  if (!q->done_ev[c.slot]) CHECK_HIP(hipEventCreateWithFlags(&q->done_ev[c.slot], hipEventDisableTiming));
  CHECK_HIP(hipEventRecord(q->done_ev[c.slot], c.s));
  q->done_armed[c.slot] = true;
  return MI355_SUCCESS;
}

// 9a. results left in flight: the read-back into the pending object's own pinned buffer, collect() takes them
static int read_back_pending(Call& c, DlschPending* pend, int32_t* ret, float* avg)
{
  mi355_dlsch_t* q     = c.q;
  const size_t   bytes = back_bytes(c.ntb);
  if (bytes > pend->cap) {
    if (pend->host) (void)hipHostFree(pend->host);
    pend->host = nullptr;
    pend->cap  = 0;
    CHECK_HIP(stage_host_alloc((void**)&pend->host, bytes + bytes / 2 + 4096));
    pend->cap = bytes + bytes / 2 + 4096;
  }
  if (!pend->ev) CHECK_HIP(hipEventCreateWithFlags(&pend->ev, hipEventDisableTiming));
  CHECK_HIP(stage_copy(pend->host, c.m.d_ret, bytes, c.s));
  CHECK_HIP(hipEventRecord(pend->ev, c.s));
  pend->invalid.resize(c.ntb);
  for (uint32_t t = 0; t < c.ntb; t++) pend->invalid[t] = q->plan.tbd[t].invalid ? 1 : 0;
  pend->ntb       = c.ntb;
  pend->avg_off   = rnd256(c.ntb * 4);
  pend->ret       = ret;
  pend->avg       = avg;
  pend->spec_mask = &q->spec_mask;
  pend->max_its   = q->max_its;
  pend->armed     = true;
  return MI355_SUCCESS;
}

// 9b. the caller's host work, then the read-back into the object's pinned buffer, waited for
static int read_back_now(Call& c, WaitHook hook, int32_t* ret, float* avg)
{
  mi355_dlsch_t* q = c.q;
  if (hook.fn) hook.fn(hook.ctx);
  CHECK_HIP(q->back.reserve(back_bytes(c.ntb)));
  CHECK_HIP(stage_copy(q->back.host, c.m.d_ret, back_bytes(c.ntb), c.s));
  CHECK_HIP(wait_stream(c.s));
  const TbDesc* tbd = q->plan.tbd.data();
  take_results(q->back.host, c.ntb, [&](uint32_t t) { return tbd[t].invalid != 0; }, ret, avg, &q->spec_mask, q->max_its);
  return MI355_SUCCESS;
}

int mi355::dlsch_decode_dev_hook(mi355_dlsch_t* q, mi355_softbuffer_pool_t* pool, const void* d_e_bits,
                                 const mi355_dlsch_tb_t* tbs, uint32_t ntb, uint8_t* d_data, int32_t* ret,
                                 float* avg_iterations, void* stream, mi355::WaitHook hook, bool llr8,
                                 mi355::DlschPending* pend, bool after_s, bool rm_done)
{
  if (!q || !pool || !tbs || !ret || (ntb && !d_e_bits)) return MI355_ERROR_INVALID_INPUTS;
  if (ntb == 0) return MI355_SUCCESS;
  if (pend && pend->armed) return MI355_ERROR; // not collected: nothing is planned or launched
  std::lock_guard<std::mutex> lock(q->mu);
  const bool     prof = env_host_prof();
  const HostTime t0   = host_now();
  CHECK_HIP(hipSetDevice(q->device));
  Call c{q, pool, d_e_bits, d_data, ntb, stream ? (hipStream_t)stream : q->own, llr8, after_s, rm_done};
  int  r = 0;
  if ((r = plan_call(c, tbs))) return r;
  if ((r = carve_scratch(c))) return r;
  if ((r = upload_staged(c))) return r;
  if ((r = launch_prologue(c))) return r;
  c.live.reserve(q->plan.groups.size());
  for (const DlschGroup& g : q->plan.groups)
    if ((r = setup_group(c, g))) return r;
  if ((r = launch_latency(c))) return r;
  if ((r = run_halfits(c))) return r;
  if ((r = launch_epilogue(c))) return r;
  const HostTime t1 = host_now();
  if (pend) return read_back_pending(c, pend, ret, avg_iterations);
  if ((r = read_back_now(c, hook, ret, avg_iterations))) return r;
  if (prof)
    fprintf(stderr, "[mi355 host] dlsch_decode_dev: plan+launch %.1f us, wait+readback %.1f us\n", host_us(t0, t1),
            host_us(t1, host_now()));
  return MI355_SUCCESS;
}
