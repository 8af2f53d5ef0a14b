// srsran_amd/csrc/dlsch_object.h -- the objects behind include/srsran_amd/dlsch.h and what their translation units
// share: softbuffer_pool.cpp (the pool), dlsch_tables.cpp (the cached device tables) and dlsch_runtime.cpp (create /
// setters, the latency-path limit and profiler, the decode).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <map>
#include <mutex>

#include "../../include/srsran_amd/dlsch.h"
#include "../../include/srsran_amd/tdec.h"
#include "device_mem.h"
#include "dlsch_internal.h"
#include "dlsch_plan.h"
#include "host_staging.h"

struct mi355_softbuffer_pool {
  int      device = 0;
  uint32_t nof_sb = 0, max_cb = 0;
  int16_t* buf    = nullptr; // nof_sb * max_cb * SB_STRIDE
  uint8_t* cb_crc = nullptr; // nof_sb * max_cb
  uint8_t* data   = nullptr; // nof_sb * max_cb * SB_DATA
  uint8_t* fresh  = nullptr; // nof_sb * max_cb: buffer logically zero (lazy reset)
  // batched reset lists {softbuffer, code blocks to reset}, two in turn: a call's list upload waits only for the
  // reset kernel that read the same buffer two calls ago (ev_list), not for everything queued before it
  mi355::DevMem d_list[2]; // uint2
  uint32_t   list_cap[2] = {0, 0};
  hipEvent_t ev_list[2]  = {nullptr, nullptr};
  bool       ev_armed[2] = {false, false};
  uint32_t   lpar        = 0;
  mi355::HostStaging st_list;
};

struct mi355_dlsch {
  int                                     device = 0;
  hipStream_t                             own    = nullptr;
  uint32_t                                max_its = 10; // SRSLTE_PDSCH_MAX_TDEC_ITERS, sch.c:35
  std::map<uint32_t, mi355_tdec_batch_t*> dec;          // one decoder workspace per K
  mi355::DevCache<uint64_t>               rm;           // (K << 2 | rv) -> device table (uint16_t)
  mi355::DevCache<uint64_t>               rm8;          // the same for the 8-bit decoder layout
  struct Compact {
    mi355::DevMem d; // uint16_t
    uint32_t      nq = 0, qoff = 0;
  };
  mi355::DevCache<uint64_t, Compact>      rmc;          // (K, rv, E) -> compact image table (dlsch_rm_compact)
  std::map<uint32_t, mi355_tdec8_t*>      dec8;         // 8-bit decoder workspace per K
  mi355::DevCache<uint32_t>               scales;       // K -> per-lane CRC scale factors (uint32_t)
  mi355::DevCache<uint32_t>               tb_scales;    // TB bytes -> per-thread CRC24A scale factors (epilogue)
  mi355::DevMem                           crc;          // CrcTable [0] CRC24A, [1] CRC24B
  // per-call scratch, two in turn: a call's descriptor upload waits only for the epilogue of the call before last
  // (done_ev of the same slot, the last reader of its staged part), so a batch enqueued behind one still in flight
  // (find_and_decode's second chunk) uploads at once instead of at the first one's end
  mi355::DevScratch scratch[2];
  hipEvent_t        done_ev[2]    = {nullptr, nullptr};
  bool              done_armed[2] = {false, false};
  uint32_t          par           = 0;
  std::mutex        mu;
  bool              prof = false;
  mi355::DlschPlan   plan; // the call's host plan (under mu), kept for its vectors' capacity
  mi355::HostStaging stage;
  mi355::HostStaging back; // pinned read-back of ret | avg
  // bit h: half-iteration h runs speculatively (spec_policy); until a batch has been seen, the first DEC2
  std::atomic<uint32_t> spec_mask{1u << 1};
};

namespace mi355 {

// The cached device tables of a decoder object (dlsch_tables.cpp; built by dlsch_tables.h on first use).  The caller
// holds q->mu and has set the device.
int dlsch_rm16_inv(mi355_dlsch_t* q, uint32_t K, uint32_t rv, const uint16_t** out); // rm16_table
int dlsch_rm8_inv(mi355_dlsch_t* q, uint32_t K, uint32_t rv, const uint16_t** out);  // rm8_inv_table
int dlsch_crc_scales(mi355_dlsch_t* q, uint32_t K, const uint32_t** out);            // crc_scales_table
// Never evicted: descriptors planned earlier in the same call hold their pointers, and the cache is bounded by the
// distinct TB byte counts a decoder ever sees (1 KB each; every size up to the largest TBS would be 48 MB, the LTE
// tables' 190 distinct sizes 190 KB).
int dlsch_tb_crc_scales(mi355_dlsch_t* q, uint32_t nbytes, const uint32_t** out);    // tb_crc_scales_table

} // namespace mi355
