// srsran_amd/csrc/pdsch_object.h -- the object behind include/srsran_amd/pdsch.h, the plans of a call and what the
// receiver's translation units share: pdsch_maps.cpp (the two device caches), pdsch_eqrm.cpp (pdsch_eq_rm's plan),
// pdsch_frontend.cpp (layout, upload, launches) and pdsch_runtime.cpp (create / setters, job planning, the decode).
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/srsran_amd/dlsch.h"
#include "../../include/srsran_amd/pdsch.h"
#include "../../include/srsran_amd/tdec.h"
#include "device_mem.h"
#include "host_staging.h"
#include "pdsch_internal.h"
#include "runtime_internal.h"

namespace mi355 {

// RE extraction map of one (allocation, cfi, subframe) in HBM: the image of pdsch_re_map.h
struct MapEntry {
  uint16_t* d = nullptr;
  uint32_t  n = 0, g0 = 0, g1 = 0, ncols = 0;
  const uint16_t* inv() const { return d + ((n + 1) & ~1u); }
  const uint16_t* cols() const { return inv() + (g1 - g0); } // distinct subcarriers of the REs
};
// the cache's entry: the map and the buffer d points into (recycled through map_free, trim_maps)
struct MapSlot : MapEntry {
  DevMem mem;
};

struct JobPlan {
  PdschJobDev dev{};
  uint32_t    cw_of_tb[2]{};
  size_t      d_off[2]{}, e_off[2]{}; // element offsets in the arenas (d_off: symbols and their csi alike)
  bool        decode[2]{};
};

// a batch decoded through pdsch_eq_rm (pdsch_internal.h)
struct EqRmPlan {
  std::vector<EqRmJob> rj;
  uint32_t             max_c = 0, img = 0, cimg = 0;
  EqRmPool             pool{};
};

} // namespace mi355

struct mi355_pdsch {
  int                                  device = 0;
  std::unique_ptr<mi355::PdschPending> api_pend;          // mi355_pdsch_decode_launch's results in flight
  bool                                 api_armed = false;
  mi355_cell_t                         cell{};
  uint32_t                             nof_rx = 1;
  hipStream_t                          own    = nullptr;
  mi355_dlsch_t*                       dlsch  = nullptr;
  uint32_t                             max_its = 10; // SRSLTE_PDSCH_MAX_TDEC_ITERS
  mi355::DevMem                        gold; // uint32_t
  mi355::DevCache<std::string, mi355::MapSlot> maps; // extraction maps in HBM
  // the previous lookup per subframe index (get_map's key): a batch of consecutive subframes cycles through them
  mi355::MapEntry                      last_map[10]{};
  uint32_t                             last_map_hdr[10][4]{};
  uint8_t                              last_map_prb[10][2][MI355_MAX_PRB]{};
  // packed descrambling sequences per c_init
  mi355::DevCache<uint32_t, mi355::DevMem, std::unordered_map<uint32_t, mi355::DevMem>> scr;
  // bounds of the two caches, checked once per call before planning (mi355_pdsch_debug_set_cache_limits)
  uint32_t                             max_maps = 8192, max_scr = 4096;
  mi355::DevScratch                    scratch;
  // evicted extraction maps' buffers: freed at destroy (hipFree waits for the whole device, which would stall every
  // other worker's stream) and reused for new maps
  std::vector<mi355::DevMem>           map_free;
  std::vector<mi355::JobPlan>          last; // plans of the last call (debug_stage)
  float2*                              d_arena   = nullptr;
  float*                               csi_arena = nullptr;
  int16_t*                             e_arena   = nullptr;
  bool                                 llr8      = false; // pdsch.llr_is_8bit (srsUE pdsch_8bit_decoder)
  bool                                 ce_inv    = false; // mi355_pdsch_set_ce_invariant
  mi355::HostStaging                   stage;
  hipEvent_t                           fe_done  = nullptr; // after the last front-end kernel of the previous batch
  bool                                 fe_armed = false;
  // the last batch went through pdsch_eq_rm, which leaves no LLRs in e: mi355_pdsch_debug_stage produces them once,
  // on demand, with pdsch_eq_llr over the same descriptors (still in the scratch until the next batch)
  bool                                 e_pending = false;
  const mi355::PdschJobDev*            last_jobs_dev = nullptr;
  uint32_t                             last_njobs = 0, last_max_fpairs = 0;
  std::vector<uint32_t>                last_fkeys;
  std::mutex                           mu;
};

namespace mi355 {

// The caller of these holds q->mu and has set the device.
// pdsch_maps.cpp: the bounds (once per call, before planning) and the look-ups of the two caches
int trim_maps(mi355_pdsch_t* q);
int get_map(mi355_pdsch_t* q, const mi355_pdsch_grant_t& g, uint32_t cfi, uint32_t sf, MapEntry* out);
int trim_scr(mi355_pdsch_t* q, hipStream_t s);
// *fresh: the sequence is still to be generated into *d (pdsch_launch_scr_pack)
int get_scr(mi355_pdsch_t* q, uint32_t c_init, uint32_t** d, bool* fresh);
// pdsch_eqrm.cpp: whether the whole batch goes through pdsch_eq_rm, and then its plan
bool plan_eq_rm(mi355_pdsch_t* q, mi355_softbuffer_pool_t* pool, const mi355_pdsch_job_t* jobs,
                const std::vector<JobPlan>& plans, EqRmPlan& er);
// pdsch_frontend.cpp: front end over planned jobs; fills plans' d_off / e_off and device pointers and runs the
// equaliser and LLR kernels on s (er: pdsch_eq_rm instead, LLRs and rate dematching included)
int run_frontend(mi355_pdsch_t* q, const mi355_pdsch_job_t* jobs, std::vector<JobPlan>& plans, hipStream_t s,
                 bool after_s = false, const EqRmPlan* er = nullptr);

} // namespace mi355
