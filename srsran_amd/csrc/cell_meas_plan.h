// srsran_amd/csrc/cell_meas_plan.h -- host-only rules of the neighbour-cell measurement: the input contract of a job,
// the block count of the stage-1 correlation and the grouping of the jobs by capture, so that the samples of a block go
// through LDS once for all the cells of a group.  No HIP here: tools/cell_meas_plan_check builds this header alone.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <functional>
#include <numeric>
#include <vector>

#include "../../include/srsran_amd/cell_meas.h"

#ifdef __HIPCC__
#define CM_HD __host__ __device__
#else
#define CM_HD
#endif

namespace mi355 {

constexpr uint32_t CM_CELLS      = 4;    // cells a correlation workgroup serves from one staging of the samples
constexpr uint32_t CM_TILE       = 1024; // lags per correlation workgroup
constexpr uint32_t CM_MAX_BLOCKS = 10;   // SRSLTE_NOF_SF_X_FRAME: the correlation covers a frame or less

// srslte_symbol_sz (phy_common.c:353-380) with the non-standard rates the reference defaults to
inline uint32_t cm_symbol_sz(uint32_t nof_prb)
{
  static const uint32_t lim[6] = {6, 15, 25, 50, 75, 110};
  static const uint32_t ns[6]  = {128, 256, 384, 768, 1024, 1536};
  if (nof_prb == 0) return 0;
  for (int i = 0; i < 6; i++)
    if (nof_prb <= lim[i]) return ns[i];
  return 0;
}

// samples the block loop of find_peak covers (refsignal_dl_sync.c:313) and its number of blocks
CM_HD inline uint32_t cm_limited(uint32_t nsamples, uint32_t sf_len)
{
  return nsamples - sf_len < CM_MAX_BLOCKS * sf_len ? nsamples - sf_len : CM_MAX_BLOCKS * sf_len;
}
CM_HD inline uint32_t cm_nblocks(uint32_t nsamples, uint32_t sf_len) { return (cm_limited(nsamples, sf_len) + sf_len - 1) / sf_len; }
CM_HD inline uint32_t cm_ntiles(uint32_t sf_len) { return (sf_len + CM_TILE - 1) / CM_TILE; }

// nsamples = m sf_len, 2 <= m <= max_nof_sf; a cell of the list; an input
inline bool cm_job_ok(const mi355_cell_meas_job_t& j, uint32_t sf_len, uint32_t max_nof_sf, uint32_t ncells)
{
  if (!j.input || !sf_len || j.nsamples % sf_len) return false;
  const uint32_t m = j.nsamples / sf_len;
  return m >= 2 && m <= max_nof_sf && j.cell < ncells;
}

// up to CM_CELLS jobs on one capture
struct CmGroup {
  const void* in;
  uint32_t    nsamples, nblocks, ncell, pad;
  uint32_t    cell[CM_CELLS], job[CM_CELLS];
};

// Validates every job, then groups them: jobs with the same (input, nsamples) in their order of appearance, CM_CELLS to
// a group.  Every job lands in exactly one group.  false: a job breaks the contract and groups is left empty.
inline bool cm_plan(const mi355_cell_meas_job_t* jobs, uint32_t njobs, uint32_t sf_len, uint32_t max_nof_sf,
                    uint32_t ncells, std::vector<CmGroup>& groups)
{
  groups.clear();
  for (uint32_t i = 0; i < njobs; i++)
    if (!cm_job_ok(jobs[i], sf_len, max_nof_sf, ncells)) return false;
  std::vector<uint32_t> order(njobs);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    if (jobs[a].input != jobs[b].input) return std::less<const void*>()(jobs[a].input, jobs[b].input);
    return jobs[a].nsamples < jobs[b].nsamples;
  });
  for (uint32_t k = 0; k < njobs; k++) {
    const mi355_cell_meas_job_t& j = jobs[order[k]];
    if (groups.empty() || groups.back().ncell == CM_CELLS || groups.back().in != j.input ||
        groups.back().nsamples != j.nsamples) {
      CmGroup g{};
      g.in       = j.input;
      g.nsamples = j.nsamples;
      g.nblocks  = cm_nblocks(j.nsamples, sf_len);
      groups.push_back(g);
    }
    CmGroup& g        = groups.back();
    g.cell[g.ncell]   = j.cell;
    g.job[g.ncell++]  = order[k];
  }
  return true;
}

} // namespace mi355
