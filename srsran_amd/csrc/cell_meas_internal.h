// srsran_amd/csrc/cell_meas_internal.h -- descriptors shared by the neighbour-cell measurement kernels
// (cell_meas_kernels.hip) and their host runtime (cell_meas_runtime.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/srsran_amd/cell_meas.h"
#include "../../include/srsran_amd/tdec.h"
#include "cell_meas_plan.h"

namespace mi355 {

constexpr uint32_t CM_KT     = 128; // taps staged in LDS at a time (every sf_len is a multiple)
constexpr uint32_t CM_LPT    = 4;   // lags per thread: CM_TILE / 256
constexpr uint32_t CM_SF_LDS = 16;  // subframes whose symbol correlations the measure kernel keeps in LDS at a time

// the cell as the grid kernel needs it
struct CmCellDev {
  uint32_t id, nof_ports;
};

// what a correlation workgroup leaves per (job, block, lag tile)
struct CmPartial {
  double   pmax; // max |c|^2
  double   psum; // sum |c|^2
  uint32_t arg;  // lowest lag (within the block) of the maximum
  uint32_t pad;
};

// what the measure kernel leaves per job beside the per-subframe records
struct CmHead {
  float    peak_value, rms_avg;
  uint32_t stage1_peak, stage1_found, peak_shifted;
  int32_t  peak_idx; // what find_peak returns
  uint32_t sf_count, pad;
};

struct CmJobDev {
  const float2* in;
  uint32_t      nsamples, cell;
};

struct CmSfJobDev {
  const float2* in;
  uint32_t      cell, sf_idx;
};

struct CmArgs {
  const float2*         seq;      // [cell][10][sf_len]
  const CmGroup*        groups;
  const CmJobDev*       jobs;
  CmPartial*            part;     // [job][CM_MAX_BLOCKS][ntiles]
  CmHead*               head;     // [job]
  mi355_cell_meas_sf_t* sf;       // [job][max_nof_sf]
  uint32_t              njobs, ngroups, max_blocks;
  uint32_t              nof_prb, N, cp0, cp1, sf_len, ntiles, max_nof_sf;
  uint32_t              stage2;   // 0: find_peak only
};

struct CmGridArgs {
  const CmCellDev* cells;  // [n] of this chunk
  const float2*    pilots; // [n][2][10][4 * 2 nof_prb]
  const float2*    pss;    // [3][62]
  const float*     sss;    // [n][2][62]
  float2*          grids;  // [n][10][14 * nre]
  uint32_t         n, nof_prb;
};

hipError_t cm_launch_grid(const CmGridArgs& a, hipStream_t s);
hipError_t cm_launch_corr(const CmArgs& a, hipStream_t s);
hipError_t cm_launch_measure(const CmArgs& a, hipStream_t s);
hipError_t cm_launch_measure_sf(const CmArgs& a, const CmSfJobDev* jobs, uint32_t n, mi355_cell_meas_sf_t* out,
                                hipStream_t s);

} // namespace mi355
