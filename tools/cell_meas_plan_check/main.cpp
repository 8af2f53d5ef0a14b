// tools/cell_meas_plan_check/main.cpp -- stand-alone host check of srsran_amd/csrc/cell_meas_plan.h, built with the
// address and undefined-behaviour sanitizers by tests/test_cell_meas_plan_host.py.  No GPU, no HIP headers.
//
// What it checks:
//   * the input contract: nsamples = m sf_len with 2 <= m <= max_nof_sf, a cell of the list, a non-null input; one bad
//     job anywhere fails the whole plan and leaves no group behind;
//   * the block count of find_peak's loop: min(nsamples - sf_len, 10 sf_len) / sf_len, so 1 block for m = 2 and 10 from
//     m = 11 on;
//   * the grouping: every job in exactly one group, a group's jobs share (input, nsamples), at most CM_CELLS to a group,
//     no group more than needed; whatever the order of the jobs, the same set of jobs per capture and the same number
//     of groups (which jobs of a capture share a group follows their order of appearance);
//   * the brute-force list of 504 cells on one capture: 126 full groups.
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <random>
#include <set>
#include <vector>

#include "cell_meas_plan.h"

using namespace mi355;

#define REQUIRE(x)                                                                                                     \
  do {                                                                                                                 \
    if (!(x)) {                                                                                                        \
      fprintf(stderr, "cell_meas_plan_check: %s:%d: %s\n", __FILE__, __LINE__, #x);                                    \
      exit(1);                                                                                                         \
    }                                                                                                                  \
  } while (0)

static void check_groups(const std::vector<mi355_cell_meas_job_t>& jobs, const std::vector<CmGroup>& groups,
                         uint32_t sf_len)
{
  std::vector<int>                                       seen(jobs.size(), 0);
  std::map<std::pair<const void*, uint32_t>, uint32_t> per_capture, groups_of;
  for (const auto& j : jobs) per_capture[{j.input, j.nsamples}]++;
  for (const CmGroup& g : groups) {
    REQUIRE(g.ncell >= 1 && g.ncell <= CM_CELLS);
    REQUIRE(g.nblocks == cm_nblocks(g.nsamples, sf_len) && g.nblocks >= 1 && g.nblocks <= CM_MAX_BLOCKS);
    groups_of[{g.in, g.nsamples}]++;
    for (uint32_t c = 0; c < g.ncell; c++) {
      REQUIRE(g.job[c] < jobs.size());
      const auto& j = jobs[g.job[c]];
      REQUIRE(j.input == g.in && j.nsamples == g.nsamples && j.cell == g.cell[c]);
      seen[g.job[c]]++;
    }
  }
  for (int s : seen) REQUIRE(s == 1);
  for (const auto& kv : per_capture) REQUIRE(groups_of[kv.first] == (kv.second + CM_CELLS - 1) / CM_CELLS);
}

int main()
{
  const uint32_t sf_len = 1920, max_sf = 12, ncells = 504;
  static float   cap[4][8]; // stand-ins for captures: only their addresses are used
  std::vector<CmGroup> groups;

  // the contract
  const mi355_cell_meas_job_t good{cap[0], 6 * sf_len, 3};
  REQUIRE(cm_job_ok(good, sf_len, max_sf, ncells));
  for (uint32_t ns : {0u, sf_len, sf_len + 1, 2 * sf_len - 1, 2 * sf_len + 1, 13 * sf_len, 6 * sf_len + 960}) {
    mi355_cell_meas_job_t j = good;
    j.nsamples              = ns;
    REQUIRE(!cm_job_ok(j, sf_len, max_sf, ncells));
  }
  for (uint32_t m = 2; m <= max_sf; m++) {
    mi355_cell_meas_job_t j = good;
    j.nsamples              = m * sf_len;
    REQUIRE(cm_job_ok(j, sf_len, max_sf, ncells));
    REQUIRE(cm_nblocks(j.nsamples, sf_len) == (m - 1 < 10 ? m - 1 : 10));
    REQUIRE(cm_limited(j.nsamples, sf_len) == cm_nblocks(j.nsamples, sf_len) * sf_len);
  }
  {
    mi355_cell_meas_job_t j = good;
    j.cell                  = ncells;
    REQUIRE(!cm_job_ok(j, sf_len, max_sf, ncells));
    j       = good;
    j.input = nullptr;
    REQUIRE(!cm_job_ok(j, sf_len, max_sf, ncells));
    REQUIRE(!cm_job_ok(good, 0, max_sf, ncells));
  }
  REQUIRE(cm_ntiles(1920) == 2 && cm_ntiles(1024) == 1 && cm_ntiles(1025) == 2 && cm_ntiles(23040) == 23);
  REQUIRE(cm_symbol_sz(6) == 128 && cm_symbol_sz(15) == 256 && cm_symbol_sz(25) == 384 && cm_symbol_sz(100) == 1536 &&
          cm_symbol_sz(0) == 0 && cm_symbol_sz(111) == 0);

  // one bad job fails the plan
  {
    std::vector<mi355_cell_meas_job_t> jobs(9, good);
    jobs[7].nsamples = 6 * sf_len + 1;
    REQUIRE(!cm_plan(jobs.data(), (uint32_t)jobs.size(), sf_len, max_sf, ncells, groups) && groups.empty());
    jobs[7] = good;
    REQUIRE(cm_plan(jobs.data(), (uint32_t)jobs.size(), sf_len, max_sf, ncells, groups) && groups.size() == 3);
    check_groups(jobs, groups, sf_len);
    REQUIRE(cm_plan(jobs.data(), 0, sf_len, max_sf, ncells, groups) && groups.empty());
  }

  // brute force: 504 cells on one capture
  {
    std::vector<mi355_cell_meas_job_t> jobs;
    for (uint32_t c = 0; c < 504; c++) jobs.push_back({cap[1], 6 * sf_len, c});
    REQUIRE(cm_plan(jobs.data(), 504, sf_len, max_sf, ncells, groups) && groups.size() == 126);
    check_groups(jobs, groups, sf_len);
    for (const CmGroup& g : groups) REQUIRE(g.ncell == CM_CELLS && g.nblocks == 5);
  }

  // random mixes; the same jobs per capture and as many groups whatever the order
  std::mt19937 rng(1);
  for (int trial = 0; trial < 200; trial++) {
    std::vector<mi355_cell_meas_job_t> jobs(1 + rng() % 40);
    for (auto& j : jobs) j = {cap[rng() % 4], (2 + rng() % 3) * sf_len, (uint32_t)(rng() % ncells)};
    REQUIRE(cm_plan(jobs.data(), (uint32_t)jobs.size(), sf_len, max_sf, ncells, groups));
    check_groups(jobs, groups, sf_len);
    // the jobs of each capture as a multiset of cells: the same from the shuffled list
    auto per_capture = [](const std::vector<CmGroup>& gs) {
      std::map<std::pair<const void*, uint32_t>, std::multiset<uint32_t>> m;
      for (const CmGroup& g : gs)
        for (uint32_t c = 0; c < g.ncell; c++) m[{g.in, g.nsamples}].insert(g.cell[c]);
      return m;
    };
    std::vector<uint32_t> perm(jobs.size());
    for (size_t i = 0; i < perm.size(); i++) perm[i] = (uint32_t)i;
    std::shuffle(perm.begin(), perm.end(), rng);
    std::vector<mi355_cell_meas_job_t> shuffled;
    for (uint32_t p : perm) shuffled.push_back(jobs[p]);
    std::vector<CmGroup> g2;
    REQUIRE(cm_plan(shuffled.data(), (uint32_t)shuffled.size(), sf_len, max_sf, ncells, g2));
    check_groups(shuffled, g2, sf_len);
    REQUIRE(g2.size() == groups.size());
    REQUIRE(per_capture(g2) == per_capture(groups));
  }
  printf("cell_meas_plan_check: OK\n");
  return 0;
}
