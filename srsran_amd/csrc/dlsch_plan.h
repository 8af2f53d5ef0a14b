// srsran_amd/csrc/dlsch_plan.h -- host planning of one DL-SCH decode call (sch.c:363-401, 503-530) over plain data:
// per TB its segmentation and its place in the K-grouped code-block arrays (the code-block descriptors themselves are
// expanded on the device by the prologue), per K one group.  Host-only, no HIP (tools/dlsch_plan_check runs it on the
// CPU).
#pragma once
#include <algorithm>
#include <stdint.h>
#include <vector>

#include "../../include/srsran_amd/dlsch.h"
#include "dlsch_layout.h"
#include "rm_tables.h"

namespace mi355 {

// the code blocks of one K: one rate-dematching launch and one decoder workspace
struct DlschGroup {
  uint32_t K, n;   // code-block size, code blocks
  uint32_t rvmask; // redundancy versions present (bit rv)
  uint32_t fold2;  // LDS pairs of the rate dematcher: max over the members of (min(E_max, N) + 1) / 2
  uint32_t off;    // first code block in the call's CB arrays
  size_t   doff;   // first byte in the call's decision bytes (n * K / 8 per group)
};

struct DlschPlan {
  std::vector<TbDesc>     tbd;    // per TB; crc_scale (a device pointer) is left null for the caller to fill where C > 0
  std::vector<DlschGroup> groups; // first-seen order, K1 before K2 within a TB: every CB index depends on it
  std::vector<uint8_t>    grp;    // (scratch of plan_tbs: the K1 / K2 group of each TB)
  size_t                  total_cb = 0, dec_bytes = 0;
};

// int8 LLRs: the 8-bit window decoders, or K <= 400 through the 16-bit generic one (turbodecoder.c:458-483);
// 400 < K <= 800 would decode a partly unconverted buffer in the reference
inline bool dlsch_k_ok8(uint32_t K) { return tdec_subblocks_8bit(K) >= 16 || K <= 400; }

// Fills p (its vectors keep their capacity from call to call).  A TB is marked invalid for a softbuffer out of range,
// rv > 3, Qm = 0 or a segmentation error; tbs = 0 succeeds with nothing to decode (C = 0); then filler bits or
// C > max_cb are invalid (sch.c:517-527), and with llr8 a code-block size the 8-bit mode cannot decode.
inline void plan_tbs(DlschPlan& p, const mi355_dlsch_tb_t* tbs, uint32_t ntb, uint32_t nof_sb, uint32_t max_cb, bool llr8)
{
  p.tbd.assign(ntb, TbDesc{});
  p.grp.assign(2 * (size_t)ntb, 0);
  p.groups.clear();
  auto group_of = [&](uint32_t K) {
    for (uint32_t i = 0; i < p.groups.size(); i++)
      if (p.groups[i].K == K) return i;
    p.groups.push_back(DlschGroup{K, 0, 0, 0, 0, 0}); // few distinct K
    return (uint32_t)p.groups.size() - 1;
  };
  uint32_t seg_tbs = UINT32_MAX;
  CbSegm   seg{};
  int      seg_err = 0;
  for (uint32_t t = 0; t < ntb; t++) {
    const mi355_dlsch_tb_t& in = tbs[t];
    TbDesc&                 d  = p.tbd[t];
    d.tbs                      = in.tbs;
    d.data_off                 = in.data_offset;
    if (in.tbs != seg_tbs) {
      seg_err = cbsegm(in.tbs, &seg);
      seg_tbs = in.tbs;
    }
    if (in.softbuffer >= nof_sb || in.rv > 3 || in.Qm == 0 || seg_err) {
      d.invalid = 1;
      continue;
    }
    if (in.tbs == 0 || seg.C == 0) continue; // nothing to decode: success
    if (seg.F || seg.C > max_cb) {           // sch.c:517-527
      d.invalid = 1;
      continue;
    }
    if (llr8 && ((seg.C1 && !dlsch_k_ok8(seg.K1)) || (seg.C > seg.C1 && !dlsch_k_ok8(seg.K2)))) {
      d.invalid = 1;
      continue;
    }
    d.C          = seg.C;
    d.C1         = seg.C1;
    d.K1         = seg.K1;
    d.K2         = seg.K2;
    d.slot0      = in.softbuffer * max_cb;
    d.Qm         = in.Qm;
    d.nof_e_bits = in.nof_e_bits;
    d.rv         = in.rv;
    d.e_off      = in.e_offset;
    // the largest E of the TB's code blocks (sch.c:391-401: Qm * (G' / C), +Qm for the last gamma), for the rate
    // dematcher's LDS image (min(E, N) per code block)
    const uint32_t emax = in.Qm * (in.nof_e_bits / in.Qm / seg.C + 1);
    auto           join = [&](uint32_t which, uint32_t K, uint32_t ncb) {
      const uint32_t g     = group_of(K);
      DlschGroup&    G     = p.groups[g];
      p.grp[2 * t + which] = (uint8_t)g;
      d.cb_base[which]     = G.n; // (within the group; the group's offset is added below)
      G.n += ncb;
      G.rvmask |= 1u << in.rv;
      G.fold2 = std::max(G.fold2, (std::min(emax, 3 * K + 12) + 1) / 2); // (an odd E: its last LLR is half a pair)
    };
    if (seg.C1) join(0, seg.K1, seg.C1);
    if (seg.C > seg.C1) join(1, seg.K2, seg.C - seg.C1);
  }
  p.total_cb = p.dec_bytes = 0;
  for (DlschGroup& G : p.groups) {
    G.off  = (uint32_t)p.total_cb;
    G.doff = p.dec_bytes;
    p.total_cb += G.n;
    p.dec_bytes += (size_t)G.n * (G.K / 8);
  }
  for (uint32_t t = 0; t < ntb; t++) {
    if (!p.tbd[t].C) continue;
    p.tbd[t].cb_base[0] += p.groups[p.grp[2 * t]].off;
    p.tbd[t].cb_base[1] += p.groups[p.grp[2 * t + 1]].off;
  }
}

} // namespace mi355
