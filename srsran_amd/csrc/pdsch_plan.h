// srsran_amd/csrc/pdsch_plan.h -- the host-only rules of a PDSCH decode call over plain data: which equaliser
// configurations are admitted, the power allocation, the scrambling seed, the layout of the front end's device scratch
// and which jobs pdsch_eq_rm can take.  No HIP (tools/pdsch_plan_check runs it on the CPU).
#pragma once
#include <algorithm>
#include <cmath>
#include <stddef.h>
#include <stdint.h>

#include "../../include/srsran_amd/pdsch.h"
#include "../../include/srsran_amd/tdec.h"
#include "rm_tables.h"

namespace mi355 {

inline uint32_t mod_bits(uint32_t mod)
{
  switch (mod) {
    case MI355_MOD_BPSK: return 1;
    case MI355_MOD_QPSK: return 2;
    case MI355_MOD_16QAM: return 4;
    case MI355_MOD_64QAM: return 6;
    case MI355_MOD_256QAM: return 8;
  }
  return 0;
}

// The range checks of srslte_pdsch_decode's inputs (MI355_ERROR_INVALID_INPUTS), then the equaliser configurations
// there are (precoding.c:1876-1938 with MMSE and csi; MI355_ERROR otherwise).  *cb: the codebook index.
inline int pdsch_admit(uint32_t cfi, uint32_t sch, uint32_t np, uint32_t nrx, uint32_t L, uint32_t nof_tb, uint32_t pmi,
                       uint32_t* cb)
{
  if (cfi < 1 || cfi > 3 || L == 0 || L > 4 || nof_tb == 0 || nof_tb > 2 || L < nof_tb)
    return MI355_ERROR_INVALID_INPUTS;
  *cb     = nof_tb == 1 ? pmi : pmi + 1;
  bool ok = false;
  switch (sch) {
    case MI355_TXSCHEME_PORT0: ok = np == 1 && L == 1; break;
    case MI355_TXSCHEME_DIVERSITY: ok = (np == 2 || np == 4) && L == np && nof_tb == 1; break;
    case MI355_TXSCHEME_SPATIALMUX:
      ok = np == 2 && nrx == 2 && L == nof_tb && ((L == 2 && *cb <= 2) || (L == 1 && *cb <= 3));
      break;
    case MI355_TXSCHEME_CDD: ok = np == 2 && nrx == 2 && L == 2 && nof_tb == 2; break;
  }
  return ok ? MI355_SUCCESS : MI355_ERROR;
}

// power allocation (pdsch.c:575-611, 926-932); ns0: OFDM symbols of the first slot.  rhob_mask: the symbols l' scaled
// by rhob_inv
struct PdschPower {
  float    scaling = 1.0f, rhob_inv = 1.0f;
  uint32_t rhob_mask = 0;
};
inline int pdsch_power(const mi355_pdsch_cfg_t& cfg, uint32_t np, uint32_t cp, uint32_t ns0, PdschPower* out)
{
  // 36.213 Table 5.2-1 rho_B / rho_A (pdsch.c:44-46)
  static const float kCellSpecificRatio[2][4] = {{1.0f / 1.0f, 4.0f / 5.0f, 3.0f / 5.0f, 2.0f / 5.0f},
                                                 {5.0f / 4.0f, 1.0f / 1.0f, 3.0f / 4.0f, 1.0f / 2.0f}};
  *out = PdschPower{};
  if (!cfg.power_scale) return MI355_SUCCESS;
  if (cfg.p_b > 3) return MI355_ERROR_INVALID_INPUTS;
  const float rho_a = (float)((double)powf(10.0f, cfg.p_a / 20.0f) * (np == 1 ? 1.0 : 1.4142135623730951));
  const float rho_b = sqrtf(kCellSpecificRatio[np == 1 ? 0 : 1][cfg.p_b]);
  if (rho_b != 0.0f && rho_b != 1.0f) {
    out->rhob_inv = 1.0f / rho_b;
    for (uint32_t s = 0; s < 2; s++) {
      out->rhob_mask |= 1u << (s * ns0 + 0);
      out->rhob_mask |= 1u << (s * ns0 + (cp == MI355_CP_NORM ? 4 : 3));
      if (np == 4) out->rhob_mask |= 1u << (s * ns0 + 1);
    }
  }
  if (rho_a != 0.0f && std::isnormal(rho_a)) out->scaling = rho_a;
  return MI355_SUCCESS;
}

// the scrambling sequence's seed (36.211 6.3.1; srslte_sequence_pdsch)
inline uint32_t pdsch_c_init(uint16_t rnti, uint32_t cw_idx, uint32_t tti, uint32_t cell_id)
{
  return ((uint32_t)rnti << 14) + (cw_idx << 13) + ((tti % 10) << 9) + cell_id;
}

// The front end's device scratch of one call, byte offsets from its base:
//   [staged descriptors: jobs | cws | nci | ndst | rj] [d | csi | e | cmax | cfin | wtab]
// The staged part mirrors the pinned host buffer (256-byte slots, uploaded with one copy): job and codeword
// descriptors, the c_init and destination of each descrambling sequence to generate, and pdsch_eq_rm's jobs.  Then the
// arenas: equalised symbols (nd float2), their csi (nd float), the LLRs (ne int16), the per-block csi maxima
// (2 x nparts per job; written by every equaliser block that has work, read by the LLR kernel: no initialisation),
// their per-codeword maximum, and nwt bytes of two-layer MMSE matrices (PdschJobDev.wtab).  Every region starts on a
// 256-byte boundary.
struct FrontLayout {
  size_t jobs, cws, nci, ndst, rj, staged; // staged: the bytes of the staged part = the first arena's offset
  size_t d, csi, e, cmax, cfin, wtab, total;
};
inline FrontLayout front_layout(size_t njobs, size_t ncw, size_t n_new_scr, size_t nd, size_t ne, size_t nparts, size_t nwt,
                                bool with_eqrm, size_t job_bytes, size_t cw_bytes, size_t rj_bytes)
{
  auto        rnd = [](size_t b) { return (b + 255) / 256 * 256; };
  FrontLayout l{};
  l.cws    = l.jobs + rnd(njobs * job_bytes);
  l.nci    = l.cws + rnd(ncw * cw_bytes);
  l.ndst   = l.nci + rnd(n_new_scr * 4);
  l.rj     = l.ndst + rnd(n_new_scr * 8);
  l.staged = l.rj + (with_eqrm ? rnd(njobs * rj_bytes) : 0);
  l.d      = l.staged;
  l.csi    = l.d + rnd(nd * 8);
  l.e      = l.csi + rnd(nd * 4);
  l.cmax   = l.e + rnd(ne * 2);
  l.cfin   = l.cmax + rnd(njobs * 2 * nparts * 4);
  l.wtab   = l.cfin + rnd(ncw * 4);
  l.total  = l.wtab + nwt;
  return l;
}

// One transport block as pdsch_eq_rm's planning reads it, and the segmentation of the previous one (a batch has few
// distinct TB sizes)
struct EqRmTb {
  int32_t  tbs;
  uint32_t nof_bits, qm, rv, softbuffer;
};
struct SegCache {
  uint32_t tbs = UINT32_MAX;
  CbSegm   seg{};
  int      err = 0;
};
// what a qualifying job's workgroups share: nt transport blocks to decode (0: the rest is zero) of C code blocks,
// C1 of size K1 then K2 (used[kx]: the size occurs), Qm bits per symbol, Gp symbols; a code block has E[0] LLRs, the
// last Gp % C ones E[1] (nE = 1 where all have E[0]); n_max: the largest E
struct EqRmShape {
  uint32_t nt, C, C1, K1, K2, Qm, Gp, n_max, E[2], nE;
  bool     used[2];
};
// pdsch_eq_rm takes a job whose transport blocks to decode (decode[t]) have one modulation, TBS and E (so code block c
// of either codeword comes from the same REs), no filler bits, at most max_cb code blocks, E <= N for every code block
// (no wrap-around), rv <= 3 and a softbuffer of the pool
inline bool eqrm_job_shape(const EqRmTb tb[2], const bool decode[2], uint32_t max_cb, uint32_t nof_sb, SegCache& sc,
                           EqRmShape* out)
{
  EqRmShape s{};
  uint32_t  tbs = 0, nbits = 0;
  for (uint32_t t = 0; t < 2; t++) {
    if (!decode[t]) continue;
    if (s.nt && (tb[t].qm != s.Qm || (uint32_t)tb[t].tbs != tbs || tb[t].nof_bits != nbits)) return false;
    if (tb[t].tbs <= 0) return false;
    if ((uint32_t)tb[t].tbs != sc.tbs) sc.tbs = (uint32_t)tb[t].tbs, sc.err = cbsegm(sc.tbs, &sc.seg);
    const CbSegm& seg = sc.seg;
    if (sc.err || seg.F || seg.C == 0 || seg.C > max_cb || tb[t].softbuffer >= nof_sb || tb[t].rv > 3 || tb[t].qm == 0)
      return false;
    tbs = (uint32_t)tb[t].tbs, nbits = tb[t].nof_bits, s.nt++;
    s.C = seg.C, s.C1 = seg.C1, s.K1 = seg.K1, s.K2 = seg.K2, s.Qm = tb[t].qm, s.Gp = nbits / s.Qm;
    s.E[0] = s.Qm * (s.Gp / s.C), s.E[1] = s.E[0] + s.Qm, s.nE = s.Gp % s.C ? 2 : 1;
    s.n_max             = s.E[1];
    s.used[0]           = s.K1 && s.C1;
    s.used[1]           = s.K2 && s.C1 != s.C;
    const uint32_t kmin = s.C1 ? (s.C1 < s.C ? std::min(s.K1, s.K2) : s.K1) : s.K2;
    if (s.n_max > 3 * kmin + 12) return false;
  }
  *out = s;
  return true;
}

} // namespace mi355
