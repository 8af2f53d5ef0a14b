// srsran_amd/csrc/pdsch_re_map.h -- the RE extraction order of a PDSCH grant (srslte_pdsch_get, pdsch.c:83-228) and the
// map image the receiver keeps in HBM per (allocation, cfi, subframe).  Host-only, no HIP (tools/pdsch_plan_check runs
// it on the CPU); mi355_pdsch_re_map and the map cache (pdsch_maps.cpp) both go through here.
#pragma once
#include <algorithm>
#include <stdint.h>
#include <vector>

#include "../../include/srsran_amd/pdsch.h"

namespace mi355 {

inline uint32_t nsymb_of(const mi355_cell_t& c) { return c.cp == MI355_CP_EXT ? 6 : 7; }

// pdsch_cp_skip_symbol (pdsch.c:83-114)
inline bool skip_symbol(const mi355_cell_t& c, const uint32_t ns[2], uint32_t sf, uint32_t s, uint32_t l, uint32_t n)
{
  if (!(n >= c.nof_prb / 2 - 3 && n < c.nof_prb / 2 + 3 + (c.nof_prb % 2))) return false;
  if (c.frame_type == MI355_FDD) {
    if (s == 0 && (sf == 0 || sf == 5) && l >= ns[s] - 2) return true;
  } else {
    if (s == 1 && (sf == 0 || sf == 5) && l >= ns[s] - 1) return true;
    if (s == 0 && (sf == 1 || sf == 6) && l == 2) return true;
  }
  return s == 1 && sf == 0 && l < 4;
}

// The extraction order of srslte_pdsch_cp(get) (pdsch.c:136-228): per slot, per OFDM symbol from the first
// non-control one, per allocated PRB; CRS REs skipped as prb_cp_ref does (prb_dl.c:46-74: `offset` REs, then
// nof_intervals-1 times {skip 1, copy 12/nof_refs-1}, then {skip 1, copy interval-offset} if positive);
// PSS/SSS/PBCH PRBs dropped except their outer halves for odd bandwidths.
template <class Emit> uint32_t walk_map(const mi355_cell_t& c, const mi355_pdsch_grant_t& g, uint32_t cfi, uint32_t sf,
                                        Emit emit)
{
  const uint32_t ns[2]    = {g.nof_symb_slot[0] ? g.nof_symb_slot[0] : nsymb_of(c),
                             g.nof_symb_slot[1] ? g.nof_symb_slot[1] : nsymb_of(c)};
  const uint32_t nof_refs = c.nof_ports == 1 ? 2 : 4;
  const uint32_t lstart0  = cfi + (c.nof_prb < 10 ? 1 : 0); // SRSLTE_NOF_CTRL_SYMBOLS
  const int      ri       = 12 / (int)nof_refs - 1;
  uint32_t       k        = 0;
  auto           cp_ref   = [&](uint32_t p, int off, int intervals) {
    for (int i = 0; i < off; i++) emit(k++, p++);
    for (int j = 0; j < intervals - 1; j++) {
      p++;
      for (int i = 0; i < ri; i++) emit(k++, p++);
    }
    if (ri - off > 0) {
      p++;
      for (int i = 0; i < ri - off; i++) emit(k++, p++);
    }
  };
  for (uint32_t s = 0; s < 2; s++) {
    for (uint32_t l = s == 0 ? lstart0 : 0; l < ns[s]; l++) {
      const uint32_t nsymb_cp = nsymb_of(c);
      const bool     has_crs  = (l == 1 && c.nof_ports == 4) || l == 0 || l == nsymb_cp - 3; // SRSLTE_SYMBOL_HAS_REF
      const int      off      = !has_crs ? 0
                                : c.nof_ports == 1 ? (int)(l == 0 ? c.id % 6 : (c.id + 3) % 6)
                                                   : (int)(c.id % 3); // pdsch_cp_crs_offset
      const uint32_t lp = l + s * ns[0];
      for (uint32_t n = 0; n < c.nof_prb; n++) {
        if (!g.prb_idx[s][n]) continue;
        uint32_t p = (lp * c.nof_prb + n) * 12;
        if (!skip_symbol(c, ns, sf, s, l, n)) {
          if (has_crs) {
            cp_ref(p, off, (int)nof_refs);
          } else {
            for (uint32_t i = 0; i < 12; i++) emit(k++, p + i);
          }
        } else if (c.nof_prb % 2) {
          if (n == c.nof_prb / 2 - 3 || n == c.nof_prb / 2 + 3) {
            if (n == c.nof_prb / 2 + 3) p += 6;
            if (has_crs) {
              cp_ref(p, off, (int)nof_refs / 2);
            } else {
              for (uint32_t i = 0; i < 6; i++) emit(k++, p + i);
            }
          }
        }
      }
    }
  }
  return k;
}

// RE extraction map of one (allocation, cfi, subframe) as uploaded: all = [RE index -> grid index (n) | pad to an even
// count | grid index g0 + t -> RE index or 0xffff (g1 - g0) | distinct subcarriers of the REs, ascending (ncols)],
// the inverse letting the single-RE equalisers walk the grid.  Unused slots hold 0xffff.
struct ReMapImage {
  std::vector<uint16_t> all;
  uint32_t              n = 0, g0 = 0, g1 = 0, ncols = 0;
};

inline ReMapImage build_re_map(const mi355_cell_t& c, const mi355_pdsch_grant_t& g, uint32_t cfi, uint32_t sf)
{
  ReMapImage            m;
  std::vector<uint16_t> idx;
  idx.reserve(14 * 12 * c.nof_prb);
  walk_map(c, g, cfi, sf, [&](uint32_t, uint32_t p) { idx.push_back((uint16_t)p); });
  m.n = (uint32_t)idx.size();
  if (m.n) {
    m.g0 = *std::min_element(idx.begin(), idx.end());
    m.g1 = *std::max_element(idx.begin(), idx.end()) + 1u;
  }
  const uint32_t        row = 12 * c.nof_prb;
  std::vector<uint8_t>  used(row, 0);
  for (uint16_t gi : idx) used[gi % row] = 1;
  std::vector<uint16_t> cols;
  for (uint32_t k = 0; k < row; k++)
    if (used[k]) cols.push_back((uint16_t)k);
  m.ncols            = (uint32_t)cols.size();
  const uint32_t inv = (m.n + 1) & ~1u;
  m.all.assign(inv + (m.g1 - m.g0) + m.ncols, 0xffff);
  std::copy(idx.begin(), idx.end(), m.all.begin());
  for (uint32_t i = 0; i < m.n; i++) m.all[inv + idx[i] - m.g0] = (uint16_t)i;
  std::copy(cols.begin(), cols.end(), m.all.begin() + inv + (m.g1 - m.g0));
  return m;
}

} // namespace mi355
