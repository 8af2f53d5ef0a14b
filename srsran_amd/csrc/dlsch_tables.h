// srsran_amd/csrc/dlsch_tables.h -- host builders of the DL-SCH's device tables: the inverse rate-dematching tables
// with their parity-row minima, the compact decoder-order image, the CRC byte tables and the CRC scale factors.  Pure
// functions returning the bytes that dlsch_tables.cpp (and tdec8_runtime.cpp) upload; host-only, no HIP
// (tools/dlsch_plan_check checks them on the CPU).
#pragma once
#include <algorithm>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "dlsch_layout.h"
#include "rm_tables.h"

namespace mi355 {

// decoder buffer length of K in the layout of nsb sub-blocks (0: linear)
inline uint32_t rm_buflen_nsb(uint32_t K, uint32_t nsb) { return nsb ? 3 * (K + 32) + 12 : 3 * K + 12; }
inline uint32_t rm_buflen(uint32_t K) { return rm_buflen_nsb(K, tdec_subblocks(K)); }

// inverse of a rate-dematching table t (circular index r -> decoder position): len entries, decoder position ->
// circular index, `fill` where no circular-buffer bit lands
inline std::vector<uint16_t> rm_inverse(const std::vector<uint16_t>& t, size_t len, uint16_t fill)
{
  std::vector<uint16_t> inv(len, fill);
  for (size_t r = 0; r < t.size(); r++) inv[t[r]] = (uint16_t)r;
  return inv;
}
inline std::vector<uint16_t> rm_inverse(uint32_t K, uint32_t rv, uint32_t nsb, size_t len, uint16_t fill)
{
  return rm_inverse(rm_rx_table_nsb(K, rv, nsb), len, fill);
}

// the 16-bit decoder's table of (K, rv): buflen + 1 inverse entries, then (rm_rowmin_off) the parity-row minima of the
// 16-window layout, L = K / 16 rows per stream; rows >= L, the padding and every row of another layout stay 0 (defined)
inline std::vector<uint16_t> rm16_table(uint32_t K, uint32_t rv)
{
  const uint32_t        buflen = rm_buflen(K);
  std::vector<uint16_t> inv    = rm_inverse(K, rv, tdec_subblocks(K), buflen + 1, RM_NONE);
  inv.resize(rm_rowmin_off(buflen) + rm_rowmin_len(), 0);
  if (tdec_subblocks(K) == 16) {
    uint16_t*      rmin = inv.data() + rm_rowmin_off(buflen);
    const uint32_t L    = K / 16;
    for (uint32_t s = 0; s < 2; s++)
      for (uint32_t j = 0; j < L; j++) {
        uint16_t m = RM_NONE;
        for (uint32_t w = 0; w < 16; w++) m = std::min(m, inv[(s + 1) * (K + 32) + j * 16 + w]);
        rmin[s * 32 * SB_ROWMASK_WORDS + j] = m;
      }
  }
  return inv;
}

// the same for the 8-bit decoder buffer layout (srslte_rm_turbo_rx_lut_8bit: sub-blocks of the 8-bit decoder); no minima
inline std::vector<uint16_t> rm8_inv_table(uint32_t K, uint32_t rv)
{
  const uint32_t nsb = tdec_subblocks_8bit(K);
  return rm_inverse(K, rv, nsb, rm_buflen_nsb(K, nsb) + 1, RM_NONE);
}

// The compact decoder-order image of (K, rv, E), 0 < E <= 3 K + 12 (runtime_internal.h, dlsch_rm_compact): tab[r], r < E,
// is LLR r's image slot; at u16 offset qoff the nq quad entries (u32 each), then 8 u16 of padding.
struct RmCompact {
  std::vector<uint16_t> tab;
  uint32_t              nq = 0, qoff = 0;
};
inline RmCompact rm_compact_table(uint32_t K, uint32_t rv, uint32_t E)
{
  const std::vector<uint16_t> t      = rm_rx_table(K, rv); // circular index r -> decoder position
  const uint32_t              buflen = rm_buflen(K), nquad = (buflen + 7) / 8;
  const std::vector<uint16_t> inv    = rm_inverse(t, buflen, RM_NONE);
  // a parity row (16-window layout) is written iff one of its 16 positions receives an LLR r < E (rm_image.h)
  auto defined = [&](uint32_t pos) {
    if (tdec_subblocks(K) != 16) return true;
    const uint32_t sl = K + 32, s = pos / sl;
    if (s == 0 || s > 2) return true;
    const uint32_t j = (pos - s * sl) >> 4;
    if (j >= 32 * SB_ROWMASK_WORDS || j >= K / 16) return true;
    for (uint32_t w = 0; w < 16; w++)
      if (inv[s * sl + j * 16 + w] < E) return true;
    return false;
  };
  // quad entries: decoder quad index | (bit p: position 8 q + p receives an LLR r < E) << 16; the image slots of the
  // other positions are never written, and the rate dematcher masks them to zero
  std::vector<uint16_t> rank(nquad, 0xffff);
  std::vector<uint32_t> qlist;
  for (uint32_t qd = 0; qd < nquad; qd++) {
    if (!defined(8 * qd)) continue;
    uint32_t m = 0;
    for (uint32_t p = 0; p < 8 && 8 * qd + p < buflen; p++) m |= (uint32_t)(inv[8 * qd + p] < E) << p;
    rank[qd] = (uint16_t)qlist.size();
    qlist.push_back(qd | m << 16);
  }
  RmCompact c;
  c.nq   = (uint32_t)qlist.size();
  c.qoff = (E + 7) / 8 * 8; // u16 offset of the quad entries (16-byte aligned)
  c.tab.assign(c.qoff + 2 * qlist.size() + 8, 0);
  for (uint32_t r = 0; r < E; r++) {
    const uint32_t pos = t[r];
    if (rank[pos / 8] == 0xffff) return RmCompact{}; // (cannot happen: the quad holds LLR r < E) -- empty = error
    c.tab[r] = (uint16_t)(8 * rank[pos / 8] + pos % 8);
  }
  memcpy(c.tab.data() + c.qoff, qlist.data(), qlist.size() * 4);
  return c;
}

// a * b mod P over GF(2), degree < 24 (poly with the x^24 term)
inline uint32_t gf2_mulmod24(uint32_t a, uint32_t b, uint32_t poly)
{
  uint32_t r = 0;
  for (int i = 23; i >= 0; i--) {
    r <<= 1;
    if (r & 0x1000000u) r ^= poly;
    if ((b >> i) & 1u) r ^= a;
  }
  return r & 0xffffffu;
}

// x^(8 n) mod P by square and multiply
inline uint32_t gf2_xpow8(uint32_t n, uint32_t poly)
{
  uint32_t sc = 1, x8 = 1u << 8; // x^(8 * 2^i)
  for (; n; n >>= 1) {
    if (n & 1) sc = gf2_mulmod24(sc, x8, poly);
    x8 = gf2_mulmod24(x8, x8, poly);
  }
  return sc;
}

constexpr uint32_t CRC24A_POLY = 0x1864CFB, CRC24B_POLY = 0x1800063; // crc.h:40-41

// byte table + x^(8*2^i) mod P (start from x^8, square repeatedly)
inline CrcTable make_crc_table(uint32_t poly)
{
  CrcTable t{};
  t.poly = poly;
  for (uint32_t i = 0; i < 256; i++) {
    uint32_t c = i << 16;
    for (int j = 0; j < 8; j++) c = (c & 0x800000) ? ((c << 1) ^ poly) & 0xffffff : (c << 1) & 0xffffff;
    t.t[i] = c;
  }
  uint32_t p = 1u << 8;
  for (int i = 0; i < 24; i++) {
    t.pw[i] = p;
    p       = gf2_mulmod24(p, p, poly);
  }
  return t;
}

// per-lane CRC chunk scale factors for the decision bytes of K (wave_crc24_scaled), both polynomials.
// [0, 128): 64 lanes of a wave (dlsch_cb_check); [128, 144): the NL = nsb / 2 lanes of a code block in the window
// decoder's fused check (tdec_kernels.hip), 8 per polynomial
inline std::vector<uint32_t> crc_scales_table(uint32_t K)
{
  std::vector<uint32_t> t(144, 0u);
  const uint32_t        nbytes = K / 8, chunk = (nbytes + 63) / 64;
  const uint32_t        polys[2] = {CRC24A_POLY, CRC24B_POLY};
  const uint32_t        nl = std::max(1u, tdec_subblocks(K) / 2), cl = nbytes / nl;
  for (int pi = 0; pi < 2; pi++) {
    for (uint32_t lane = 0; lane < 64; lane++) {
      const uint32_t b0 = std::min(nbytes, lane * chunk), b1 = std::min(nbytes, b0 + chunk);
      t[pi * 64 + lane] = gf2_xpow8(nbytes - b1, polys[pi]);
    }
    for (uint32_t l = 0; l < nl && l < 8; l++) t[128 + 8 * pi + l] = gf2_xpow8(nbytes - (l + 1) * cl, polys[pi]);
  }
  return t;
}

// the TB epilogue's CRC24A of nbytes bytes by 256 threads (block_crc24_scaled4): thread t's factor
// x^(8 * bytes after its chunk) mod P, chunk = ceil(nbytes / 256) rounded up to a word
inline std::vector<uint32_t> tb_crc_scales_table(uint32_t nbytes)
{
  std::vector<uint32_t> t(256);
  const uint32_t        chunk = ((nbytes + 255) / 256 + 3) / 4 * 4;
  for (uint32_t tid = 0; tid < 256; tid++) {
    const uint32_t b0 = std::min(nbytes, tid * chunk), b1 = std::min(nbytes, b0 + chunk);
    t[tid] = gf2_xpow8(nbytes - b1, CRC24A_POLY);
  }
  return t;
}

} // namespace mi355
