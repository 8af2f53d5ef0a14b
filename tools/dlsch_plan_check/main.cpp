// tools/dlsch_plan_check/main.cpp -- host check of the DL-SCH's table builders (srsran_amd/csrc/dlsch_tables.h) and call
// planning (dlsch_plan.h), for a sanitizer build (no GPU, no HIP, nothing preloaded):
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Isrsran_amd/csrc
//       tools/dlsch_plan_check/main.cpp -o /tmp/dlsch_plan_check && /tmp/dlsch_plan_check
// Checks, for all 188 code-block sizes x rv 0-3 x both sub-block rules: the inverse rate-dematching tables are
// permutations of the circular buffer with RM_NONE elsewhere, the parity-row minima are the brute-force ones, the
// compact image maps every LLR to its quad's slot; the CRC tables against a bit-serial CRC, the scale factors against
// x^0 = 1, the power law and the chunked CRC they exist for; the plan of a mixed batch (both LLR widths).
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "dlsch_plan.h"
#include "dlsch_tables.h"
#include "rm_tables.h"

using namespace mi355;

static int g_failed = 0;
#define EXPECT(c)                                                                                                      \
  do {                                                                                                                 \
    if (!(c)) {                                                                                                        \
      if (g_failed++ < 20) fprintf(stderr, "%s:%d: EXPECT(%s) failed [%s]\n", __FILE__, __LINE__, #c, g_ctx);          \
    }                                                                                                                  \
  } while (0)
static char g_ctx[96] = "";
#define CTX(...) snprintf(g_ctx, sizeof(g_ctx), __VA_ARGS__)

// ---------------------------------------------------------------- inverse tables and row minima

// inv[0, len): every circular index 0 .. N-1 exactly once, all below buflen, RM_NONE elsewhere
static void check_inverse(const uint16_t* inv, size_t len, uint32_t buflen, uint32_t N)
{
  std::vector<uint8_t> seen(N, 0);
  uint32_t             found = 0;
  for (size_t pos = 0; pos < len; pos++) {
    if (inv[pos] == RM_NONE) continue;
    EXPECT(pos < buflen && inv[pos] < N && !seen[inv[pos]]);
    if (inv[pos] < N) seen[inv[pos]] = 1, found++;
  }
  EXPECT(found == N);
}

static void inverse_tables()
{
  for (int i = 0; i < LTE_NOF_CB_SIZES; i++) {
    const uint32_t K = lte_qpp_table[i][0], N = 3 * K + 12;
    for (uint32_t rv = 0; rv < 4; rv++) {
      CTX("K=%u rv=%u", K, rv);
      // the 16-bit decoder's rule: buflen + 1 entries, then the row minima
      const uint32_t              nsb = tdec_subblocks(K), buflen = nsb ? 3 * (K + 32) + 12 : N;
      const std::vector<uint16_t> t16 = rm16_table(K, rv);
      EXPECT(rm_buflen(K) == buflen && t16.size() == rm_rowmin_off(buflen) + rm_rowmin_len());
      check_inverse(t16.data(), buflen + 1, buflen, N);
      EXPECT(t16[buflen] == RM_NONE);
      for (size_t p = buflen + 1; p < rm_rowmin_off(buflen); p++) EXPECT(t16[p] == 0);
      const uint16_t* rmin = t16.data() + rm_rowmin_off(buflen);
      for (uint32_t s = 0; s < 2; s++)
        for (uint32_t j = 0; j < 32 * SB_ROWMASK_WORDS; j++) {
          uint16_t m = 0; // rows >= K / 16 and every row of another layout
          if (nsb == 16 && j < K / 16) {
            m = RM_NONE;
            for (uint32_t w = 0; w < 16; w++) m = std::min(m, t16[(s + 1) * (K + 32) + 16 * j + w]);
          }
          EXPECT(rmin[s * 32 * SB_ROWMASK_WORDS + j] == m);
        }
      // the 8-bit decoder's rule: buflen + 1 entries in the DL-SCH, buflen in the stand-alone rate dematcher
      const uint32_t              nsb8 = tdec_subblocks_8bit(K), buflen8 = nsb8 ? 3 * (K + 32) + 12 : N;
      const std::vector<uint16_t> t8 = rm8_inv_table(K, rv), t8s = rm_inverse(K, rv, nsb8, buflen8, RM_NONE);
      EXPECT(rm_buflen_nsb(K, nsb8) == buflen8 && t8.size() == buflen8 + 1 && t8s.size() == buflen8);
      check_inverse(t8.data(), t8.size(), buflen8, N);
      EXPECT(t8[buflen8] == RM_NONE && !memcmp(t8.data(), t8s.data(), 2 * buflen8));
      if (nsb8 == nsb) EXPECT(!memcmp(t8.data(), t16.data(), 2 * (buflen + 1)));
    }
  }
}

// ---------------------------------------------------------------- compact image

static void compact_tables()
{
  for (int i = 0; i < LTE_NOF_CB_SIZES; i++) {
    const uint32_t K = lte_qpp_table[i][0], N = 3 * K + 12, buflen = rm_buflen(K);
    const uint32_t Es[6] = {1, 2, N / 3, N / 2, N - 1, N};
    for (uint32_t rv = 0; rv < 4; rv++) {
      const std::vector<uint16_t> t = rm_rx_table(K, rv);
      for (uint32_t E : Es) {
        CTX("K=%u rv=%u E=%u", K, rv, E);
        const RmCompact c = rm_compact_table(K, rv, E);
        EXPECT(c.qoff == (E + 7) / 8 * 8 && c.tab.size() == c.qoff + 2 * (size_t)c.nq + 8);
        if (c.tab.size() != c.qoff + 2 * (size_t)c.nq + 8) continue;
        std::vector<uint32_t> quad(c.nq);
        memcpy(quad.data(), c.tab.data() + c.qoff, 4 * (size_t)c.nq);
        uint32_t bits = 0;
        for (uint32_t k = 0; k < c.nq; k++) {
          EXPECT((quad[k] & 0xffff) < (buflen + 7) / 8 && (quad[k] >> 24) == 0);
          if (k) EXPECT((quad[k] & 0xffff) > (quad[k - 1] & 0xffff)); // decoder order
          bits += (uint32_t)__builtin_popcount(quad[k] >> 16);
        }
        EXPECT(bits == E); // a mask bit per LLR and no other
        for (uint32_t r = 0; r < E; r++) {
          const uint32_t rank = c.tab[r] / 8u, place = c.tab[r] % 8u;
          EXPECT(rank < c.nq);
          if (rank >= c.nq) break;
          EXPECT(8 * (quad[rank] & 0xffff) + place == t[r] && ((quad[rank] >> (16 + place)) & 1u));
        }
        for (size_t p = E; p < c.qoff; p++) EXPECT(c.tab[p] == 0);
        for (size_t p = c.tab.size() - 8; p < c.tab.size(); p++) EXPECT(c.tab[p] == 0);
      }
    }
  }
}

// ---------------------------------------------------------------- CRC tables and scale factors

static uint32_t crc24_serial(const uint8_t* d, size_t n, uint32_t poly)
{
  uint32_t reg = 0;
  for (size_t i = 0; i < 8 * n; i++) {
    const uint32_t bit = (d[i / 8] >> (7 - i % 8)) & 1u;
    const uint32_t top = ((reg >> 23) & 1u) ^ bit;
    reg                = (reg << 1) & 0xffffffu;
    if (top) reg ^= poly & 0xffffffu;
  }
  return reg;
}

static uint32_t crc24_table(const CrcTable& t, const uint8_t* d, size_t n)
{
  uint32_t c = 0;
  for (size_t i = 0; i < n; i++) c = ((c << 8) & 0xffffffu) ^ t.t[((c >> 16) & 0xffu) ^ d[i]];
  return c;
}

// the CRC of d from per-chunk CRCs and their scale factors, as the kernels combine them: chunk l = bytes [l c, (l+1) c)
static uint32_t crc24_chunked(const CrcTable& t, const uint8_t* d, uint32_t n, uint32_t chunk, const uint32_t* scale,
                              uint32_t lanes)
{
  uint32_t c = 0;
  for (uint32_t l = 0; l < lanes; l++) {
    const uint32_t b0 = std::min(n, l * chunk), b1 = std::min(n, b0 + chunk);
    c ^= gf2_mulmod24(crc24_table(t, d + b0, b1 - b0), scale[l], t.poly);
  }
  return c;
}

static void crc_tables()
{
  const uint32_t polys[2] = {CRC24A_POLY, CRC24B_POLY};
  EXPECT(CRC24A_POLY == 0x1864CFB && CRC24B_POLY == 0x1800063);
  std::vector<uint8_t> msg(12000);
  uint32_t             lcg = 12345;
  for (uint8_t& b : msg) b = (uint8_t)((lcg = lcg * 1664525u + 1013904223u) >> 24);
  for (int pi = 0; pi < 2; pi++) {
    const CrcTable t = make_crc_table(polys[pi]);
    EXPECT(t.poly == polys[pi]);
    for (size_t n : {0, 1, 2, 3, 5, 64, 767, 768, 12000}) {
      CTX("poly %d n=%zu", pi, n);
      EXPECT(crc24_table(t, msg.data(), n) == crc24_serial(msg.data(), n, polys[pi]));
    }
    const uint8_t one[3] = {0, 0, 1}; // x^0 through the register: x^24 mod P
    EXPECT(crc24_table(t, one, 3) == (polys[pi] & 0xffffffu));
    for (uint32_t i = 0; i < 24; i++) EXPECT(t.pw[i] == gf2_xpow8(1u << i, polys[pi]));
    EXPECT(gf2_xpow8(0, polys[pi]) == 1 && gf2_xpow8(1, polys[pi]) == 0x100 && gf2_xpow8(2, polys[pi]) == 0x10000);
    for (uint32_t a : {0u, 1u, 7u, 95u, 768u, 37000u})
      for (uint32_t b : {0u, 3u, 64u, 767u, 9421u})
        EXPECT(gf2_xpow8(a + b, polys[pi]) == gf2_mulmod24(gf2_xpow8(a, polys[pi]), gf2_xpow8(b, polys[pi]), polys[pi]));
  }
  const CrcTable ta = make_crc_table(CRC24A_POLY), tb = make_crc_table(CRC24B_POLY);
  // a one-chunk message: lane 0 holds all of it, nothing follows, factor x^0 = 1
  const std::vector<uint32_t> s1 = crc_scales_table(8);
  EXPECT(s1.size() == 144 && s1[0] == 1 && s1[64] == 1 && s1[128] == 1 && s1[136] == 1);
  EXPECT(tb_crc_scales_table(1)[0] == 1 && tb_crc_scales_table(4)[0] == 1);
  for (int i = 0; i < LTE_NOF_CB_SIZES; i++) {
    const uint32_t K = lte_qpp_table[i][0], nb = K / 8, nl = std::max(1u, tdec_subblocks(K) / 2);
    CTX("crc scales K=%u", K);
    const std::vector<uint32_t> s = crc_scales_table(K);
    EXPECT(s.size() == 144);
    EXPECT(crc24_chunked(ta, msg.data(), nb, (nb + 63) / 64, &s[0], 64) == crc24_serial(msg.data(), nb, CRC24A_POLY));
    EXPECT(crc24_chunked(tb, msg.data(), nb, (nb + 63) / 64, &s[64], 64) == crc24_serial(msg.data(), nb, CRC24B_POLY));
    if (nb % nl == 0) { // the window decoder's lanes: nl equal chunks
      EXPECT(crc24_chunked(ta, msg.data(), nb, nb / nl, &s[128], nl) == crc24_serial(msg.data(), nb, CRC24A_POLY));
      EXPECT(crc24_chunked(tb, msg.data(), nb, nb / nl, &s[136], nl) == crc24_serial(msg.data(), nb, CRC24B_POLY));
    }
    for (uint32_t l = nl; l < 8; l++) EXPECT(s[128 + l] == 0 && s[136 + l] == 0);
  }
  for (uint32_t nb : {1u, 2u, 5u, 125u, 256u, 257u, 1023u, 1024u, 1025u, 9422u, 12000u}) {
    CTX("tb crc scales nbytes=%u", nb);
    const std::vector<uint32_t> s = tb_crc_scales_table(nb);
    const uint32_t chunk = ((nb + 255) / 256 + 3) / 4 * 4;
    EXPECT(s.size() == 256);
    EXPECT(crc24_chunked(ta, msg.data(), nb, chunk, s.data(), 256) == crc24_serial(msg.data(), nb, CRC24A_POLY));
  }
}

// ---------------------------------------------------------------- the plan

struct Tb {
  uint32_t tbs, Qm, G, rv, sb;
  int      bad; // 0 decoded, 1 invalid, 2 nothing to decode (success)
};

// tests/test_dlsch_gpu.py CASES, then: a TB of two code-block sizes (6136: K1 = 3136 then K2 = 3072), tbs 6200 (two
// code blocks of K = 3136), and the five entries the planner does not decode
static const uint32_t NOF_SB = 24, MAX_CB = 16;
static const Tb       BATCH[] = {
    {15840, 2, 30000, 0, 0, 0}, {97896, 8, 115200, 1, 1, 0}, {97896, 8, 115200, 0, 2, 0}, {30576, 6, 36300, 2, 3, 0},
    {1000, 2, 3010, 0, 4, 0},   {456, 2, 1500, 3, 5, 0},     {0, 2, 100, 0, 6, 2},        {40, 2, 200, 0, 7, 0},
    {6120, 4, 14402, 0, 8, 0},  {1000, 2, 3010, 0, 24, 1},   {75376, 6, 86400, 3, 9, 0},  {2600, 2, 7800, 0, 10, 0},
    {1000, 2, 3010, 4, 11, 1},  {144, 2, 1080, 0, 12, 0},    {6136, 2, 14000, 1, 13, 0},  {256, 2, 1080, 0, 14, 0},
    {1000, 0, 3010, 0, 15, 1},  {40, 2, 600, 2, 16, 0},      {149776, 6, 180000, 0, 17, 1}, {6200, 2, 13000, 0, 18, 0},
    {6136, 2, 25000, 0, 19, 0}};

static void check_plan(DlschPlan& p, bool llr8)
{
  const uint32_t                ntb = sizeof(BATCH) / sizeof(BATCH[0]);
  std::vector<mi355_dlsch_tb_t> in(ntb);
  for (uint32_t t = 0; t < ntb; t++) {
    in[t] = mi355_dlsch_tb_t{BATCH[t].tbs, BATCH[t].G, BATCH[t].Qm, BATCH[t].rv, BATCH[t].sb, 1000u * t, 77u * t};
  }
  plan_tbs(p, in.data(), ntb, NOF_SB, MAX_CB, llr8);
  EXPECT(p.tbd.size() == ntb);
  // expected: the groups in first-seen order (K1 before K2), their members' ranges in TB order
  struct Want {
    uint32_t K, n, rvmask, fold2;
  };
  std::vector<Want> want;
  uint32_t          nbad = 0;
  for (uint32_t t = 0; t < ntb; t++) {
    CTX("plan llr8=%d tb %u", (int)llr8, t);
    const TbDesc& d = p.tbd[t];
    CbSegm        sg{};
    EXPECT(cbsegm(BATCH[t].tbs, &sg) == 0);
    int bad = BATCH[t].bad;
    if (llr8 && !bad && ((sg.K1 > 400 && sg.K1 <= 800) || (sg.C2 && sg.K2 > 400 && sg.K2 <= 800))) bad = 1;
    nbad += BATCH[t].bad != 0;
    EXPECT(d.tbs == BATCH[t].tbs && d.data_off == 77u * t && d.invalid == (bad == 1 ? 1u : 0u));
    if (bad) {
      EXPECT(d.C == 0 && d.crc_scale == nullptr);
      continue;
    }
    EXPECT(d.C == sg.C && d.C1 == sg.C1 && d.K1 == sg.K1 && d.K2 == sg.K2 && sg.F == 0 && sg.C <= MAX_CB);
    EXPECT(d.slot0 == BATCH[t].sb * MAX_CB && d.Qm == BATCH[t].Qm && d.nof_e_bits == BATCH[t].G && d.rv == BATCH[t].rv);
    EXPECT(d.e_off == 1000u * t && d.crc_scale == nullptr);
    // the largest E of its code blocks (sch.c:391-401), from the per-block formula
    const uint32_t Gp = BATCH[t].G / BATCH[t].Qm, gamma = Gp % sg.C;
    uint32_t       emax = 0;
    for (uint32_t cb = 0; cb < sg.C; cb++)
      emax = std::max(emax, BATCH[t].Qm * (cb + gamma < sg.C ? Gp / sg.C : (Gp + sg.C - 1) / sg.C));
    const uint32_t part[2][2] = {{sg.K1, sg.C1}, {sg.K2, sg.C - sg.C1}};
    for (int w = 0; w < 2; w++) {
      if (!part[w][1]) continue;
      size_t g = 0;
      while (g < want.size() && want[g].K != part[w][0]) g++;
      if (g == want.size()) want.push_back(Want{part[w][0], 0, 0, 0});
      // its range follows the group's earlier members'
      EXPECT(g < p.groups.size() && d.cb_base[w] == p.groups[g].off + want[g].n);
      want[g].n += part[w][1];
      want[g].rvmask |= 1u << BATCH[t].rv;
      want[g].fold2 = std::max(want[g].fold2, (std::min(emax, 3 * part[w][0] + 12) + 1) / 2);
    }
  }
  EXPECT(nbad == 5);
  CTX("plan llr8=%d groups", (int)llr8);
  EXPECT(p.groups.size() == want.size());
  size_t off = 0, doff = 0;
  for (size_t g = 0; g < want.size() && g < p.groups.size(); g++) { // the ranges partition [0, total_cb) group by group
    const DlschGroup& G = p.groups[g];
    EXPECT(G.K == want[g].K && G.n == want[g].n && G.rvmask == want[g].rvmask);
    EXPECT(G.off == off && G.doff == doff);
    EXPECT(G.fold2 >= want[g].fold2 && G.fold2 <= (3 * G.K + 12 + 1) / 2);
    off += G.n;
    doff += (size_t)G.n * (G.K / 8);
  }
  EXPECT(p.total_cb == off && p.dec_bytes == doff);
  // the two-size TB: K1 first, and 3136 first seen there; 456 (K = 480) only with 16-bit LLRs
  bool has480 = false, order = false;
  for (size_t g = 0; g + 1 < p.groups.size(); g++) order |= p.groups[g].K == 3136 && p.groups[g + 1].K == 3072;
  for (const DlschGroup& G : p.groups) has480 |= G.K == 480;
  EXPECT(order && has480 == !llr8);
}

static void plans()
{
  DlschPlan p, again;
  check_plan(p, false);
  const size_t ncb16 = p.total_cb;
  check_plan(p, true); // the same object: nothing of the last call's is left
  EXPECT(p.total_cb + 1 == ncb16);
  check_plan(p, false);
  check_plan(again, false);
  EXPECT(p.groups.size() == again.groups.size() && p.total_cb == again.total_cb && p.dec_bytes == again.dec_bytes);
  EXPECT(!memcmp(p.tbd.data(), again.tbd.data(), p.tbd.size() * sizeof(TbDesc)));
  plan_tbs(p, nullptr, 0, NOF_SB, MAX_CB, false);
  EXPECT(p.tbd.empty() && p.groups.empty() && p.total_cb == 0 && p.dec_bytes == 0);
}

int main()
{
  inverse_tables();
  compact_tables();
  crc_tables();
  plans();
  if (g_failed) {
    fprintf(stderr, "dlsch_plan_check: %d checks failed\n", g_failed);
    return 1;
  }
  printf("dlsch_plan_check: OK\n");
  return 0;
}
