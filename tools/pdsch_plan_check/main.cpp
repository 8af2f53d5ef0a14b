// tools/pdsch_plan_check/main.cpp -- host check of the PDSCH receiver's host-only rules (srsran_amd/csrc/pdsch_re_map.h,
// pdsch_plan.h), for a sanitizer build (no GPU, no HIP, nothing preloaded):
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Isrsran_amd/csrc
//       tools/pdsch_plan_check/main.cpp -o /tmp/pdsch_plan_check && /tmp/pdsch_plan_check
// Checks: the RE extraction order and the map image over bandwidths x ports x cell ids x cfi x subframes x duplex x CP x
// allocations (distinct indices inside the allocated PRBs and outside the control region, the inverse, the pad, the
// column list, the image length; an empty allocation); the front end's scratch layout over its counts (order,
// alignment, disjoint regions, the total against the sum written out here); the admission table and range checks with
// their return codes, the power allocation and the scrambling seed; pdsch_eq_rm's job-shape rule against cbsegm.
// (That the extraction order is the reference's is pinned by tests/test_ref_pins.py through mi355_pdsch_re_map.)
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <vector>

#include "pdsch_plan.h"
#include "pdsch_re_map.h"

using namespace mi355;

static int  g_failed   = 0;
static char g_ctx[128] = "";
#define EXPECT(c)                                                                                                      \
  do {                                                                                                                 \
    if (!(c)) {                                                                                                        \
      if (g_failed++ < 20) fprintf(stderr, "%s:%d: EXPECT(%s) failed [%s]\n", __FILE__, __LINE__, #c, g_ctx);          \
    }                                                                                                                  \
  } while (0)
#define CTX(...) snprintf(g_ctx, sizeof(g_ctx), __VA_ARGS__)

// ---------------------------------------------------------------- RE map and image

static void check_map(const mi355_cell_t& c, const mi355_pdsch_grant_t& g, uint32_t cfi, uint32_t sf)
{
  const uint32_t ns = c.cp == MI355_CP_EXT ? 6 : 7, row = 12 * c.nof_prb, G = 2 * ns * row;
  EXPECT(G <= 65536); // every grid index fits uint16_t
  // (plain arrays and one EXPECT per property: the sweep is a hundred million REs in an unoptimised build)
  static uint32_t idx[65536];
  static uint8_t  seen[65536], col[12 * MI355_MAX_PRB];
  memset(seen, 0, sizeof(seen)), memset(col, 0, sizeof(col));
  uint32_t       next = 0;
  bool           in_order = true;
  const uint32_t n = walk_map(c, g, cfi, sf, [&](uint32_t k, uint32_t p) {
    in_order &= k == next;
    if (next < G) idx[next] = p;
    next++;
  });
  EXPECT(in_order && n == next && n <= G);
  if (n > G) return;
  const uint32_t ctrl = cfi + (c.nof_prb < 10 ? 1 : 0);
  uint32_t       lo = UINT32_MAX, hi = 0;
  bool           ok = true; // distinct, in an allocated PRB of its slot, outside the control symbols
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t p = idx[i], lp = p / row, prb = p % row / 12, s = lp / ns, l = lp % ns;
    if (p >= G || seen[p] || !g.prb_idx[s][prb] || (s == 0 && l < ctrl)) {
      ok = false;
      break;
    }
    seen[p] = col[p % row] = 1;
    lo = p < lo ? p : lo, hi = p > hi ? p : hi;
  }
  EXPECT(ok);
  if (!ok) return;
  const ReMapImage m = build_re_map(c, g, cfi, sf);
  const uint32_t   inv = (n + 1) & ~1u;
  EXPECT(m.n == n && (n == 0 ? m.g0 == 0 && m.g1 == 0 : m.g0 == lo && m.g1 == hi + 1));
  EXPECT(m.all.size() == (size_t)inv + (m.g1 - m.g0) + m.ncols);
  if (m.n != n || m.all.size() != (size_t)inv + (m.g1 - m.g0) + m.ncols) return;
  const uint16_t* all = m.all.data();
  for (uint32_t i = 0; i < n; i++) ok &= all[i] == idx[i] && all[inv + idx[i] - m.g0] == i;
  EXPECT(ok);
  if (n & 1) EXPECT(all[n] == 0xffff);
  uint32_t holes = 0;
  for (uint32_t t = 0; t < m.g1 - m.g0; t++) holes += all[inv + t] == 0xffff;
  EXPECT(holes == m.g1 - m.g0 - n); // every inverse entry that is no RE's
  const uint16_t* cols = all + inv + (m.g1 - m.g0);
  uint32_t        ncol = 0;
  for (uint32_t k = 0; k < row; k++) ncol += col[k];
  EXPECT(m.ncols == ncol);
  for (uint32_t k = 0; k < m.ncols; k++) ok &= cols[k] < row && col[cols[k]] && (k == 0 || cols[k] > cols[k - 1]);
  EXPECT(ok);
}

static void re_maps()
{
  const uint32_t prbs[] = {6, 7, 15, 25, 27, 50, 75, 100, 110}, ports[] = {1, 2, 4}, ids[] = {0, 1, 2, 5, 301};
  const uint32_t sfs[]  = {0, 1, 5, 6};
  for (uint32_t np : prbs) {
    // the allocations: full, a fixed pseudo-random one, one that differs between the slots, none
    mi355_pdsch_grant_t alloc[4];
    memset(alloc, 0, sizeof(alloc));
    uint32_t lcg = 1000 + np;
    for (uint32_t n = 0; n < np; n++) {
      alloc[0].prb_idx[0][n] = alloc[0].prb_idx[1][n] = 1;
      alloc[1].prb_idx[0][n] = alloc[1].prb_idx[1][n] = ((lcg = lcg * 1664525u + 1013904223u) >> 24) & 1;
      alloc[2].prb_idx[0][n] = alloc[1].prb_idx[0][n];
      alloc[2].prb_idx[1][n] = ((lcg = lcg * 1664525u + 1013904223u) >> 24) & 1;
    }
    for (uint32_t nports : ports)
      for (uint32_t id : ids)
        for (uint32_t cp = 0; cp < 2; cp++)
          for (uint32_t tdd = 0; tdd < 2; tdd++) {
            const mi355_cell_t c{np, nports, id, cp, tdd, 0, 0};
            for (uint32_t a = 0; a < 4; a++) {
              // nof_symb_slot: 0 (the CP's count) and written out, in turn
              alloc[a].nof_symb_slot[0] = alloc[a].nof_symb_slot[1] = (id & 1) ? (cp ? 6 : 7) : 0;
              for (uint32_t cfi = 1; cfi <= 3; cfi++)
                for (uint32_t sf : sfs) {
                  CTX("map prb=%u ports=%u id=%u cp=%u tdd=%u alloc=%u cfi=%u sf=%u", np, nports, id, cp, tdd, a, cfi, sf);
                  check_map(c, alloc[a], cfi, sf);
                }
            }
            EXPECT(build_re_map(c, alloc[3], 1, 0).n == 0 && build_re_map(c, alloc[3], 1, 0).all.empty());
            EXPECT(build_re_map(c, alloc[0], 2, 3).n > 0);
          }
  }
}

// ---------------------------------------------------------------- FrontLayout

static size_t slot256(size_t n) { return (n + 255) / 256 * 256; } // staged_size (host_staging.h)

static void layouts()
{
  const size_t sizes[2][3] = {{248, 96, 120}, {1, 257, 3}}; // job, codeword, eq_rm job descriptor bytes
  const size_t njobs_[] = {1, 2, 3, 2048}, nds[] = {0, 64, 64 * 1200, (size_t)2048 * 2 * 18496};
  const size_t nes[] = {0, 64, 128 * 999, (size_t)2048 * 2 * 147968}, nparts_[] = {0, 1, 17}, nwts[] = {0, 3 * 57600};
  for (const auto& sz : sizes)
    for (size_t nj : njobs_)
      for (size_t ncw = 0; ncw <= 2 * nj; ncw++) {
        CTX("layout sizes %zu %zu %zu njobs=%zu ncw=%zu", sz[0], sz[1], sz[2], nj, ncw);
        for (size_t nscr : {(size_t)0, std::min<size_t>(1, ncw), ncw})
          for (size_t nd : nds)
            for (size_t ne : nes)
              for (size_t npart : nparts_)
                for (size_t nwt : nwts)
                  for (int er = 0; er < 2; er++) {
                    const FrontLayout l = front_layout(nj, ncw, nscr, nd, ne, npart, nwt, er, sz[0], sz[1], sz[2]);
                    // the regions in the documented order, with their payloads
                    const size_t off[12]  = {l.jobs, l.cws, l.nci,  l.ndst, l.rj,   l.d,   l.csi,
                                             l.e,    l.cmax, l.cfin, l.wtab, l.total};
                    const size_t need[11] = {nj * sz[0], ncw * sz[1], nscr * 4, nscr * 8, er ? nj * sz[2] : 0, nd * 8,
                                             nd * 4,     ne * 2,      nj * 2 * npart * 4, ncw * 4, nwt};
                    bool ok = l.jobs == 0 && l.staged == l.d;
                    for (int k = 0; k < 11; k++) // aligned, at least its payload, ending where the next begins
                      ok &= off[k] % 256 == 0 && off[k + 1] >= off[k] + need[k] && off[k + 1] - off[k] < need[k] + 256;
                    EXPECT(ok);
                    EXPECT(l.staged == slot256(nj * sz[0]) + slot256(ncw * sz[1]) + slot256(nscr * 4) +
                                           slot256(nscr * 8) + (er ? slot256(nj * sz[2]) : 0));
                    EXPECT(l.total == l.staged + slot256(nd * 8) + slot256(nd * 4) + slot256(ne * 2) +
                                          slot256(nj * 2 * npart * 4) + slot256(ncw * 4) + nwt);
                  }
      }
}

// ---------------------------------------------------------------- admission, power, seed

// the switch of plan_job as a table: scheme -> (ports, rx antennas (0: any), layers, transport blocks, largest codebook
// index) rows
static int admit_want(uint32_t cfi, uint32_t sch, uint32_t np, uint32_t nrx, uint32_t L, uint32_t ntb, uint32_t pmi)
{
  if (cfi == 0 || cfi >= 4 || L < 1 || L > 4 || ntb < 1 || ntb > 2 || L < ntb) return MI355_ERROR_INVALID_INPUTS;
  static const uint32_t rows[][6] = {{0, 1, 0, 1, 1, 99}, {1, 2, 0, 2, 1, 99}, {1, 4, 0, 4, 1, 99}, {2, 2, 2, 1, 1, 3},
                                     {2, 2, 2, 2, 2, 2},  {3, 2, 2, 2, 2, 99}};
  const uint32_t cb = ntb == 1 ? pmi : pmi + 1;
  for (const auto& r : rows)
    if (r[0] == sch && r[1] == np && (r[2] == 0 || r[2] == nrx) && r[3] == L && r[4] == ntb && cb <= r[5])
      return MI355_SUCCESS;
  return MI355_ERROR;
}

static void admission()
{
  EXPECT(MI355_SUCCESS == 0 && MI355_ERROR == -1 && MI355_ERROR_INVALID_INPUTS == -2);
  for (uint32_t cfi = 0; cfi <= 4; cfi++)
    for (uint32_t sch = 0; sch <= 3; sch++)
      for (uint32_t np : {1u, 2u, 4u})
        for (uint32_t nrx = 1; nrx <= 2; nrx++)
          for (uint32_t L = 0; L <= 5; L++)
            for (uint32_t ntb = 0; ntb <= 3; ntb++)
              for (uint32_t pmi = 0; pmi <= 3; pmi++) {
                CTX("admit cfi=%u sch=%u np=%u nrx=%u L=%u ntb=%u pmi=%u", cfi, sch, np, nrx, L, ntb, pmi);
                uint32_t  cb = 77;
                const int r = pdsch_admit(cfi, sch, np, nrx, L, ntb, pmi, &cb);
                EXPECT(r == admit_want(cfi, sch, np, nrx, L, ntb, pmi));
                if (r != MI355_ERROR_INVALID_INPUTS) EXPECT(cb == (ntb == 1 ? pmi : pmi + 1));
              }
  CTX("power");
  mi355_pdsch_cfg_t cfg;
  memset(&cfg, 0, sizeof(cfg));
  PdschPower     pw;
  volatile float pa = -3.0f; // (powf at run time here as well)
  cfg.p_b = 7; // not looked at without power_scale
  EXPECT(pdsch_power(cfg, 2, MI355_CP_NORM, 7, &pw) == MI355_SUCCESS && pw.scaling == 1.0f && pw.rhob_inv == 1.0f &&
         pw.rhob_mask == 0);
  cfg.power_scale = 1;
  for (uint32_t pb = 4; pb < 8; pb++) {
    cfg.p_b = pb;
    EXPECT(pdsch_power(cfg, 1, MI355_CP_NORM, 7, &pw) == MI355_ERROR_INVALID_INPUTS);
  }
  cfg.p_b = 0, cfg.p_a = 0.0f; // one port: rho_a = rho_b = 1, nothing to scale
  EXPECT(pdsch_power(cfg, 1, MI355_CP_NORM, 7, &pw) == MI355_SUCCESS && pw.scaling == 1.0f && pw.rhob_inv == 1.0f &&
         pw.rhob_mask == 0);
  cfg.p_b = 1, cfg.p_a = -3.0f; // rho_b = sqrt(4/5): the CRS symbols 0 and 4 (3 with the extended CP) of either slot
  EXPECT(pdsch_power(cfg, 1, MI355_CP_NORM, 7, &pw) == MI355_SUCCESS && pw.rhob_inv == 1.0f / sqrtf(4.0f / 5.0f) &&
         pw.rhob_mask == (1u << 0 | 1u << 4 | 1u << 7 | 1u << 11) && pw.scaling == powf(10.0f, pa / 20.0f));
  cfg.p_b = 2; // rho_b = sqrt(3/4) with more than one port; four ports: symbol 1 too
  EXPECT(pdsch_power(cfg, 4, MI355_CP_EXT, 6, &pw) == MI355_SUCCESS && pw.rhob_mask == (0x0b | 0x0b << 6) && pw.rhob_inv == 1.0f / sqrtf(3.0f / 4.0f) &&
         pw.scaling == (float)((double)powf(10.0f, pa / 20.0f) * 1.4142135623730951));
  cfg.p_b = 1; // two ports: ratio 1, only rho_a
  EXPECT(pdsch_power(cfg, 2, MI355_CP_NORM, 7, &pw) == MI355_SUCCESS && pw.rhob_inv == 1.0f && pw.rhob_mask == 0);
  CTX("c_init"); // 36.211 6.3.1: rnti 2^14 + q 2^13 + floor(ns / 2) 2^9 + cell id, disjoint fields
  EXPECT(pdsch_c_init(0x1234, 1, 13, 301) == (0x1234u << 14 | 1u << 13 | 3u << 9 | 301u));
  EXPECT(pdsch_c_init(0xffff, 0, 9, 503) == (0xffffu << 14 | 9u << 9 | 503u));
}

// ---------------------------------------------------------------- pdsch_eq_rm's job shape

static const uint32_t NOF_SB = 24, MAX_CB = 16;

static bool shape(EqRmTb a, EqRmTb b, bool da, bool db, EqRmShape* s)
{
  const EqRmTb tb[2] = {a, b};
  const bool   dec[2] = {da, db};
  SegCache     fresh;
  static SegCache kept; // as a batch uses it: the previous job's segmentation
  EqRmShape       s2;
  memset(s, 0, sizeof(*s)), memset(&s2, 0, sizeof(s2));
  const bool r = eqrm_job_shape(tb, dec, MAX_CB, NOF_SB, fresh, s), r2 = eqrm_job_shape(tb, dec, MAX_CB, NOF_SB, kept, &s2);
  EXPECT(r == r2);
  if (r) {
    EXPECT(s->nt == s2.nt && s->C == s2.C && s->C1 == s2.C1 && s->K1 == s2.K1 && s->K2 == s2.K2 && s->Qm == s2.Qm);
    EXPECT(s->Gp == s2.Gp && s->n_max == s2.n_max && s->E[0] == s2.E[0] && s->E[1] == s2.E[1] && s->nE == s2.nE);
    EXPECT(s->used[0] == s2.used[0] && s->used[1] == s2.used[1]);
  }
  return r;
}

static void eqrm_shapes()
{
  // one code block (40, 6120: K = 6144), two sizes (6136: K1 = 3136, K2 = 3072), two of one size (6200), filler bits
  // (1001: B = 1025 in K = 1056), 13 and 16 code blocks, 25 (more than max_cb)
  const uint32_t tbss[] = {40, 616, 6120, 6136, 6200, 1001, 75376, 97896, 149776};
  EqRmShape      s;
  for (uint32_t tbs : tbss) {
    CbSegm sg{};
    EXPECT(cbsegm(tbs, &sg) == 0);
    if (tbs == 6136) EXPECT(sg.C == 2 && sg.K1 == 3136 && sg.K2 == 3072 && sg.C1 && sg.C2);
    if (tbs == 1001) EXPECT(sg.F != 0);
    const uint32_t kmin = !sg.C2 ? sg.K1 : !sg.C1 ? sg.K2 : std::min(sg.K1, sg.K2), N = 3 * kmin + 12;
    for (uint32_t qm : {2u, 4u, 6u, 8u}) {
      // few symbols; the most for which every code block has E <= N (its last C - 1 code blocks one symbol more); one more
      const uint32_t gp_fit = sg.C * ((N - qm) / qm) + sg.C - 1, gps[] = {10 * sg.C, 10 * sg.C + 1, gp_fit, gp_fit + 1};
      for (uint32_t gi = 0; gi < 4; gi++)
        for (uint32_t rv = 0; rv < 4; rv++) {
          CTX("eqrm tbs=%u qm=%u gp=%u rv=%u", tbs, qm, gps[gi], rv);
          const uint32_t Gp = gps[gi], gamma = Gp % sg.C;
          const EqRmTb   t{(int32_t)tbs, Gp * qm, qm, rv, 3};
          uint32_t       emax = 0, emin = UINT32_MAX; // per code block (sch.c:391-401)
          for (uint32_t cb = 0; cb < sg.C; cb++) {
            const uint32_t E = qm * (cb + gamma < sg.C ? Gp / sg.C : (Gp + sg.C - 1) / sg.C);
            emax = std::max(emax, E), emin = std::min(emin, E);
          }
          const bool want = sg.F == 0 && sg.C <= MAX_CB && gi != 3;
          const bool got  = shape(t, t, true, true, &s);
          EXPECT(got == want);
          if (!got || !want) continue;
          EXPECT(s.nt == 2 && s.C == sg.C && s.C1 == sg.C1 && s.K1 == sg.K1 && s.K2 == sg.K2 && s.Qm == qm && s.Gp == Gp);
          EXPECT(s.n_max >= emax && s.n_max <= N && s.E[0] == emin && s.E[1] == emin + qm && s.nE == (gamma ? 2u : 1u));
          if (gamma) EXPECT(s.E[1] == emax);
          EXPECT(s.used[0] == (sg.C1 != 0) && s.used[1] == (sg.C2 != 0));
          EXPECT(shape(t, t, true, false, &s) && s.nt == 1 && s.C == sg.C && shape(t, t, false, true, &s) && s.nt == 1);
        }
    }
  }
  CTX("eqrm disqualified");
  const EqRmTb ok{6136, 14000, 2, 1, 5};
  EXPECT(shape(ok, ok, true, true, &s) && s.C == 2 && s.C1 == 1 && s.used[0] && s.used[1] && s.Gp == 7000);
  EXPECT(shape(ok, ok, false, false, &s) && s.nt == 0 && s.C == 0 && s.n_max == 0); // nothing to decode
  EqRmTb b = ok;
  b.rv = 3; // the redundancy versions may differ
  EXPECT(shape(ok, b, true, true, &s));
  b = ok, b.rv = 4;
  EXPECT(!shape(ok, b, true, true, &s) && !shape(b, ok, true, true, &s) && shape(ok, b, true, false, &s));
  b = ok, b.qm = 4;
  EXPECT(!shape(ok, b, true, true, &s) && shape(ok, b, true, false, &s));
  b = ok, b.tbs = 6200;
  EXPECT(!shape(ok, b, true, true, &s));
  b = ok, b.nof_bits = 14002;
  EXPECT(!shape(ok, b, true, true, &s));
  b = ok, b.softbuffer = NOF_SB;
  EXPECT(!shape(ok, b, true, true, &s) && !shape(b, b, true, false, &s));
  b.softbuffer = UINT32_MAX;
  EXPECT(!shape(b, ok, true, true, &s));
  b = ok, b.qm = 0;
  EXPECT(!shape(b, b, true, true, &s));
  b = ok, b.tbs = 0;
  EXPECT(!shape(b, b, true, true, &s));
  b.tbs = -8;
  EXPECT(!shape(b, b, true, true, &s));
}

int main()
{
  re_maps();
  layouts();
  admission();
  eqrm_shapes();
  if (g_failed) {
    fprintf(stderr, "pdsch_plan_check: %d checks failed\n", g_failed);
    return 1;
  }
  printf("pdsch_plan_check: OK\n");
  return 0;
}
