// srsran_amd/csrc/sync_host.cpp -- host functions of the cell search: the PSS / SSS sequences and their tables, the
// put_slot functions and the cell-search vote.  No GPU work here.
#include <string.h>

#include <vector>

#include "sync_internal.h"

namespace mi355 {

namespace {

// the three m-sequences of 36.211 6.11.2.1 as +-1 (generate_zsc_tilde): x(i+5) from the listed taps, x(4) = 1
void m_sequences(int* s_t, int* c_t, int* z_t)
{
  auto run = [](int* out, std::initializer_list<int> taps) {
    int x[SSS_N] = {0};
    x[4]         = 1;
    for (uint32_t i = 0; i + 5 < SSS_N; i++) {
      int v = 0;
      for (int t : taps) v += x[i + t];
      x[i + 5] = v % 2;
    }
    for (uint32_t i = 0; i < SSS_N; i++) out[i] = 1 - 2 * x[i];
  };
  run(s_t, {2, 0});
  run(c_t, {3, 0});
  run(z_t, {4, 2, 1, 0});
}

} // namespace

void sss_m0m1(uint32_t n_id_1, uint32_t* m0, uint32_t* m1)
{
  const uint32_t qp = n_id_1 / 30, q = (n_id_1 + qp * (qp + 1) / 2) / 30, mp = n_id_1 + q * (q + 1) / 2;
  *m0 = mp % SSS_N;
  *m1 = (*m0 + mp / SSS_N + 1) % SSS_N;
}

void sss_tables(SssTables* t)
{
  int s_t[SSS_N], c_t[SSS_N], z_t[SSS_N];
  m_sequences(s_t, c_t, z_t);
  memset(t, 0, sizeof(*t));
  for (uint32_t m = 0; m < SSS_N; m++)
    for (uint32_t i = 0; i < SSS_N; i++) {
      t->s[m][i]  = (float)s_t[(i + m) % SSS_N];
      t->z1[m][i] = (float)z_t[(i + m % 8) % SSS_N];
    }
  for (uint32_t m = 0; m < SSS_N; m++)
    for (uint32_t i = 0; i + 1 < SSS_N; i++) t->sd[m][i] = t->s[m][i + 1] * t->s[m][i];
  for (uint32_t id2 = 0; id2 < SYNC_HYPS; id2++)
    for (uint32_t i = 0; i < SSS_N; i++) {
      t->c[id2][0][i] = (float)c_t[(i + id2) % SSS_N];
      t->c[id2][1][i] = (float)c_t[(i + id2 + 3) % SSS_N];
    }
  for (uint32_t id1 = 0; id1 < 168; id1++) {
    uint32_t m0, m1;
    sss_m0m1(id1, &m0, &m1);
    t->n_id_1[m0][m1 - 1] = id1;
  }
}

} // namespace mi355

using namespace mi355;

extern "C" {

int mi355_pss_generate(uint32_t n_id_2, float* pss62)
{
  if (n_id_2 > 2 || !pss62) return MI355_ERROR_INVALID_INPUTS;
  pss_sequence(n_id_2, (float2*)pss62);
  return MI355_SUCCESS;
}

int mi355_sss_generate(uint32_t cell_id, float* sf0_62, float* sf5_62)
{
  if (cell_id > 503 || !sf0_62 || !sf5_62) return MI355_ERROR_INVALID_INPUTS;
  static const SssTables* T = [] {
    auto* t = new SssTables;
    sss_tables(t);
    return t;
  }();
  uint32_t m0, m1;
  sss_m0m1(cell_id / 3, &m0, &m1);
  const float *c0 = T->c[cell_id % 3][0], *c1 = T->c[cell_id % 3][1];
  for (uint32_t i = 0; i < SSS_N; i++) {
    sf0_62[2 * i]     = T->s[m0][i] * c0[i];
    sf0_62[2 * i + 1] = T->s[m1][i] * c1[i] * T->z1[m0][i];
    sf5_62[2 * i]     = T->s[m1][i] * c0[i];
    sf5_62[2 * i + 1] = T->s[m0][i] * c1[i] * T->z1[m1][i];
  }
  return MI355_SUCCESS;
}

void mi355_pss_put_slot(const float* pss62, float* slot, uint32_t nof_prb, uint32_t cp)
{
  const uint32_t nsymb = cp == MI355_CP_NORM ? 7 : 6, nre = 12 * nof_prb;
  const uint32_t k     = (nsymb - 1) * nre + nre / 2 - 31;
  memset(slot + 2 * (k - 5), 0, 5 * 2 * sizeof(float));
  memcpy(slot + 2 * k, pss62, MI355_PSS_LEN * 2 * sizeof(float));
  memset(slot + 2 * (k + MI355_PSS_LEN), 0, 5 * 2 * sizeof(float));
}

void mi355_sss_put_slot(const float* sss62, float* slot, uint32_t nof_prb, uint32_t cp)
{
  const uint32_t nsymb = cp == MI355_CP_NORM ? 7 : 6, nre = 12 * nof_prb;
  const uint32_t k     = (nsymb - 2) * nre + nre / 2 - 31;
  if (k <= 5) return;
  memset(slot + 2 * (k - 5), 0, 5 * 2 * sizeof(float));
  for (uint32_t i = 0; i < MI355_SSS_LEN; i++) slot[2 * (k + i)] = sss62[i], slot[2 * (k + i) + 1] = 0.f;
  memset(slot + 2 * (k + MI355_SSS_LEN), 0, 5 * 2 * sizeof(float));
}

int mi355_cellsearch_pick(const mi355_sync_res_t* found, uint32_t n, mi355_cellsearch_res_t* out)
{
  if (!found || !out || !n) return MI355_ERROR_INVALID_INPUTS;
  // the reference's mode count: candidate i counts itself and every later, not yet counted candidate of its id
  std::vector<uint8_t>  counted(n, 0);
  std::vector<uint32_t> ntimes(n, 0);
  for (uint32_t i = 0; i < n; i++) {
    uint32_t cnt = 1;
    for (uint32_t j = i + 1; j < n; j++)
      if (found[j].cell_id == found[i].cell_id && !counted[j]) counted[j] = 1, cnt++;
    ntimes[i] = cnt;
  }
  uint32_t max_times = 0, mode_pos = 0;
  for (uint32_t i = 0; i < n; i++)
    if (ntimes[i] > max_times) max_times = ntimes[i], mode_pos = i;
  memset(out, 0, sizeof(*out));
  out->cell_id      = (uint32_t)found[mode_pos].cell_id;
  uint32_t nof_norm = 0, nof_fdd = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (found[i].cell_id == found[mode_pos].cell_id) {
      nof_norm += found[i].cp == MI355_CP_NORM;
      nof_fdd += found[i].frame_type == MI355_FDD;
    }
    out->peak += found[i].peak_abs;
  }
  out->peak /= n;
  out->cp         = nof_norm > ntimes[mode_pos] / 2 ? MI355_CP_NORM : MI355_CP_EXT;
  out->frame_type = nof_fdd > ntimes[mode_pos] / 2 ? MI355_FDD : MI355_TDD;
  out->mode       = (float)ntimes[mode_pos] / n;
  out->psr        = found[n - 1].peak_value;
  out->cfo        = found[n - 1].cfo_pss_mean;
  return MI355_SUCCESS;
}

} // extern "C"
