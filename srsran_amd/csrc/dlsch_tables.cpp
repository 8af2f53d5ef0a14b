// srsran_amd/csrc/dlsch_tables.cpp -- the DL-SCH object's device tables: built by dlsch_tables.h on first use, uploaded
// and cached in the object by key.
#include <hip/hip_runtime.h>

#include "dlsch_object.h"
#include "dlsch_tables.h"
#include "runtime_internal.h"

using namespace mi355;

// cache[key] as a T table: on a miss the vector build() returns, uploaded
template <class T, class Key, class Build> static int cached(DevCache<Key>& cache, Key key, const T** out, Build build)
{
  DevMem* m = nullptr;
  int     e = cache.get(key, &m, [&](DevMem& d) -> int {
    CHECK_HIP(d.upload(build()));
    return MI355_SUCCESS;
  });
  if (!e) *out = m->as<T>();
  return e;
}

static uint64_t rm_key(uint32_t K, uint32_t rv) { return ((uint64_t)K << 2) | rv; }

int mi355::dlsch_rm16_inv(mi355_dlsch_t* q, uint32_t K, uint32_t rv, const uint16_t** out)
{
  return cached(q->rm, rm_key(K, rv), out, [&] { return rm16_table(K, rv); });
}

int mi355::dlsch_rm8_inv(mi355_dlsch_t* q, uint32_t K, uint32_t rv, const uint16_t** out)
{
  return cached(q->rm8, rm_key(K, rv), out, [&] { return rm8_inv_table(K, rv); });
}

int mi355::dlsch_crc_scales(mi355_dlsch_t* q, uint32_t K, const uint32_t** out)
{
  return cached(q->scales, K, out, [&] { return crc_scales_table(K); });
}

int mi355::dlsch_tb_crc_scales(mi355_dlsch_t* q, uint32_t nbytes, const uint32_t** out)
{
  return cached(q->tb_scales, nbytes, out, [&] { return tb_crc_scales_table(nbytes); });
}

int mi355::dlsch_rm_inv(mi355_dlsch_t* q, uint32_t K, uint32_t rv, const uint16_t** out)
{
  if (!q || rv > 3) return MI355_ERROR_INVALID_INPUTS;
  std::lock_guard<std::mutex> lock(q->mu);
  CHECK_HIP(hipSetDevice(q->device));
  return dlsch_rm16_inv(q, K, rv, out);
}

uint32_t mi355::dlsch_rm_buflen(uint32_t K) { return rm_buflen(K); }

int mi355::dlsch_rm_compact(mi355_dlsch_t* q, uint32_t K, uint32_t rv, uint32_t E, const uint16_t** tab, uint32_t* nq,
                            uint32_t* qoff)
{
  if (!q || rv > 3 || E == 0 || E > 3 * K + 12) return MI355_ERROR_INVALID_INPUTS;
  std::lock_guard<std::mutex> lock(q->mu);
  CHECK_HIP(hipSetDevice(q->device));
  mi355_dlsch::Compact* c = nullptr;
  int e = q->rmc.get((rm_key(K, rv) << 16) | E, &c, [&](mi355_dlsch::Compact& ent) -> int {
    const RmCompact t = rm_compact_table(K, rv, E);
    if (t.tab.empty()) return MI355_ERROR;
    CHECK_HIP(ent.d.upload(t.tab));
    ent.nq = t.nq, ent.qoff = t.qoff;
    return MI355_SUCCESS;
  });
  if (e) return e;
  *tab  = c->d.as<uint16_t>();
  *nq   = c->nq;
  *qoff = c->qoff;
  return MI355_SUCCESS;
}
