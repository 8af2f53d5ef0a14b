// srsran_amd/csrc/pdsch_maps.cpp -- the PDSCH receiver's two device caches: RE extraction maps, built on the host
// (pdsch_re_map.h) once per (grant allocation, cfi, subframe), and packed descrambling sequences per c_init, filled by
// the front end's pdsch_scr_pack.  Both are bounded once per call.
#include <hip/hip_runtime.h>

#include <string.h>
#include <string>

#include "pdsch_object.h"
#include "pdsch_re_map.h"

namespace mi355 {

// Bound the map cache, once per call and before any job of the batch is planned: a map handed to a job stays intact
// until the next call on this receiver begins (the batch's front end and mi355_pdsch_debug_stage's on-demand
// pdsch_eq_llr read it), so the bound is soft by one batch's distinct allocations.  The maps' last readers are the
// front-end kernels of the previous batch (fe_done; the debug stage waits for its own kernel): once they are done the
// buffers are reused for new maps, without a free (hipFree would wait for the whole device).
int trim_maps(mi355_pdsch_t* q)
{
  if (q->maps.size() < q->max_maps) return MI355_SUCCESS;
  if (q->fe_armed) CHECK_HIP(wait_event(q->fe_done));
  for (auto& kv : q->maps.map) q->map_free.push_back(std::move(kv.second.mem));
  q->maps.clear();
  for (auto& m : q->last_map) m = MapEntry{};
  return MI355_SUCCESS;
}

int get_map(mi355_pdsch_t* q, const mi355_pdsch_grant_t& g, uint32_t cfi, uint32_t sf, MapEntry* out)
{
  // the jobs of a batch usually share the allocation: compare with the previous lookup of this subframe index first
  const uint32_t  np = q->cell.nof_prb, z = sf % 10;
  const uint32_t  hdr[4] = {cfi, sf, g.nof_symb_slot[0], g.nof_symb_slot[1]};
  if (q->last_map[z].d && !memcmp(q->last_map_hdr[z], hdr, sizeof(hdr)) &&
      !memcmp(q->last_map_prb[z][0], g.prb_idx[0], np) && !memcmp(q->last_map_prb[z][1], g.prb_idx[1], np)) {
    *out = q->last_map[z];
    return MI355_SUCCESS;
  }
  std::string key;
  key.reserve(16 + 2 * np);
  key.append((const char*)hdr, sizeof(hdr));
  key.append((const char*)g.prb_idx[0], np);
  key.append((const char*)g.prb_idx[1], np);
  MapSlot* slot = nullptr;
  int      r    = q->maps.get(key, &slot, [&](MapSlot& e) -> int {
    const ReMapImage m = build_re_map(q->cell, g, cfi, sf);
    e.n = m.n, e.g0 = m.g0, e.g1 = m.g1, e.ncols = m.ncols;
    const size_t need = std::max<size_t>(m.all.size(), 1) * sizeof(uint16_t);
    for (size_t k = 0; k < q->map_free.size(); k++) // an evicted map's buffer that fits
      if (q->map_free[k].bytes >= need) {
        std::swap(e.mem, q->map_free[k]);
        std::swap(q->map_free[k], q->map_free.back());
        q->map_free.pop_back();
        break;
      }
    if (!e.mem.p) CHECK_HIP(e.mem.alloc(need));
    CHECK_HIP(e.mem.upload(m.all)); // into the buffer just chosen (waits for the copy to land, device_mem.h)
    e.d = e.mem.as<uint16_t>();
    return MI355_SUCCESS;
  });
  if (r) return r;
  *out           = *slot;
  q->last_map[z] = *slot;
  memcpy(q->last_map_hdr[z], hdr, sizeof(hdr));
  memcpy(q->last_map_prb[z][0], g.prb_idx[0], np);
  memcpy(q->last_map_prb[z][1], g.prb_idx[1], np);
  return MI355_SUCCESS;
}

// bound the sequence cache (~76 MB at 4096), once per call and before its look-ups; waits for the calling stream only
int trim_scr(mi355_pdsch_t* q, hipStream_t s)
{
  if (q->scr.size() <= q->max_scr) return MI355_SUCCESS;
  CHECK_HIP(hipStreamSynchronize(s));
  q->scr.clear();
  return MI355_SUCCESS;
}

int get_scr(mi355_pdsch_t* q, uint32_t c_init, uint32_t** d, bool* fresh)
{
  void* p = nullptr;
  CHECK_HIP(q->scr.get_alloc(c_init, (PDSCH_GOLD_MAX / 32) * 4, &p, fresh));
  *d = (uint32_t*)p;
  return MI355_SUCCESS;
}

} // namespace mi355
