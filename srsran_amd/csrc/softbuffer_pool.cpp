// srsran_amd/csrc/softbuffer_pool.cpp -- the HARQ softbuffer pool of include/srsran_amd/dlsch.h: per code-block slot
// the decoder buffer, the CB-CRC flag, the decoded data and the lazy-reset flag; resets are kernels over the flags.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dlsch_object.h"
#include "runtime_internal.h"
#include "stage_copy.h"

using namespace mi355;

extern "C" {

int mi355_softbuffer_pool_create(mi355_softbuffer_pool_t** p, uint32_t nof_sb, uint32_t max_cb, int device)
{
  if (!p || !nof_sb || !max_cb) return MI355_ERROR_INVALID_INPUTS;
  CHECK_HIP(hipSetDevice(device));
  auto*        s  = new mi355_softbuffer_pool;
  const size_t nc = (size_t)nof_sb * max_cb;
  s->device       = device;
  s->nof_sb       = nof_sb;
  s->max_cb       = max_cb;
  if (hipMalloc(&s->buf, nc * SB_STRIDE * 2) != hipSuccess || hipMalloc(&s->cb_crc, nc) != hipSuccess ||
      hipMalloc(&s->data, nc * SB_DATA) != hipSuccess || hipMalloc(&s->fresh, nc) != hipSuccess) {
    mi355_softbuffer_pool_destroy(s);
    return MI355_ERROR;
  }
  (void)hipMemset(s->fresh, 1, nc); // every buffer starts logically zero
  (void)hipMemset(s->cb_crc, 0, nc);
  (void)hipMemset(s->data, 0, nc * SB_DATA);
  (void)hipDeviceSynchronize();
  *p = s;
  return MI355_SUCCESS;
}

void mi355_softbuffer_pool_destroy(mi355_softbuffer_pool_t* p)
{
  if (!p) return;
  (void)hipFree(p->buf);
  (void)hipFree(p->cb_crc);
  (void)hipFree(p->data);
  (void)hipFree(p->fresh);
  for (int k = 0; k < 2; k++) {
    if (p->ev_armed[k]) (void)hipEventSynchronize(p->ev_list[k]);
    if (p->ev_list[k]) (void)hipEventDestroy(p->ev_list[k]);
  }
  delete p;
}

int mi355_softbuffer_reset_cb(mi355_softbuffer_pool_t* p, uint32_t sb, uint32_t nof_cb, void* stream)
{
  if (!p || sb >= p->nof_sb) return MI355_ERROR_INVALID_INPUTS;
  // softbuffer.c:134-154 clears nof_cb buffers/data and ALL cb_crc flags
  CHECK_HIP(hipSetDevice(p->device));
  hipStream_t    s  = (hipStream_t)stream;
  const uint32_t nc = std::min(nof_cb, p->max_cb);
  DlschResetArgs a{p->fresh, p->cb_crc, (size_t)sb * p->max_cb, nc, p->max_cb}; // one launch for both
  CHECK_HIP(dlsch_launch_reset(a, s));
  if (!s) CHECK_HIP(hipStreamSynchronize(nullptr)); // (dlsch.h: NULL = done on return)
  return MI355_SUCCESS;
}

int mi355_softbuffer_reset(mi355_softbuffer_pool_t* p, uint32_t sb, void* stream)
{
  return mi355_softbuffer_reset_cb(p, sb, p ? p->max_cb : 0, stream);
}

int mi355_softbuffer_reset_tbs(mi355_softbuffer_pool_t* p, uint32_t sb, uint32_t tbs, void* stream)
{
  return mi355_softbuffer_reset_cb(p, sb, (tbs + 24) / (6144 - 24) + 1, stream); // softbuffer.c:128-132
}

int mi355_softbuffer_reset_tbs_batch(mi355_softbuffer_pool_t* p, const uint32_t* sbs, const uint32_t* tbs, uint32_t n,
                                     void* stream)
{
  if (!p || (n && (!sbs || !tbs))) return MI355_ERROR_INVALID_INPUTS;
  if (!n) return MI355_SUCCESS;
  CHECK_HIP(hipSetDevice(p->device));
  hipStream_t    s = (hipStream_t)stream;
  const uint32_t k = p->lpar;
  p->lpar ^= 1u;
  if (n > p->list_cap[k]) {
    if (p->ev_armed[k]) CHECK_HIP(hipEventSynchronize(p->ev_list[k]));
    p->ev_armed[k] = false;
    p->list_cap[k] = n + n / 2 + 64;
    CHECK_HIP(p->d_list[k].alloc(p->list_cap[k] * sizeof(uint2))); // (frees the list this one outgrew)
  }
  if (!p->ev_list[k]) CHECK_HIP(hipEventCreateWithFlags(&p->ev_list[k], hipEventDisableTiming));
  CHECK_HIP(p->st_list.reserve(n * sizeof(uint2)));
  auto* l = (uint2*)p->st_list.slot(n * sizeof(uint2));
  for (uint32_t i = 0; i < n; i++) {
    if (sbs[i] >= p->nof_sb) return MI355_ERROR_INVALID_INPUTS;
    l[i] = make_uint2(sbs[i], std::min((tbs[i] + 24) / (6144 - 24) + 1, p->max_cb)); // softbuffer.c:128-132
  }
  // list buffer k was last read by the reset kernel of the call before last: the copy waits for that one only
  CHECK_HIP(p->st_list.upload(p->d_list[k].p, s, false, p->ev_armed[k] ? p->ev_list[k] : nullptr));
  CHECK_HIP(dlsch_launch_reset_list(p->d_list[k].as<uint2>(), n, p->max_cb, p->fresh, p->cb_crc, s));
  CHECK_HIP(hipEventRecord(p->ev_list[k], s));
  p->ev_armed[k] = true;
  if (!s) CHECK_HIP(hipStreamSynchronize(nullptr)); // (dlsch.h: NULL = done on return)
  return MI355_SUCCESS;
}

int mi355_softbuffer_reset_all(mi355_softbuffer_pool_t* p, void* stream)
{
  if (!p) return MI355_ERROR_INVALID_INPUTS;
  for (uint32_t i = 0; i < p->nof_sb; i++) {
    int r = mi355_softbuffer_reset(p, i, stream);
    if (r) return r;
  }
  return MI355_SUCCESS;
}

int mi355_softbuffer_reset_range(mi355_softbuffer_pool_t* p, uint32_t first, uint32_t n, void* stream)
{
  if (!p || first + n > p->nof_sb) return MI355_ERROR_INVALID_INPUTS;
  if (!n) return MI355_SUCCESS;
  CHECK_HIP(hipSetDevice(p->device));
  DlschResetArgs a{p->fresh, p->cb_crc, (size_t)first * p->max_cb, (size_t)n * p->max_cb, 0};
  CHECK_HIP(dlsch_launch_reset(a, (hipStream_t)stream));
  if (!stream) CHECK_HIP(hipStreamSynchronize(nullptr)); // (dlsch.h: NULL = done on return)
  return MI355_SUCCESS;
}

int mi355_softbuffer_pool_buffer(mi355_softbuffer_pool_t* p, int16_t** buf, uint32_t* stride, uint32_t* max_cb)
{
  if (!p) return MI355_ERROR_INVALID_INPUTS;
  if (buf) *buf = p->buf;
  if (stride) *stride = SB_STRIDE;
  if (max_cb) *max_cb = p->max_cb;
  return MI355_SUCCESS;
}

int mi355_softbuffer_pool_materialize(mi355_softbuffer_pool_t* p, uint32_t first, uint32_t n, void* stream)
{
  if (!p || first > p->nof_sb || n > p->nof_sb - first) return MI355_ERROR_INVALID_INPUTS;
  CHECK_HIP(hipSetDevice(p->device));
  CHECK_HIP(dlsch_launch_materialize(p->buf, SB_STRIDE, p->fresh, (size_t)first * p->max_cb, n * p->max_cb,
                                     (hipStream_t)stream));
  if (!stream) CHECK_HIP(hipStreamSynchronize(nullptr));
  return MI355_SUCCESS;
}

int mi355_softbuffer_pool_data(mi355_softbuffer_pool_t* p, uint8_t** data, uint32_t* stride, uint32_t* nof_sb)
{
  if (!p) return MI355_ERROR_INVALID_INPUTS;
  if (data) *data = p->data;
  if (stride) *stride = SB_DATA;
  if (nof_sb) *nof_sb = p->nof_sb;
  return MI355_SUCCESS;
}

int mi355_softbuffer_get_cb_crc(mi355_softbuffer_pool_t* p, uint32_t sb, uint8_t* cb_crc, void* stream)
{
  if (!p || !cb_crc || sb >= p->nof_sb) return MI355_ERROR_INVALID_INPUTS;
  CHECK_HIP(hipSetDevice(p->device));
  hipStream_t s = (hipStream_t)stream;
  CHECK_HIP(hipMemcpyAsync(cb_crc, p->cb_crc + (size_t)sb * p->max_cb, p->max_cb, hipMemcpyDeviceToHost, s));
  CHECK_HIP(wait_stream(s));
  return MI355_SUCCESS;
}

int mi355_softbuffer_get_cb_crc_async(mi355_softbuffer_pool_t* p, uint32_t sb, uint8_t* cb_crc, void* stream)
{
  if (!p || !cb_crc || sb >= p->nof_sb) return MI355_ERROR_INVALID_INPUTS;
  CHECK_HIP(hipSetDevice(p->device));
  CHECK_HIP(hipMemcpyAsync(cb_crc, p->cb_crc + (size_t)sb * p->max_cb, p->max_cb, hipMemcpyDeviceToHost,
                           (hipStream_t)stream));
  return MI355_SUCCESS;
}

int mi355_softbuffer_cb_crc_dev(mi355_softbuffer_pool_t* p, uint32_t sb, const uint8_t** d_cb_crc)
{
  if (!p || !d_cb_crc || sb >= p->nof_sb) return MI355_ERROR_INVALID_INPUTS;
  *d_cb_crc = p->cb_crc + (size_t)sb * p->max_cb;
  return MI355_SUCCESS;
}

} // extern "C"

mi355::SoftbufferView mi355::softbuffer_view(mi355_softbuffer_pool_t* p)
{
  return SoftbufferView{p->buf, SB_STRIDE, p->cb_crc, p->fresh, p->nof_sb, p->max_cb};
}
