// srsran_amd/csrc/device_mem.h -- ownership of the host runtimes' device memory: one-shot tables (DevMem), keyed table
// caches (DevCache) and grow-only scratch (DevScratch).  Everything here frees in its destructor; every destroy() does
// hipSetDevice + hipDeviceSynchronize before `delete q`, so the members' destructors run with the device idle.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <stddef.h>
#include <stdio.h>
#include <utility>
#include <vector>

// (expects MI355_ERROR from the public headers at the point of use)
#define CHECK_HIP(x)                                                                                                   \
  do {                                                                                                                 \
    hipError_t e_ = (x);                                                                                               \
    if (e_ != hipSuccess) {                                                                                            \
      fprintf(stderr, "[srsran_amd] %s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));                 \
      return MI355_ERROR;                                                                                              \
    }                                                                                                                  \
  } while (0)

namespace mi355 {

// one owned device allocation
struct DevMem {
  void*  p     = nullptr;
  size_t bytes = 0; // capacity of p

  DevMem() = default;
  DevMem(DevMem&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
  DevMem& operator=(DevMem&& o) noexcept
  {
    std::swap(p, o.p);
    std::swap(bytes, o.bytes);
    return *this;
  }
  ~DevMem() { reset(); }
  // hipFree waits for the whole device: only where nothing can be in flight, or the caller has synchronised
  void reset()
  {
    if (p) (void)hipFree(p);
    p = nullptr, bytes = 0;
  }
  template <class T> T* as() const { return (T*)p; }
  // a fresh allocation (hipMalloc alignment >= 256 B); whatever was held is freed first
  hipError_t alloc(size_t n)
  {
    reset();
    hipError_t e = hipMalloc(&p, n);
    if (e == hipSuccess) bytes = n;
    else p = nullptr;
    return e;
  }
  // host -> device, into the held allocation where it is large enough.  A pageable-source copy may return before its
  // DMA lands, and the kernels that read the table run on non-blocking streams the null stream does not order against:
  // hence the wait, paid once per table.
  hipError_t upload(const void* host, size_t n)
  {
    hipError_t e = hipSuccess;
    if ((!p || n > bytes) && (e = alloc(n)) != hipSuccess) return e;
    if (!n) return hipSuccess;
    if ((e = hipMemcpy(p, host, n, hipMemcpyHostToDevice)) != hipSuccess) return e;
    return hipStreamSynchronize(nullptr);
  }
  template <class T> hipError_t upload(const std::vector<T>& v) { return upload(v.data(), v.size() * sizeof(T)); }
};

// Device tables built on first use, by key.  Entry owns its device memory through DevMem members and keeps whatever
// small fields the site wants beside them; Map is the site's container (std::map or std::unordered_map of Key to Entry).
template <class Key, class Entry = DevMem, class Map = std::map<Key, Entry>> struct DevCache {
  Map map;

  // find, else build(entry) (0, or the site's error code) and insert.  The entry is built outside the map and moved
  // in only once build has uploaded all of it: a failed build inserts nothing and its allocations are freed here.
  template <class Build> int get(const Key& key, Entry** out, Build build)
  {
    auto it = map.find(key);
    if (it == map.end()) {
      Entry e;
      int   r = build(e);
      if (r) return r;
      it = map.emplace(key, std::move(e)).first;
    }
    *out = &it->second;
    return 0;
  }
  // allocate-only lookup (Entry = DevMem) for tables a kernel fills later: *fresh tells the caller to queue the fill
  hipError_t get_alloc(const Key& key, size_t bytes, void** out, bool* fresh)
  {
    auto it = map.find(key);
    *fresh  = it == map.end();
    if (*fresh) {
      DevMem     m;
      hipError_t e = m.alloc(bytes);
      if (e != hipSuccess) return e;
      it = map.emplace(key, std::move(m)).first;
    }
    *out = it->second.p;
    return hipSuccess;
  }
  size_t size() const { return map.size(); }
  // frees every entry (hipFree): the caller has waited for the entries' readers
  void clear() { map.clear(); }
};

// Grow-only scratch / workspace.
struct DevScratch {
  // Retire: the outgrown buffer may still be read by the owner's batch in flight, and hipFree would wait for the whole
  //   device (stalling every other worker's stream): kept on the retired list until destruction.
  // SyncFree: hipDeviceSynchronize, free, allocate -- for workspaces too large to keep.
  enum Policy { Retire, SyncFree };
  DevMem              cur;
  std::vector<DevMem> retired;

  char*  base() const { return (char*)cur.p; }
  size_t cap() const { return cur.bytes; }
  // at least `bytes`; a buffer that has to grow is allocated with grown_cap (the site's headroom formula) and
  // *grew is set (left alone otherwise)
  hipError_t reserve(size_t bytes, size_t grown_cap, Policy policy, bool* grew = nullptr)
  {
    if (bytes <= cur.bytes) return hipSuccess;
    if (cur.p) {
      if (policy == Retire) {
        retired.push_back(std::move(cur));
      } else {
        hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess) return e;
      }
    }
    if (grew) *grew = true;
    return cur.alloc(grown_cap);
  }
};

} // namespace mi355
