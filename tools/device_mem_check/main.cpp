// tools/device_mem_check/main.cpp -- host check of the ownership logic in srsran_amd/csrc/device_mem.h against the
// stub HIP calls beside this file, for a sanitizer build (no GPU, nothing preloaded):
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Itools/device_mem_check
//       -Isrsran_amd/csrc tools/device_mem_check/main.cpp -o /tmp/device_mem_check && /tmp/device_mem_check
// Checks: move semantics, upload = copy + null-stream wait, a cache entry is inserted only after its build succeeded
// (a build that fails midway leaves nothing behind and leaks nothing), the allocate-only lookup, Retire keeps outgrown
// buffers until destruction and frees each once, SyncFree waits for the device and keeps nothing; allocations and
// frees balance after destruction.
#include <stdint.h>
#include <stdio.h>
#include <unordered_map>

#define MI355_ERROR -1
#include "device_mem.h"

using namespace mi355;

static int g_failed = 0;
#define EXPECT(c)                                                                                                      \
  do {                                                                                                                 \
    if (!(c)) {                                                                                                        \
      fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #c);                                          \
      g_failed++;                                                                                                      \
    }                                                                                                                  \
  } while (0)

struct Two { // an entry of two tables, as the turbo decoder's per-K tables
  DevMem a, b;
  int    n = 0;
};

static int build_two(Two& t, const std::vector<uint32_t>& v)
{
  CHECK_HIP(t.a.upload(v));
  CHECK_HIP(t.b.upload(v)); // (the second allocation is the one told to fail)
  t.n = (int)v.size();
  return 0;
}

static void dev_mem()
{
  const std::vector<uint16_t> v(100, 7);
  DevMem                      a;
  EXPECT(a.upload(v) == hipSuccess && a.bytes == 200 && g_hip.copies == 1 && g_hip.stream_syncs == 1);
  EXPECT(!memcmp(a.p, v.data(), 200));
  void* p = a.p;
  EXPECT(a.upload(v.data(), 50) == hipSuccess && a.p == p && g_hip.allocs == 1); // fits: reused
  DevMem b(std::move(a));
  EXPECT(!a.p && !a.bytes && b.p == p);
  DevMem c;
  EXPECT(c.alloc(10) == hipSuccess);
  c = std::move(b); // c's old allocation ends up in b and is freed with it
  EXPECT(c.p == p && b.bytes == 10);
  EXPECT(c.alloc(400) == hipSuccess && g_hip.frees == 1); // alloc frees what was held
  g_hip.fail_alloc = 1;
  EXPECT(c.alloc(8) != hipSuccess && !c.p && !c.bytes);
}

static void dev_cache()
{
  const std::vector<uint32_t> v(16, 3);
  DevCache<uint32_t, Two>     cache;
  Two*                        t = nullptr;
  g_hip.fail_alloc               = 2; // the build's second table
  EXPECT(cache.get(5, &t, [&](Two& e) { return build_two(e, v); }) == MI355_ERROR);
  EXPECT(cache.size() == 0 && !t && g_hip.allocs == g_hip.frees); // nothing inserted, the first table freed
  EXPECT(cache.get(5, &t, [&](Two& e) { return build_two(e, v); }) == 0 && t && t->n == 16);
  EXPECT(cache.get(6, &t, [&](Two&) { return -2; }) == -2 && cache.size() == 1); // the site's own error code
  Two* again  = nullptr;
  int  builds = 0;
  EXPECT(cache.get(5, &again, [&](Two&) { return builds++, 0; }) == 0 && again && again->n == 16 && !builds); // found

  DevCache<uint32_t, DevMem, std::unordered_map<uint32_t, DevMem>> seq;
  void* d     = nullptr;
  bool  fresh = false;
  EXPECT(seq.get_alloc(9, 64, &d, &fresh) == hipSuccess && fresh && d);
  void* d2 = nullptr;
  EXPECT(seq.get_alloc(9, 64, &d2, &fresh) == hipSuccess && !fresh && d2 == d);
  g_hip.fail_alloc = 1;
  EXPECT(seq.get_alloc(10, 64, &d2, &fresh) != hipSuccess && seq.size() == 1);
  const int frees = g_hip.frees;
  seq.clear();
  EXPECT(seq.size() == 0 && g_hip.frees == frees + 1);
}

static void dev_scratch()
{
  {
    DevScratch s;
    bool       grew = false;
    EXPECT(s.reserve(100, 128, DevScratch::Retire, &grew) == hipSuccess && grew && s.cap() == 128);
    char* p = s.base();
    grew    = false;
    EXPECT(s.reserve(128, 999, DevScratch::Retire, &grew) == hipSuccess && !grew && s.base() == p);
    const int frees = g_hip.frees, syncs = g_hip.device_syncs;
    EXPECT(s.reserve(129, 256, DevScratch::Retire, &grew) == hipSuccess && grew && s.cap() == 256);
    EXPECT(s.retired.size() == 1 && s.retired[0].p == p && g_hip.frees == frees && g_hip.device_syncs == syncs);
    g_hip.fail_alloc = 1;
    EXPECT(s.reserve(300, 512, DevScratch::Retire) != hipSuccess && !s.base() && s.cap() == 0 && s.retired.size() == 2);
    EXPECT(s.reserve(300, 512, DevScratch::Retire) == hipSuccess && s.retired.size() == 2);
  } // destructor: the buffer and both retired ones, once each
  {
    DevScratch s;
    EXPECT(s.reserve(100, 128, DevScratch::SyncFree) == hipSuccess && g_hip.device_syncs == 0);
    const int frees = g_hip.frees;
    EXPECT(s.reserve(200, 256, DevScratch::SyncFree) == hipSuccess && g_hip.device_syncs == 1);
    EXPECT(g_hip.frees == frees + 1 && s.retired.empty() && s.cap() == 256);
  }
}

int main()
{
  for (auto* f : {&dev_mem, &dev_cache, &dev_scratch}) {
    g_hip = StubHip{};
    (*f)();
    EXPECT(g_hip.allocs == g_hip.frees); // everything the part allocated was freed exactly once
  }
  printf("device_mem_check: %s\n", g_failed ? "FAILED" : "ok");
  return g_failed ? 1 : 0;
}
