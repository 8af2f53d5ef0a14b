// srsran_amd/csrc/host_env.h -- the environment knobs the ue_dl and control-stage runtimes share, each read once
// (INTEGRATION.md lists them), and the clock behind the "[mi355 host]" phase timings.
#pragma once
#include <chrono>
#include <stdint.h>
#include <stdlib.h>

namespace mi355 {

inline int env_int(const char* name) { return getenv(name) ? atoi(getenv(name)) : 0; }

// one-subframe calls: descriptors in the kernel arguments (MI355_NO_INLINE_JOBS=1: always uploaded, A/B timing)
inline bool env_inline_jobs() { static const bool v = env_int("MI355_NO_INLINE_JOBS") == 0; return v; }
// MI355_HOST_PROF: host-side phase timing to stderr
inline bool env_host_prof() { static const bool v = getenv("MI355_HOST_PROF") != nullptr; return v; }
// MI355_UEDL_CHUNKS = 1..8: find_and_decode's chunk count where mi355_ue_dl_set_chunks has not set one (else 0)
inline uint32_t env_uedl_chunks() { static const int v = env_int("MI355_UEDL_CHUNKS"); return v >= 1 && v <= 8 ? v : 0; }
// MI355_UEDL_SPLIT0 = 1..99 (A/B timing): the first of two chunks' share in percent (else 0)
inline uint32_t env_uedl_split0() { static const int v = env_int("MI355_UEDL_SPLIT0"); return v > 0 && v < 100 ? v : 0; }

using HostTime = std::chrono::steady_clock::time_point;
inline HostTime host_now() { return std::chrono::steady_clock::now(); }
inline double   host_us(HostTime a, HostTime b) { return std::chrono::duration<double, std::micro>(b - a).count(); }

} // namespace mi355
