// srsran_amd/csrc/host_env.h -- the environment knobs of the host runtimes (ue_dl, control stage, PDSCH, DL-SCH), each read
// once unless it says otherwise (INTEGRATION.md lists them), and the clock behind the "[mi355 host]" phase timings.
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

// MI355_DLSCH_LAT_CBS: the DL-SCH latency path's code-block limit until mi355_dlsch_set_latency_path sets one (0: off);
// read by the first call that needs the limit (dlsch_runtime.cpp keeps the value)
inline int env_dlsch_lat_cbs() { return getenv("MI355_DLSCH_LAT_CBS") ? atoi(getenv("MI355_DLSCH_LAT_CBS")) : 256; }
// MI355_TDEC_SPEC=0 (A/B timing): no speculative DEC2 half-iterations
inline bool env_tdec_spec() { static const bool v = !getenv("MI355_TDEC_SPEC") || env_int("MI355_TDEC_SPEC") != 0; return v; }
// MI355_NO_ROWMASK=1 (A/B timing): the MAP kernel reads every parity row
inline bool env_no_rowmask() { static const bool v = env_int("MI355_NO_ROWMASK") != 0; return v; }
// MI355_LAT_WAVES=4 (A/B timing): latency-path workgroups of four waves, the beta recursion in wave 2
inline bool env_lat_waves4() { static const bool v = env_int("MI355_LAT_WAVES") == 4; return v; }
// latency path: two more waves per code block compute the second parts' output passes beside the recursions
// (tdec_win_lat.hip); MI355_LAT_OWAVES=0 keeps them in the recursion waves (A/B timing)
inline bool env_lat_owaves() { static const bool v = !getenv("MI355_LAT_OWAVES") || env_int("MI355_LAT_OWAVES") != 0; return v; }
// MI355_RM_SPARSE=0 (A/B timing): fresh decoder buffers written whole, zero parity rows included
inline bool env_rm_sparse() { static const bool v = !getenv("MI355_RM_SPARSE") || env_int("MI355_RM_SPARSE") != 0; return v; }

// MI355_NO_EQRM (A/B, tests): never pdsch_eq_rm.  Set means present, whatever the value; read on every call (tests set
// and clear it within one process)
inline bool env_no_eqrm() { return getenv("MI355_NO_EQRM") != nullptr; }
// MI355_EQRM_COMPACT=0 (A/B timing): pdsch_eq_rm's lean path gathers through the inverse table, no compact image
inline bool env_eqrm_compact() { static const bool v = !getenv("MI355_EQRM_COMPACT") || env_int("MI355_EQRM_COMPACT") != 0; return v; }
// MI355_EQRM_DIAG (measurement only, wrong results): 1 = pdsch_eq_rm without rate dematching, 2 = without equalisation
inline int env_eqrm_diag() { static const int v = env_int("MI355_EQRM_DIAG"); return v; }

using HostTime =std::chrono::steady_clock::time_point;
inline HostTime host_now() { return std::chrono::steady_clock::now(); }
inline double   host_us(HostTime a, HostTime b) { return std::chrono::duration<double, std::micro>(b - a).count(); }

} // namespace mi355
