// srsran_amd/csrc/dlsch_layout.h -- what the DL-SCH's host planning and table builders (dlsch_plan.h, dlsch_tables.h)
// share with its kernels: the softbuffer slot layout, the TB descriptor, the CRC table and the inverse rate-dematching
// table's extent.  Host-only C++: nothing here needs the HIP headers (dlsch_internal.h adds the kernels' argument blocks).
#pragma once
#include <stdint.h>

#define SB_STRIDE 18600 // SOFTBUFFER_SIZE (softbuffer.h:50): int16 per code-block softbuffer
#define SB_DATA 768     // bytes of decoded CB data kept per code block (softbuffer.c:146)
#define SB_CONV8 10240  // int16 offset in a slot of the converted copy of an int8 K <= 400 buffer (8-bit mode)
// parity-row bitmaps of a 16-window decoder buffer (K multiple of 16, 800 < K <= 6144, L = K / 16 <= 384 rows): at int16
// offset SB_ROWMASK of the slot (past the 3 (K + 32) + 12 = 18,540 entries of K = 6144), SB_ROWMASK_WORDS u32 for P0,
// then as many for P1; bit j: row j (the 16 windows' entries of step j) holds an LLR.  Written by every 16-bit rate
// dematcher into the slot (from rm_rowmin: fresh buffers, rows whose smallest circular index is < min(E, N); all
// ones when combining), read by the window MAP kernel, which skips the parity loads of the other rows (zero).  Word
// 2 SB_ROWMASK_WORDS holds K.  Rows without an LLR of a fresh buffer are left unwritten by the fused equaliser + rate
// dematcher (pdsch_eq_rm) and read as zero by every reader: the MAP kernel, the combining rate dematchers and
// mi355_softbuffer_pool_materialize (raw readers).
#define SB_ROWMASK 18544
#define SB_ROWMASK_WORDS 12

namespace mi355 {

struct TbDesc {
  uint32_t tbs, C, C1, K1, K2, slot0, invalid;
  uint32_t Qm, nof_e_bits, rv;
  uint32_t cb_base[2]; // index of the TB's first K1 / K2 code block in the call's (K-grouped) CB arrays
  uint64_t e_off;      // element offset of the TB's LLRs in the e_bits buffer
  uint64_t data_off;
  const uint32_t* crc_scale; // TB CRC24A over tbs/8 bytes by 256 threads: x^(8 * bytes after thread t's chunk) mod P
};

struct CrcTable {
  uint32_t t[256];
  uint32_t pw[24]; // x^(8*2^i) mod P
  uint32_t poly;   // with the x^24 term
};

constexpr uint16_t RM_NONE = 0xffff; // decoder-buffer position no circular-buffer bit maps to

// Every 16-bit inverse rate-dematching table (decoder position -> circular index, buflen + 1 entries) is followed, at
// u16 offset rm_rowmin_off(buflen), by 2 x 32 SB_ROWMASK_WORDS row minima: [stream P0, P1][row j] = the smallest
// circular index among the row's 16 window positions (RM_NONE when none); rows j >= L = K / 16, and every row of a K
// without the 16-window layout, hold 0 (always defined).
constexpr uint32_t rm_rowmin_off(uint32_t buflen) { return (buflen + 1 + 7) / 8 * 8; }
constexpr uint32_t rm_rowmin_len() { return 2 * 32 * SB_ROWMASK_WORDS; }

} // namespace mi355
