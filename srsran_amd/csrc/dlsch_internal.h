// srsran_amd/csrc/dlsch_internal.h -- device argument blocks of the DL-SCH kernels (dlsch_kernels.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dlsch_layout.h" // slot layout, TbDesc, CrcTable, RM_NONE (host-only part)

namespace mi355 {

struct CbDesc {      // one code block of one transport block
  uint32_t tb, cb, C; // transport block index in the call, CB index, CBs in the TB
  uint32_t rlen;      // K - 24 (C > 1) or K
  uint32_t rp, n_e;   // offset / count of its LLRs in the TB's e_bits (sch.c:391-401)
  // two 16-bit fields in the word rv had, so that the descriptor stays 48 bytes: rv <= 3 (the planner rejects others)
  // and nb <= K / 8 <= 768 both fit
  uint16_t rv;
  uint16_t nb;        // payload bytes it leaves at cb * rlen / 8: up to where the next CB starts (the last: K / 8)
  uint32_t slot;      // softbuffer code-block slot in the pool
  uint64_t e_off;     // element offset of the TB's LLRs in the e_bits buffer
  uint64_t data_off;  // byte offset of the TB payload in the data buffer
};

static_assert(sizeof(CbDesc) == 48, "CbDesc is read by every check kernel: keep it at three 16-byte words");

struct DlschRmArgs {
  const CbDesc*   desc;
  int             ncb;
  uint32_t        N;      // 3K+12 circular-buffer bits
  uint32_t        buflen; // decoder buffer length 3(K+32)+12 (or 3K+12 linear)
  const uint16_t* inv[4]; // [rv][decoder position] -> circular-buffer index or RM_NONE
  const int16_t*  e;
  int16_t*        sb;
  size_t          sb_stride;
  const uint8_t*  sb_crc;
  uint8_t*        fresh;  // per slot: buffer logically zero (lazy srslte_softbuffer_rx_reset)
  uint32_t        fold2;  // LDS pairs: >= max over the launch's code blocks of min(n_e, N) / 2 (0: N / 2)
  int             sparse; // fresh buffers: parity rows without an LLR are left unwritten (SB_ROWMASK)
};

// 8-bit rate dematching (srslte_rm_turbo_rx_lut_8bit into (int8_t*)softbuffer->buffer_f[cb], sch.c:403-407):
// thread per (code block, decoder position); the int8 buffer occupies the first bytes of the CB's slot
struct DlschRm8Args {
  const CbDesc*   desc;
  int             ncb;
  uint32_t        N, buflen;
  const uint16_t* inv[4];
  const int8_t*   e;
  int8_t*         sb;        // pool buffer as bytes
  size_t          sb_stride; // bytes per slot
  const uint8_t*  sb_crc;
  const uint8_t*  fresh;
  int16_t*        conv;      // K <= 400: the int16 copy the reference's 16-bit fallback decodes (nullable)
};

struct DlschCheckArgs {
  const CbDesc*  desc;
  int            ncb;
  uint32_t       K, h, max_its;
  const uint8_t* dec;
  size_t         dec_stride;
  uint8_t*       data;
  uint8_t*       done;
  const uint32_t* remaining; // running flag of this half-iteration (0: every code block finished)
  uint32_t*      next;      // running flag of the next half-iteration
  uint32_t*      its;
  uint8_t*        sb_crc;
  const CrcTable* crc24a;
  const CrcTable* crc24b;
  const uint32_t* scale; // [CRC24A | CRC24B][64 lanes]: x^(8 * bytes after the lane's chunk) mod P for K/8 bytes
};

struct DlschTbArgs {
  const TbDesc* tb;
  int           ntb;
  uint8_t*      data;
  uint8_t*      sb_crc;
  uint8_t*      sb_data;
  int32_t*        ret;
  const CrcTable* crc24a;
  // code-block arrays of the call, expanded by the prologue from the TB descriptors
  CbDesc*   desc;
  uint32_t* slot;
  uint32_t* its;
  uint8_t*  done;
  uint32_t* running; // running flag of half-iteration 0
  float*    avg;     // per TB: mean half-iterations over its code blocks (epilogue)
};

struct DlschResetArgs {
  uint8_t* fresh;
  uint8_t* sb_crc;
  size_t   slot0, ncb; // fresh flags of code blocks [slot0, slot0 + ncb) set
  size_t   ncrc;       // CB-CRC flags of [slot0, slot0 + ncrc) cleared (0: ncb)
};

hipError_t dlsch_launch_rm(const DlschRmArgs& a, hipStream_t s);
// srslte_softbuffer_rx_reset_tbs for a list of softbuffers: list[i] = {softbuffer, code blocks to reset}
hipError_t dlsch_launch_reset_list(const uint2* list, uint32_t n, uint32_t max_cb, uint8_t* fresh, uint8_t* cb_crc,
                                   hipStream_t s);
hipError_t dlsch_launch_check(const DlschCheckArgs& a, hipStream_t s);
hipError_t dlsch_launch_prologue(const DlschTbArgs& a, hipStream_t s);
hipError_t dlsch_launch_epilogue(const DlschTbArgs& a, hipStream_t s);
hipError_t dlsch_launch_reset(const DlschResetArgs& a, hipStream_t s);

hipError_t dlsch_launch_rm8(const DlschRm8Args& a, hipStream_t s);
hipError_t dlsch_launch_materialize(int16_t* sb, size_t stride, const uint8_t* fresh, size_t slot0, uint32_t nslots,
                                    hipStream_t s);

} // namespace mi355
