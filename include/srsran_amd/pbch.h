/*
 * include/srsran_amd/pbch.h -- C ABI of the MI355X PBCH receiver: MIB acquisition for batches of radio frames,
 * plus the host-side MIB packing and a PBCH encoder for synthesising test frames.
 *
 *   mi355_pbch_decode_batch   srslte_pbch_decode (phch/pbch.c:444-557), the decoder under srslte_ue_mib_decode
 *                             (ue/ue_mib.c:133-174): srslte_pbch_get (pbch.c:50-134, prb_dl.c:46-77) of the grid
 *                             and of every port's estimate, srslte_predecoding_single / _diversity +
 *                             srslte_layerdemap_diversity per port hypothesis, the float QPSK demapper, then for
 *                             every combination of 1..4 consecutive radio frames and every 40 ms phase
 *                             decode_frame (pbch.c:399-434): descrambling, srslte_rm_conv_rx (rm_conv.c:94-154),
 *                             the 1 / (2 n) scale, srslte_viterbi_decode_f (viterbi.c:548-571 +
 *                             viterbi37_avx2_16bit.c) and the masked CRC16 check (pbch.c:364-397).  Every
 *                             combination is decoded on the device; the reference's sequential search
 *                             (pbch.c:501-548), its reset on success and its history slide (pbch.c:551-554) are
 *                             replayed on the host over the results.
 *   mi355_pbch_mib_*          srslte_pbch_mib_unpack / srslte_pbch_mib_pack (pbch.c:271-357).
 *   mi355_pbch_encode_host    srslte_pbch_encode (pbch.c:561-611) into host tx grids.
 *
 * Scope: normal CP (240 REs, 480 bits per radio frame).  As in the reference only receive antenna 0 is read.
 * Numerics: ret, nof_tx_ports, sfn_offset and the payload are the reference's for the same grid / channel
 * estimates; LLRs agree with the reference's AVX2 build within float rounding.
 */
#ifndef SRSRAN_AMD_PBCH_H
#define SRSRAN_AMD_PBCH_H

#include <stddef.h>
#include <stdint.h>

#include "pdcch.h"
#include "ue_dl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI355_BCH_PAYLOAD_LEN 24     /* SRSLTE_BCH_PAYLOAD_LEN (pbch.h:48) */
#define MI355_BCH_PAYLOADCRC_LEN 40  /* SRSLTE_BCH_PAYLOADCRC_LEN */
#define MI355_PBCH_NOF_RE 240        /* PBCH_RE_CP_NORM (pbch.c:39) */

typedef struct mi355_pbch mi355_pbch_t;

/* ---------------------------------------------------------------- host functions (no GPU) */

/* srslte_pbch_mib_unpack (pbch.c:271-312): msg is MI355_BCH_PAYLOAD_LEN unpacked bits; sets cell->nof_prb,
 * phich_length, phich_resources and, when sfn is given, the SFN (multiple of 4). */
void mi355_pbch_mib_unpack(const uint8_t* msg, mi355_cell_t* cell, uint32_t* sfn);
/* srslte_pbch_mib_pack (pbch.c:321-357): payload receives MI355_BCH_PAYLOAD_LEN unpacked bits */
void mi355_pbch_mib_pack(const mi355_cell_t* cell, uint32_t sfn, uint8_t* payload);
/* srslte_pbch_encode (pbch.c:561-611): CRC16 with the port mask, tail-biting convolutional code, rate matching to
 * 1920 bits, the 480 bits of frame_idx % 4 scrambled and QPSK-modulated, transmit diversity for more than one
 * port, srslte_pbch_put into slot 1 of sf_symbols[port] (host complex float, 14 x 12 nof_prb) for every port. */
int mi355_pbch_encode_host(const mi355_cell_t* cell, const uint8_t* bch_payload, float* const* sf_symbols,
                           uint32_t frame_idx);

/* ---------------------------------------------------------------- GPU batches */

/* srslte_pbch_init + srslte_pbch_set_cell (pbch.c:140-268).  cell->nof_ports == 0: 1, 2 and 4 ports are searched
 * (search_all_ports; the caller's estimates then cover 4 ports), otherwise only that port count is tried. */
int  mi355_pbch_create(mi355_pbch_t** q, const mi355_cell_t* cell, int device);
void mi355_pbch_destroy(mi355_pbch_t* q);
/* srslte_pbch_decode_reset (pbch.c:359-362): forget the frames received so far */
void mi355_pbch_decode_reset(mi355_pbch_t* q);

/* what srslte_pbch_decode returns through its arguments */
typedef struct {
  int32_t  ret;          /* 1 MIB decoded, 0 not (srslte_pbch_decode's return value) */
  uint32_t nof_tx_ports; /* 1, 2 or 4 */
  int32_t  sfn_offset;
  uint8_t  bch_payload[MI355_BCH_PAYLOAD_LEN]; /* unpacked bits */
} mi355_pbch_res_t;

/* MI355_PBCH_INDEPENDENT: every job is decoded as the first call after a reset (frame_idx 1), e.g. many captures
 *   of one cell id; the object's history is neither read nor written.
 * MI355_PBCH_SEQUENCE: the jobs are successive radio frames of one cell.  res[i] is what srslte_pbch_decode
 *   returns on its (k + i)-th call on one object after k earlier calls; the history persists across batch calls and
 *   is cleared by mi355_pbch_decode_reset, so a batch of n equals n batches of 1. */
enum { MI355_PBCH_INDEPENDENT = 0, MI355_PBCH_SEQUENCE = 1 };

/* sfjobs[i]: the subframe-0 grid and channel estimates of one radio frame in HBM, as
 * mi355_ue_dl_decode_fft_estimate_batch leaves them (sf_symbols[0], ce[p][0]); chest[i].noise_estimate their noise.
 * Synchronous: res[njobs] is filled on return. */
int mi355_pbch_decode_batch(mi355_pbch_t* q, const mi355_dl_sf_job_t* sfjobs, const mi355_chest_dl_res_t* chest,
                            uint32_t njobs, uint32_t mode, mi355_pbch_res_t* res, void* stream);

/* Inspection of the previous decode call on q (parity tests): the 480 LLRs of job i under the port hypothesis nant
 * (one the object tries), before descrambling -- what srslte_pbch_decode writes to its history slot for that
 * hypothesis.  Returns the count (480). */
int mi355_pbch_llr(mi355_pbch_t* q, uint32_t i, uint32_t nant, float* llr480);

#ifdef __cplusplus
}
#endif
#endif
