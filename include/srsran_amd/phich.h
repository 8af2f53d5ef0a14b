/*
 * include/srsran_amd/phich.h -- C ABI of what the UE hears about its uplink on the MI355X: PHICH decoding (the HARQ
 * indicator for a PUSCH sent 4 TTIs earlier) for batches of subframes, the UL grants (DCI format 0) the control-stage
 * blind search comes across, and the host-side PHICH resource calculation, format-0 packing and a PHICH encoder for
 * synthesising test subframes.
 *
 *   mi355_ue_dl_decode_phich_batch  srslte_ue_dl_decode_phich (ue/ue_dl.c:757-790): srslte_phich_calc
 *                                   (phch/phich.c:133-144), then srslte_phich_decode (phich.c:183-315):
 *                                   srslte_regs_phich_get (regs.c:466-481) of the grid and of every port's estimate,
 *                                   srslte_predecoding_single_multi / _diversity_multi + srslte_layerdemap_diversity,
 *                                   the +-1 scrambling sequence (sequences.c:45-48), despreading with w_normal
 *                                   (phich.c:40-47, 296-301), the BPSK demapper (demod_soft.c:125-130) and
 *                                   srslte_phich_ack_decode (phich.c:149-173).
 *   mi355_ue_dl_find_ul_dci_batch   srslte_ue_dl_find_ul_dci (ue_dl.c:613-641): the format-0 messages the blind search
 *                                   of the previous control-stage call set aside (ue_dl.c:420-434, 521-532), unpacked
 *                                   by srslte_dci_msg_unpack_pusch.
 *   mi355_phich_ngroups / _calc     srslte_regs_phich_ngroups (regs.c:404-407), srslte_phich_calc.
 *   mi355_phich_encode_host         srslte_phich_encode (phich.c:320-437) into host tx grids.
 *   mi355_dci_msg_{un,}pack_pusch   srslte_dci_msg_pack_pusch / _unpack_pusch (phch/dci.c:1337-1390) over
 *                                   dci_format0_pack / _unpack (dci.c:416-574), FDD.
 *
 * Scope: FDD, normal CP (four-chip sequences, eight per group), PHICH mi = 1, normal subframes.
 * Numerics: ack_value and distance are the reference's for the same grid / channel estimates, bit for bit (the
 * equalisers are those of the PCFICH; every later operation is evaluated in the reference's order).
 */
#ifndef SRSRAN_AMD_PHICH_H
#define SRSRAN_AMD_PHICH_H

#include <stddef.h>
#include <stdint.h>

#include "pdcch.h"
#include "ue_dl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MI355_PHICH_NBITS 3          /* SRSLTE_PHICH_NBITS (phich.h:45) */
#define MI355_PHICH_NORM_NSEQUENCES 8 /* SRSLTE_PHICH_NORM_NSEQUENCES */
#define MI355_PHICH_NORM_NSF 4       /* SRSLTE_PHICH_NORM_NSF */
#define MI355_PHICH_MAX_NSYMB 12     /* SRSLTE_PHICH_MAX_NSYMB: the REs of one group */

/* srslte_phich_grant_t, srslte_phich_resource_t, srslte_phich_res_t (phich.h:82-96) */
typedef struct {
  uint32_t n_prb_lowest; /* lowest PRB of the PUSCH the indicator answers */
  uint32_t n_dmrs;       /* cyclic shift field of its UL grant */
  uint32_t I_phich;      /* 0 in FDD */
} mi355_phich_grant_t;

typedef struct {
  uint32_t ngroup;
  uint32_t nseq;
} mi355_phich_resource_t;

typedef struct {
  int32_t  ret;       /* MI355_SUCCESS, or MI355_ERROR_INVALID_INPUTS (the job never reached the device) */
  uint32_t ack_value; /* 1 ACK, 0 NACK */
  float    distance;  /* the winning correlation (srslte_phich_ack_decode's max_corr) */
} mi355_phich_res_t;

/* srslte_dci_ul_t (phch/dci.h:132-180), field by field (bool -> uint32_t as in mi355_dci_dl_t) */
enum { MI355_RA_PUSCH_HOP_DISABLED = -1, MI355_RA_PUSCH_HOP_QUART = 0, MI355_RA_PUSCH_HOP_QUART_NEG = 1,
       MI355_RA_PUSCH_HOP_HALF = 2, MI355_RA_PUSCH_HOP_TYPE2 = 3 };
typedef struct {
  uint16_t             rnti;
  uint32_t             format;
  mi355_dci_location_t location;
  uint32_t             ue_cc_idx;
  struct {
    uint32_t riv;
    uint32_t n_prb1a;
    uint32_t n_gap;
    uint32_t mode;
  } type2_alloc;
  int32_t        freq_hop_fl; /* MI355_RA_PUSCH_HOP_* */
  mi355_dci_tb_t tb;
  uint32_t       n_dmrs;
  uint32_t       cqi_request;
  uint32_t       dai;
  uint32_t       ul_idx;
  uint32_t       is_tdd;
  uint8_t        tpc_pusch;
  uint32_t       cif;
  uint32_t       cif_present;
  uint8_t        multiple_csi_request;
  uint32_t       multiple_csi_request_present;
  uint32_t       srs_request;
  uint32_t       srs_request_present;
  uint32_t       ra_type;
  uint32_t       ra_type_present;
} mi355_dci_ul_t;

/* ---------------------------------------------------------------- host functions (no GPU) */

/* srslte_phich_ngroups: PHICH groups of the cell (mi = 1), ceil(Ng * nof_prb / 8); the REG map's group count */
uint32_t mi355_phich_ngroups(const mi355_cell_t* cell);
/* srslte_phich_calc (phich.c:133-144, 36.213 9.1.2): MI355_ERROR when the cell has no group */
int mi355_phich_calc(const mi355_cell_t* cell, const mi355_phich_grant_t* grant, mi355_phich_resource_t* n_phich);
/* srslte_phich_encode (phich.c:320-437): the ACK bit three times, BPSK, spread with w_normal[nseq], scrambled, transmit
 * diversity for more than one port (the reference's plain precoding for 4 ports too, without the 36.211 6.9.2 port
 * alternation) and *added* to the group's 12 REs of sf_symbols[port] (host complex float, 14 x 12 nof_prb), so the
 * PHICHs of one group superpose.  MI355_ERROR_INVALID_INPUTS for nseq >= 8 or ngroup >= mi355_phich_ngroups. */
int mi355_phich_encode_host(const mi355_cell_t* cell, const mi355_dl_sf_cfg_t* sf, mi355_phich_resource_t n_phich,
                            uint8_t ack, float* const* sf_symbols);
/* srslte_dci_msg_unpack_pusch / srslte_dci_msg_pack_pusch (dci.c:1337-1390) for format 0, as the reference writes
 * them: the CIF is packed when dci->cif_present and read when cfg->cif_enabled; the hopping field takes 1 bit below
 * 50 PRB and 2 from 50 PRB out of the RIV's; with the 2-bit CSI request the packer writes {cqi_request, 0} and the
 * unpacker reads both bits into multiple_csi_request; the ra_type bit is read (cfg->ra_format_enabled) but never
 * packed, so it is the first padding bit.  Unpacking a payload whose flag bit says 1A returns MI355_ERROR. */
int mi355_dci_msg_unpack_pusch(const mi355_cell_t* cell, const mi355_dl_sf_cfg_t* sf, const mi355_dci_cfg_t* cfg,
                               mi355_dci_msg_t* msg, mi355_dci_ul_t* dci);
int mi355_dci_msg_pack_pusch(const mi355_cell_t* cell, const mi355_dl_sf_cfg_t* sf, const mi355_dci_cfg_t* cfg,
                             const mi355_dci_ul_t* dci, mi355_dci_msg_t* msg);

/* ---------------------------------------------------------------- GPU batches */

typedef struct {
  uint32_t            sf; /* index into sfjobs / sfs / chest; several jobs may name one subframe */
  mi355_phich_grant_t grant;
} mi355_phich_job_t;

/* srslte_ue_dl_decode_phich for njobs (subframe, grant) pairs over nsf subframes whose grids / channel estimates are
 * in HBM as mi355_ue_dl_decode_fft_estimate_batch leaves them; chest[sf].noise_estimate their noise (read by the
 * 1-port equaliser only), sfs[sf].tti % 10 the scrambling.  Synchronous: res[njobs] is filled on return.
 * A job whose group is out of range (ngroup >= mi355_phich_ngroups: FDD with I_phich = 1) or with sf >= nsf gets
 * ret = MI355_ERROR_INVALID_INPUTS, never reaches the device and leaves the other jobs' results as they are without
 * it.  njobs = 0 succeeds without a launch.
 * When no correlation exceeds srslte_phich_ack_decode's -9999 start value (a NaN soft bit: 1 port, zero estimates and
 * zero noise) the reference leaves distance unwritten; here ack_value = 0 and distance = 0 then. */
int mi355_ue_dl_decode_phich_batch(mi355_ue_dl_t* q, const mi355_dl_sf_job_t* sfjobs, const mi355_dl_sf_cfg_t* sfs,
                                   const mi355_chest_dl_res_t* chest, uint32_t nsf, const mi355_phich_job_t* jobs,
                                   uint32_t njobs, mi355_phich_res_t* res, void* stream);

/* srslte_ue_dl_find_ul_dci for the njobs subframes of the previous control-stage call on q
 * (mi355_ue_dl_find_dl_dci_batch, mi355_ue_dl_fft_estimate_find_dci_batch or mi355_ue_dl_find_and_decode_batch):
 * dci_ul[i * MI355_MAX_DCI_MSG + k] for k < nof_ul[i] are the format-0 messages its blind search kept for job i, in
 * search order (one grant seen at two aggregation levels or in both spaces is kept once), unpacked with cfgs[i].dci;
 * nof_ul[i] = -1 when unpacking fails.  The call empties the lists: a second call returns 0 everywhere.  rntis[i] = 0
 * returns 0.  njobs beyond the previous call's are MI355_ERROR_INVALID_INPUTS.
 * Deviation: the reference's pending list lives on the object and survives a TTI whose caller skips find_ul_dci; here
 * every control-stage call starts each job's list empty, which is what a caller that drains it every TTI sees. */
int mi355_ue_dl_find_ul_dci_batch(mi355_ue_dl_t* q, const mi355_dl_sf_cfg_t* sfs, const mi355_ue_dl_cfg_t* cfgs,
                                  const uint16_t* rntis, uint32_t njobs, int32_t* nof_ul, mi355_dci_ul_t* dci_ul);

#ifdef __cplusplus
}
#endif
#endif
