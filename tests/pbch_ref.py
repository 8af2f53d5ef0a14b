"""TEST INFRASTRUCTURE ONLY: a restatement of srslte_pbch_decode (lib/src/phy/phch/pbch.c:444-557) as a stateful
class and of srslte_pbch_encode (pbch.c:561-611), built from stages that already exist:

  liboracle.so             orc_ctrl_equalize, orc_rm_conv_rx / _tx, orc_conv_encode_tb, orc_viterbi_quant,
                           orc_viterbi37_tb_decode_us, orc_crc16_bits
  oracle/_ref (if built)   ref_rm_conv_rx, ref_viterbi_decode_f, ref_crc16 -- the reference's own code for those stages
                           (PbchRef(use_ref=True))

Extraction (srslte_pbch_cp over prb_cp_ref), the Gold sequence, the float QPSK demapper, the hypothesis loops and
the history buffer are written here from pbch.c."""
from __future__ import annotations

import numpy as np

import oracle
from oracle import pdcch_chain as pd

NRE, NBITS = 240, 480
RX_NULL = np.float32(10000.0)
# srslte_crc_mask (pbch.c:42-45) by port count
CRC_MASK = {1: np.zeros(16, np.uint8), 2: np.ones(16, np.uint8), 4: np.tile(np.array([0, 1], np.uint8), 8)}


def pbch_re(nof_prb: int, cell_id: int) -> np.ndarray:
    """Grid indices of the 240 PBCH REs in srslte_pbch_get order, following the pointer arithmetic of srslte_pbch_cp
    (pbch.c:54-102) and prb_cp_ref(offset = id % 3, nof_refs = 4, nof_intervals = 24) (prb_dl.c:46-77)."""
    nre = 12 * nof_prb
    ptr = 7 * nre + nof_prb * 6 - 36  # slot 1, then input += nof_prb * SRSLTE_NRE / 2 - 36
    out = []
    off = cell_id % 3
    for _ in range(2):  # symbols 0 and 1: prb_cp_ref
        out += list(range(ptr, ptr + off))
        ptr += off
        for _i in range(24 - 1):
            ptr += 1
            out += [ptr, ptr + 1]
            ptr += 2
        if 2 - off > 0:
            ptr += 1
            out += list(range(ptr, ptr + 2 - off))
            ptr += 2 - off
        ptr += nre - 2 * 36 + (1 if off == 2 else 0)
    for _ in range(2):  # symbols 2 and 3: prb_cp of 6 PRB
        out += list(range(ptr, ptr + 72))
        ptr += 72
        ptr += nre - 2 * 36
    re = np.array(out, np.int64)
    assert re.size == NRE
    return re


def crc16(bits: np.ndarray, use_ref: bool = False) -> int:
    b = np.ascontiguousarray(bits, np.uint8)
    return int(pd._ref().ref_crc16(b, b.size) if use_ref else pd._lib().orc_crc16_bits(b, b.size))


class PbchRef:
    """srslte_pbch_t: nof_ports == 0 searches 1, 2 and 4 ports on 4-port estimates (search_all_ports)."""

    def __init__(self, nof_prb: int, cell_id: int, nof_ports: int = 0, use_ref: bool = False):
        self.nof_prb, self.cell_id, self.use_ref = nof_prb, cell_id, use_ref
        self.hyps = [1, 2, 4] if nof_ports == 0 else [nof_ports]
        self.nof_ports = 4 if nof_ports == 0 else nof_ports
        self.re = pbch_re(nof_prb, cell_id)
        c = oracle.sequence_lte(cell_id, 4 * NBITS)          # srslte_sequence_pbch
        self.c_float = np.where(c != 0, -1.0, 1.0).astype(np.float32)
        self.llr = np.zeros(4 * NBITS, np.float32)
        self.frame_idx = 0
        self.last_llr = {}    # nant -> the 480 LLRs of the last call under that hypothesis (inspection)
        self.last_hit = None  # (nant, nb, dst, src) of the last success

    def reset(self):
        self.frame_idx = 0

    def equalize(self, grid, ce, nant, noise):
        y = np.ascontiguousarray(grid[self.re], np.complex64)
        h = np.ascontiguousarray(ce[:nant][:, self.re], np.complex64)
        d = np.zeros(NRE, np.complex64)
        pd._lib().orc_ctrl_equalize(y.view(np.float32), h.view(np.float32).ravel(), 1, nant, NRE,
                                    float(noise) if nant == 1 else 0.0, d.view(np.float32))
        # srslte_demod_soft_demodulate(QPSK), float
        return (d.view(np.float32) * np.float32(-np.sqrt(2))).astype(np.float32)

    def decode_bits(self, src, dst, n):
        """decode_frame (pbch.c:399-423) up to the Viterbi decoder: the 40 decided bits."""
        temp = np.full(4 * NBITS, RX_NULL, np.float32)
        temp[dst * NBITS:(dst + n) * NBITS] = (self.llr[src * NBITS:(src + n) * NBITS] *
                                               self.c_float[dst * NBITS:(dst + n) * NBITS])
        rm = np.zeros(120, np.float32)
        if self.use_ref:
            pd._ref().ref_rm_conv_rx(temp, 4 * NBITS, rm, 120)
        else:
            pd._lib().orc_rm_conv_rx(temp, 4 * NBITS, rm, 120)
        rm = (rm * np.float32(1.0 / float(np.float32(2) * np.float32(n)))).astype(np.float32)
        bits = np.zeros(40, np.uint8)
        if self.use_ref:
            pd._ref().ref_viterbi_decode_f(rm, 40, bits)
        else:
            q = np.zeros(120, np.uint16)
            pd._lib().orc_viterbi_quant(rm, 120, q)
            pd._lib().orc_viterbi37_tb_decode_us(q, 40, bits)
        return bits

    def crc_check(self, bits, nant):
        """srslte_pbch_crc_check (pbch.c:378-397): True when the masked CRC passes and the payload is not zero."""
        data = bits.copy()
        data[24:] ^= CRC_MASK[nant]
        return crc16(data, self.use_ref) == 0 and int(data[:24].sum()) != 0

    def decode(self, grid, ce, noise):
        """One srslte_pbch_decode call.  grid: (G,) rx antenna 0; ce: (ports, G) or (ports, rx, G).
        Returns (ret, nof_tx_ports, sfn_offset, payload bits or None)."""
        ce = np.asarray(ce)
        if ce.ndim == 3:
            ce = ce[:, 0]
        assert ce.shape[0] >= self.nof_ports
        self.frame_idx += 1
        f = self.frame_idx
        self.last_llr, self.last_hit = {}, None
        for nant in self.hyps:
            l = self.equalize(grid, ce, nant, noise)
            self.last_llr[nant] = l.copy()
            self.llr[NBITS * (f - 1):NBITS * f] = l
            for nb in range(f):
                for dst in range(4 - nb):
                    for src in range(f - nb):
                        bits = self.decode_bits(src, dst, nb + 1)
                        if self.crc_check(bits, nant):
                            self.last_hit = (nant, nb, dst, src)
                            self.reset()
                            return 1, nant, dst - src + f - 1, bits[:24].copy()
        if self.frame_idx == 4:
            self.llr[:3 * NBITS] = self.llr[NBITS:].copy()
            self.frame_idx = 3
        return 0, 0, 0, None


def pbch_encode(nof_prb: int, cell_id: int, nof_ports: int, payload, grids: np.ndarray, frame_idx: int) -> None:
    """srslte_pbch_encode into grids (ports, 14 * 12 * nof_prb) complex64, in place."""
    L = pd._lib()
    data = np.zeros(40, np.uint8)
    data[:24] = np.asarray(payload, np.uint8)
    crc = crc16(data[:24])
    data[24:] = np.array([(crc >> (15 - i)) & 1 for i in range(16)], np.uint8) ^ CRC_MASK[nof_ports]
    coded = np.zeros(120, np.uint8)
    L.orc_conv_encode_tb(data, 40, coded)
    rm = np.zeros(4 * NBITS, np.uint8)
    L.orc_rm_conv_tx(coded, 120, rm, 4 * NBITS)
    fi = frame_idx % 4
    c = oracle.sequence_lte(cell_id, 4 * NBITS)
    b = rm[fi * NBITS:(fi + 1) * NBITS] ^ c[fi * NBITS:(fi + 1) * NBITS]
    y = pd._precode_diversity(pd._qpsk(b), nof_ports)
    re = pbch_re(nof_prb, cell_id)
    for p in range(nof_ports):
        grids[p][re] = y[p]


# a fixed flat channel: one complex gain per transmit port
FLAT_H = np.array([0.9 + 0.3j, -0.5 + 0.7j, 0.6 - 0.6j, -0.8 - 0.2j], np.complex64)


def synth_frame(nof_prb: int, cell_id: int, nof_ports: int, est_ports: int, payload, frame_idx: int, sigma: float,
                rng: np.random.Generator, signal: bool = True):
    """Subframe 0 of one radio frame as a receiver sees it: the product's host PBCH encoder and CRS generator, the
    flat channel FLAT_H, AWGN of standard deviation sigma per real dimension, and the oracle's channel estimator for
    est_ports ports.  signal=False: CRS only (no PBCH).  Returns (grid (G,), ce (est_ports, G), noise estimate)."""
    from oracle import ue_dl_chain as uc
    from srsran_amd import enb_dl as E
    from srsran_amd import pbch as B
    from srsran_amd import pdsch as P
    G = 14 * 12 * nof_prb
    cell = P.make_cell(nof_prb, nof_ports, cell_id)
    tx = np.zeros((nof_ports, G), np.complex64)
    E.put_refs(cell, 0, tx)
    if signal:
        B.pbch_encode_host(cell, payload, tx, frame_idx)
    rx = (FLAT_H[:nof_ports, None] * tx).sum(axis=0)
    rx = (rx + sigma * (rng.standard_normal(G) + 1j * rng.standard_normal(G))).astype(np.complex64)
    ce, res = uc.chest_estimate(rx[None, :], nof_prb, est_ports, cell_id, 0)
    return rx, np.ascontiguousarray(ce[:, 0]), float(res["noise_estimate"])


def bits_of(s: str) -> np.ndarray:
    return np.array([int(ch) for ch in s], np.uint8)
