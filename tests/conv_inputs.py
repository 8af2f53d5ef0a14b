"""TEST INFRASTRUCTURE ONLY: inputs for the tail-biting convolutional decoder at every block length the API admits
(payloads of 1..128 bits + CRC16, F = 17..144), shared by tests/test_conv_decode_gpu.py (the GPU wave of
srsran_amd/csrc/conv_decode.h against the oracle) and tests/test_conv_decode_oracle.py (the oracle against the
reference's own rm_conv.c / viterbi.c / crc.c).

A block is nbits random payload bits with a valid CRC16, encoded (orc_conv_encode_tb) and rate-matched to E
(orc_rm_conv_tx); bit b is sent as an LLR of sign 2b - 1.  Every (nbits, E) comes in the input classes of CLASSES."""
from __future__ import annotations

import functools

import numpy as np

from oracle import pdcch_chain as P

RX_NULL = np.float32(10000.0)   # SRSLTE_RX_NULL (rm_conv.c): a received value equal to it reads as "nothing received"
BELOW_03 = np.nextafter(np.float32(0.3), np.float32(0))
# the gate classes: every |LLR| is one float32 value, so the gate's double sum is exact in any order of summation
GATE = {"gate_0.25": np.float32(0.25), "gate_0.3f": np.float32(0.3), "gate_below_0.3f": BELOW_03}
CLASSES = ("clean", "noisy", "noise", "sat", "zeros", "tiny", "huge", "ties", "halfsteps") + tuple(GATE)
SWEEP_E = (72, 144, 288, 576)   # the PDCCH's aggregation levels
PBCH_E = 1920
SEED = 1


def crc16_bits(bits) -> np.ndarray:
    b = np.ascontiguousarray(bits, np.uint8)
    c = int(P._lib().orc_crc16_bits(b, b.size))
    return np.array([(c >> (15 - i)) & 1 for i in range(16)], np.uint8)


def block(nbits: int, E: int, seed: int = SEED):
    """(the F = nbits + 16 block bits, the E transmitted signs as float32 +-1)"""
    rng = np.random.default_rng([seed, nbits, E])
    d = np.concatenate([rng.integers(0, 2, nbits, dtype=np.uint8), np.zeros(16, np.uint8)])
    d[nbits:] = crc16_bits(d[:nbits])
    F = nbits + 16
    coded = np.zeros(3 * F, np.uint8)
    P._lib().orc_conv_encode_tb(d, F, coded)
    e = np.zeros(E, np.uint8)
    P._lib().orc_rm_conv_tx(coded, 3 * F, e, E)
    return d, (2.0 * e - 1.0).astype(np.float32)


def inputs(nbits: int, E: int, seed: int = SEED):
    """(block bits, {class: E float32 LLRs})"""
    d, s = block(nbits, E, seed)
    rng = np.random.default_rng([seed, nbits, E, 7])
    g = rng.standard_normal(E).astype(np.float32)
    clean = s + np.float32(0.3) * g
    noisy = s + g
    out = {"clean": clean, "noisy": noisy, "noise": rng.standard_normal(E).astype(np.float32)}
    # saturation: a fifth of the entries at +-10000.0 exactly (+10000.0 collides with RX_NULL), another fifth at
    # +-9999.0, each with the sign the noisy entry had
    sat = noisy.copy()
    pick = rng.permutation(E)
    a, b = pick[: E // 5], pick[E // 5: 2 * (E // 5)]
    sat[a] = np.copysign(RX_NULL, noisy[a])
    sat[b] = np.copysign(np.float32(9999.0), noisy[b])
    out["sat"] = sat
    out["zeros"] = np.zeros(E, np.float32)                    # the quantiser's 1e-9 floor on max |x|
    out["tiny"] = clean * np.float32(1e-12)                   # below that floor
    out["huge"] = clean * np.float32(1e30)
    out["ties"] = s.copy()                                    # equal path metrics
    out["halfsteps"] = (np.round(noisy * 2) / 2).astype(np.float32)  # many exact ties after the quantisation
    for name, v in GATE.items():
        out[name] = s * v
    assert set(out) == set(CLASSES) and all(v.dtype == np.float32 and v.size == E for v in out.values())
    for v in out.values():
        v.setflags(write=False)  # shared between tests
    return d, out


def features(nbits: int, E: int) -> dict:
    """The length-dependent paths of decode_cand (conv_decode.h) a case takes, from F and E alone."""
    F = nbits + 16
    return {"nrows": (F - 1) // 32 + 1,                       # rows of the sub-block interleaver (32 - F % 32 dummies)
            "te": (3 * F - 1) % 30 + 1,                       # steps of the last 30-step decision block
            "pe": (3 * F) % 6,                                # state-layout phase after the last step
            "tb_span": (3 * F + 5) // 30 - (F + 6) // 30,     # tb1 - tb0: decision blocks the traceback walks, less one
            "zero_block": (3 * F + 5) // 30 > (3 * F - 1) // 30,  # the traceback starts in a block past the last step
            "punctured": E < 3 * F,
            "second_word": nbits >= 64,                       # parity taken from the second ballot word
            "serial_crc": F > 128}


# every value each feature can take for nbits 1..128
FEATURE_VALUES = {"nrows": {1, 2, 3, 4, 5}, "te": set(range(3, 31, 3)), "pe": {0, 3}, "tb_span": set(range(1, 11)),
                  "zero_block": {False, True}, "punctured": {False, True}, "second_word": {False, True},
                  "serial_crc": {False, True}}


def oracle_decode(llr, nbits: int, scale=None, use_ref: bool = False):
    """Rate dematching, the optional float32 scale (pbch.c:420), quantisation + tail-biting Viterbi, CRC16 remainder:
    (the F decided bits, received parity ^ CRC16(payload)).  use_ref: the reference's own functions (oracle/_ref)."""
    F = nbits + 16
    x = np.array(llr, np.float32)  # (a copy: the reference's prototypes take non-const pointers)
    rm = np.zeros(3 * F, np.float32)
    bits = np.zeros(F, np.uint8)
    if use_ref:
        P._ref().ref_rm_conv_rx(x, x.size, rm, 3 * F)
    else:
        P._lib().orc_rm_conv_rx(x, x.size, rm, 3 * F)
    if scale is not None:
        rm = (rm * np.float32(scale)).astype(np.float32)
    if use_ref:
        assert P._ref().ref_viterbi_decode_f(rm, F, bits) == 0
        crc = int(P._ref().ref_crc16(bits[:nbits].copy(), nbits))
    else:
        q = np.zeros(3 * F, np.uint16)
        P._lib().orc_viterbi_quant(rm, 3 * F, q)
        P._lib().orc_viterbi37_tb_decode_us(q, F, bits)
        crc = int(P._lib().orc_crc16_bits(bits[:nbits].copy(), nbits))
    par = int("".join(str(int(b)) for b in bits[nbits:]), 2)
    return bits, par ^ crc


@functools.lru_cache(maxsize=None)
def sweep(Es=SWEEP_E):
    """Every nbits 1..128 x E x class: a list of (nbits, E, class, LLRs, block bits)"""
    out = []
    for nbits in range(1, 129):
        for E in Es:
            d, cls = inputs(nbits, E)
            out += [(nbits, E, c, cls[c], d) for c in CLASSES]
    return out


PBCH_WINDOWS = [(n, dst) for n in (1, 2, 3, 4) for dst in range(5 - n)]   # decode_frame's (frames, 40 ms phase)
PBCH_SCALES = (0.5, 0.25, float(np.float32(1.0 / 6.0)), 0.125)            # 1 / (2 n) as a float (pbch.c:420)
SCALED_NBITS = (1, 47, 48, 64, 112, 113, 128)


@functools.lru_cache(maxsize=None)
def scaled_jobs():
    """The scaled form (the PBCH's): a list of (nbits, label, scale, 1920 LLRs, block bits).
    F = 40: every decode_frame window -- n consecutive 480-entry frames at phase dst, RX_NULL elsewhere -- under every
    scale and class; then other lengths on the whole vector at scale 0.25."""
    out = []
    d, cls = inputs(24, PBCH_E)
    for (n, dst) in PBCH_WINDOWS:
        for c in CLASSES:
            v = np.full(PBCH_E, RX_NULL, np.float32)
            v[480 * dst: 480 * (dst + n)] = cls[c][480 * dst: 480 * (dst + n)]
            v.setflags(write=False)
            out += [(24, f"{c}/n{n}/dst{dst}", s, v, d) for s in PBCH_SCALES]
    for nbits in SCALED_NBITS:
        d, cls = inputs(nbits, PBCH_E)
        out += [(nbits, c, 0.25, cls[c], d) for c in CLASSES]
    return out

