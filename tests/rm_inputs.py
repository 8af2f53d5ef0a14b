"""TEST INFRASTRUCTURE ONLY: inputs for the turbo rate dematchers at every one of the 188 code-block sizes, every
redundancy version and every class of E, shared by tests/test_rm_sweep_oracle.py (the oracle's rate dematcher and the
int8 restatement below against the compiled reference's) and tests/test_rm_sweep_gpu.py (dlsch_rm_rx, dlsch_rm8_rx and
mi355_rm_turbo_rx_8bit_dev against the oracle).

Everything is integer and bit-exact.  LLRs come from tdec_inputs.mix64 (a splitmix64 sequence written out there, no
numpy.random), seeded from (K, rv, E class, transmission, LLR class)."""
from __future__ import annotations

import functools

import numpy as np

import oracle
import tdec_inputs as TI

CB_SIZES = TI.CB_SIZES
RVS = (0, 1, 2, 3)
E_CLASSES = ("sparse_mid", "third", "N-2", "N", "N+2", "2N+18", "4N+6")
E_CLASSES8 = ("third", "N", "2N+18")
LLR_CLASSES = ("full", "pm300", "zero", "min")
RM_THREADS = 512        # dlsch_kernels.hip:25
SB_ROWMASK_WORDS = 12   # dlsch_internal.h:18
SB_STRIDE = TI.SB_STRIDE
SB_CONV8 = 10240        # dlsch_internal.h:8
# HARQ: the order of the redundancy versions of the four transmissions, round-robin over the sizes, and their E classes
HARQ_ORDERS = ((0, 2, 3, 1), (2, 0, 1, 3), (3, 1, 0, 2), (1, 3, 2, 0), (0, 0, 2, 2), (2, 3, 2, 3))
HARQ_E = ("sparse_mid", "third", "N+2", "sparse_mid")


def N_of(K: int) -> int:
    return 3 * K + 12


def nd(K: int) -> int:
    """Dummy bits in front of each sub-block interleaver input (36.212 5.1.4.1.1): 32 ceil((K + 4) / 32) - (K + 4)"""
    return 32 * -(-(K + 4) // 32) - (K + 4)


def buflen(K: int, n: int) -> int:
    """Decoder buffer length: the sub-block layout (rm_tables.h:6-7) or the linear one"""
    return 3 * (K + 32) + 12 if n else 3 * K + 12


def cols(K: int, n: int) -> np.ndarray:
    """The positions of a decoder buffer that hold code bits (systematic, parity 0, parity 1, tails)"""
    if not n:
        return np.r_[0:3 * K + 12]
    return np.r_[0:K, K + 32:2 * K + 32, 2 * K + 64:3 * K + 64, 3 * K + 96:3 * K + 108]


@functools.lru_cache(maxsize=None)
def table(K: int, rv: int) -> np.ndarray:
    """oracle.rm_turbo_table: circular-buffer index -> position in the 16-bit decoder buffer"""
    t = oracle.rm_turbo_table(K, rv)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def rowmin(K: int, rv: int):
    """16-window sizes: (2, L) smallest circular index among the 16 positions of each parity row (dlsch_layout.h
    rm_rowmin_off, dlsch_tables.h rm16_table); None for the other sizes"""
    if TI.nsb(K) != 16:
        return None
    inv = np.full(buflen(K, 16), 0xffff, np.int64)
    inv[table(K, rv)] = np.arange(N_of(K))
    L = K // 16
    rm = np.stack([inv[s * (K + 32): s * (K + 32) + K].reshape(L, 16).min(axis=1) for s in (1, 2)])
    assert rm.max() < N_of(K)
    return rm


def sparse_interval(K: int, rv: int):
    """[lo, hi]: the E <= N for which a fresh buffer has a parity row that holds an LLR (some row minimum < E) and a
    row that holds none (some row minimum >= E); None without the 16-window layout"""
    rm = rowmin(K, rv)
    if rm is None:
        return None
    return int(rm.min()) + 1, int(rm.max())


def e_classes(K: int, rv: int) -> dict:
    """E of each class of E_CLASSES (all even: Qm = 2)"""
    N = N_of(K)
    iv = sparse_interval(K, rv)
    mid = 2 * ((iv[0] + iv[1] + 2) // 4) if iv else 2 * ((2 * N + 5) // 10)  # nearest even to (lo + hi) / 2 | 0.4 N
    return {"sparse_mid": mid, "third": 2 * ((N + 3) // 6), "N-2": N - 2, "N": N, "N+2": N + 2, "2N+18": 2 * N + 18,
            "4N+6": 4 * N + 6}


def empty_rows(K: int, rv: int, E: int):
    """(P0, P1) parity rows a fresh write of E LLRs leaves without an LLR (rm_image.h:25-28: minimum >= min(E, N))"""
    rm = rowmin(K, rv)
    if rm is None:
        return 0, 0
    thr = min(E, N_of(K))
    return int((rm[0] >= thr).sum()), int((rm[1] >= thr).sum())


def rand_llrs(seed: int, n: int, cls: str) -> np.ndarray:
    """n int16 LLRs of one class: full-range (HARQ sums wrap), +-300, all zero, all -32768"""
    if cls == "zero":
        return np.zeros(n, np.int16)
    if cls == "min":
        return np.full(n, -32768, np.int16)
    w = TI.mix64(seed, n)
    if cls == "full":
        return (w >> np.uint64(48)).astype(np.uint16).view(np.int16)
    assert cls == "pm300"
    return ((w >> np.uint64(32)) % np.uint64(601)).astype(np.int64).astype(np.int16) - np.int16(300)


def llrs(K: int, rv: int, ecls: str, E: int, cls: str, tx: int = 0) -> np.ndarray:
    """The E LLRs of (K, rv, E class, transmission) of one class"""
    seed = (K << 20) | (rv << 16) | (E_CLASSES.index(ecls) << 12) | (tx << 8) | LLR_CLASSES.index(cls)
    return rand_llrs(seed, E, cls)


def llrs8(K: int, rv: int, ecls: str, E: int, tx: int = 0) -> np.ndarray:
    """E full-range int8 LLRs"""
    seed = (1 << 40) | (K << 20) | (rv << 16) | (E_CLASSES.index(ecls) << 12) | (tx << 8)
    return (TI.mix64(seed, E) >> np.uint64(56)).astype(np.uint8).view(np.int8)


def features(K: int, rv: int, E: int, e_offset: int, Qm: int = 2, fresh: bool = True) -> dict:
    """Every choice the 16-bit rate dematchers make for one single-block TB of E LLRs at int16 offset e_offset of a
    256-byte aligned buffer"""
    N, n = N_of(K), TI.nsb(K)
    P0, P1 = empty_rows(K, rv, E) if fresh else (0, 0)
    return {"nsb": n,
            # dlsch_kernels.hip:86, 98-102: one 16-byte load per lane, 4-byte pair loads, or two int16 loads per pair
            "load": "e16" if e_offset % 8 == 0 and min(E, N) % 2 == 0 else "e4" if e_offset % 2 == 0 else "unaligned",
            "fresh": fresh,                                   # dlsch_kernels.hip:107: written whole instead of read
            "wraps": -(-E // N) - 1,                          # dlsch_kernels.hip:131: accumulating passes, E > N
            "fold2": (min(E + Qm, N) + 1) // 2,               # dlsch_plan.h plan_tbs: LDS pairs of the TB
            "tail_quads": (buflen(K, n) // 2) % 4,            # dlsch_kernels.hip:156: pairs of the last, partial store
            "passes": -(-(buflen(K, n) // 2) // (4 * RM_THREADS)),  # dlsch_kernels.hip:141: quads per thread in use
            "empty_rows": (P0, P1),                           # rm_image.h rm_rowmask_word (fresh 16-window buffers)
            "sparse": n == 16 and 0 < P0 + P1,                # dlsch_kernels.hip:142: rows left unwritten
            "rows_mixed": n == 16 and 0 < P0 + P1 < 2 * (K // 16),
            # pdsch_plan.h eqrm_job_shape: pdsch_eq_rm (and its compact tables, dlsch_tables.h) only without wrap
            "eqrm_ok": E + Qm <= N}


# ------------------------------------------------------------------ int8 restatement (srslte_rm_turbo_rx_lut_8bit)

@functools.lru_cache(maxsize=None)
def table8(K: int, rv: int) -> np.ndarray:
    """The 16-bit table re-mapped to the 8-bit decoder layout (rm_tables.h:33-37: 32 windows for K % 32 == 0 and
    K > 2048, otherwise the 16-bit layout's window count)"""
    t = table(K, rv).astype(np.int64)
    n, n8 = TI.nsb(K), TI.nsb8(K) or TI.nsb(K)
    if n8 == n:
        return t
    assert n == 16 and n8 == 32
    s, pos = t // (K + 32), t % (K + 32)
    m = (pos % n) * (K // n) + pos // n                     # bit m of stream s (rm_tables.h:76 inverted)
    L8 = K // n8
    out = np.where(s < 3, s * (K + 32) + (m % L8) * n8 + m // L8, t)
    out.setflags(write=False)
    return out


def nsb8_layout(K: int) -> int:
    """Windows of the 8-bit buffer layout: 0 / 8 / 16 / 32"""
    return TI.nsb8(K) or TI.nsb(K)


def rm_rx8(e: np.ndarray, K: int, rv: int, out: np.ndarray) -> np.ndarray:
    """out[table8[i % N]] += e[i] in wrapping int8, in place"""
    t = table8(K, rv)
    N = N_of(K)
    add = np.bincount(t[np.arange(e.size) % N], e.astype(np.float64), out.size)  # (exact: small integers)
    out[:] = ((out.astype(np.int64) + add.astype(np.int64)) & 0xff).astype(np.uint8).view(np.int8)
    return out


def wrapped_sums(K: int, txs) -> int:
    """Positions of a buffer combined from transmissions [(rv, e)] whose exact sum leaves int16"""
    acc = np.zeros(SB_STRIDE, np.int64)
    N = N_of(K)
    for rv, e in txs:
        acc += np.bincount(table(K, rv)[np.arange(e.size) % N], e.astype(np.float64), SB_STRIDE).astype(np.int64)
    return int(((acc > 32767) | (acc < -32768)).sum())


# ------------------------------------------------------------------ transport blocks of several code blocks

@functools.lru_cache(maxsize=None)
def one_size_tbs(C: int) -> int:
    """The smallest TB size with C code blocks of one size and no filler bits"""
    t = 8 * ((6120 * (C - 1)) // 8)
    while True:
        sg = oracle.cbsegm(t)
        if sg["C"] == C and sg["C2"] == 0 and sg["F"] == 0:
            return t
        assert sg["C"] <= C, (C, t)
        t += 8


@functools.lru_cache(maxsize=None)
def two_size_tbs() -> tuple:
    """Every TB size of 6,200 .. 120,000 bits (multiples of 8) with two code-block sizes and no filler bits"""
    out = []
    for t in range(6200, 120001, 8):
        sg = oracle.cbsegm(t)
        if sg["C2"] > 0 and sg["F"] == 0:
            out.append(t)
    return tuple(out)
