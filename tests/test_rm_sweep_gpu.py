"""GPU: the turbo rate dematchers at every code-block size, redundancy version and class of E (tests/rm_inputs.py)
against the oracle, whose own rate dematcher tests/test_rm_sweep_oracle.py pins to the compiled reference at the same
(K, rv, E).  Bit-exact, no tolerances.

dlsch_rm_rx runs through mi355_dlsch_decode_dev (max_iterations 1 unless stated) and the decoder buffers are read back
from the pool's slots, after mi355_softbuffer_pool_materialize where the test compares whole buffers; dlsch_rm8_rx runs
through mi355_dlsch_decode8_dev; mi355_rm_turbo_rx_8bit_dev is called directly."""
from __future__ import annotations

import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import rm_inputs as RI
import tdec_inputs as TI
from srsran_amd import lib
from srsran_amd.dlsch import Dlsch, SoftbufferPool
from srsran_amd.tdec import DeviceBuffer, Tdec8Batch
from tests.pdsch_jobs import dirty_pool

gpu = pytest.mark.gpu  # (the host-side coverage tests of this file run without one)
HERE = os.path.dirname(os.path.abspath(__file__))
NSB_CLASSES = (0, 8, 16)


def _slots(pool: SoftbufferPool, nslots: int, materialize: bool = True) -> np.ndarray:
    """The first nslots code-block slots of the pool, (nslots, 18600) int16.  materialize: the parity rows a fresh
    write left unwritten are zeroed first (what they stand for); without it the raw memory."""
    L = lib()
    buf, stride, mcb = C.POINTER(C.c_int16)(), C.c_uint32(), C.c_uint32()
    L.mi355_softbuffer_pool_buffer.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_int16)), C.POINTER(C.c_uint32),
                                               C.POINTER(C.c_uint32)]
    assert L.mi355_softbuffer_pool_buffer(pool.h, C.byref(buf), C.byref(stride), C.byref(mcb)) == 0
    assert stride.value == RI.SB_STRIDE and nslots <= pool.nof_sb * mcb.value
    if materialize:
        pool.materialize()
    else:
        L.mi355_device_sync()
    got = np.zeros((nslots, stride.value), np.int16)
    L.mi355_memcpy_d2h(got.ctypes.data, C.cast(buf, C.c_void_p).value, got.nbytes)
    return got


def _pads(sizes, targets):
    """e_pad of Dlsch.decode such that TB i starts at an int16 offset = targets[i] (mod 8); also the offsets"""
    off, pads, offs = 0, [], []
    for n, t in zip(sizes, targets):
        p = (t - off) % 8
        pads.append(p)
        offs.append(off + p)
        off += p + n
    return pads, offs


def _mismatch(got: np.ndarray, want: np.ndarray, K: int):
    """None, or (differing positions, first position) over the code-bit positions of a 16-bit decoder buffer"""
    c = RI.cols(K, TI.nsb(K))
    d = np.nonzero(got[c] != want[c])[0]
    return None if d.size == 0 else (int(d.size), int(c[d[0]]))


# ------------------------------------------------------------------ fresh, every size

@gpu
@pytest.mark.parametrize("rv", RI.RVS)
def test_fresh_every_size_every_E(rv):
    """All 188 sizes as single-block TBs (tbs = K - 24, Qm 2) x the 7 E classes in one decode call of 1,316 TBs per rv,
    LLR classes cycled (full range, +-300, zero, all -32768), e_offset % 8 cycling over 0..7 across the TBs: each
    buffer equals the oracle's rate dematching into a zeroed one.  Host side: every (window-count class, E class)
    met the 16-byte, the 4-byte and the unaligned load path."""
    descs, es, meta = [], [], []
    for K in TI.CB_SIZES:
        for ecls, E in RI.e_classes(K, rv).items():
            i = len(descs)
            descs.append(dict(tbs=K - 24, Qm=2, rv=rv, softbuffer=i))
            es.append(RI.llrs(K, rv, ecls, E, RI.LLR_CLASSES[i % 4]))
            meta.append((K, ecls, E))
    assert len(descs) == 188 * 7
    pads, offs = _pads([e.size for e in es], [i % 8 for i in range(len(es))])
    met = {(TI.nsb(K), ecls, RI.features(K, rv, E, o)["load"]) for (K, ecls, E), o in zip(meta, offs)}
    assert met == {(n, c, k) for n in NSB_CLASSES for c in RI.E_CLASSES for k in ("e16", "e4", "unaligned")}
    dl, pool = Dlsch(0, 1), SoftbufferPool(len(descs), 1)
    dirty_pool(pool, dl)
    rets, _d, its = dl.decode(pool, descs, es, e_pad=pads)
    got = _slots(pool, len(descs))
    dl.close()
    pool.close()
    assert all(r in (0, -1) for r in rets) and all(v == 1.0 for v in its)
    bad = []
    for i, (K, ecls, E) in enumerate(meta):
        m = _mismatch(got[i], oracle.rm_turbo_rx(es[i], K, rv), K)
        if m:
            bad.append((K, ecls, E, offs[i] % 8, RI.LLR_CLASSES[i % 4]) + m)
    assert not bad, (len(bad), bad[:10])


# ------------------------------------------------------------------ HARQ, every size

@functools.lru_cache(maxsize=None)
def _harq(keep_flags: bool):
    """Per transmission: (descs, LLRs, oracle results, oracle buffers after it) of the 188 sizes, and per size the
    number of wrapped sums.  keep_flags False: the CB CRC flags are cleared after every transmission."""
    sbs = [oracle.Softbuffer(1) for _ in TI.CB_SIZES]
    txs, hist = [], [[] for _ in TI.CB_SIZES]
    for tx in range(4):
        descs, es, want = [], [], []
        for i, K in enumerate(TI.CB_SIZES):
            rv = RI.HARQ_ORDERS[i % len(RI.HARQ_ORDERS)][tx]
            ecls = RI.HARQ_E[tx]
            e = RI.llrs(K, rv, ecls, RI.e_classes(K, rv)[ecls], "full", tx)
            descs.append(dict(tbs=K - 24, Qm=2, rv=rv, softbuffer=i))
            es.append(e)
            if not sbs[i].cb_crc[0]:
                hist[i].append((rv, e))
            want.append(oracle.dlsch_decode_tb(e, K - 24, 2, rv, 1, sbs[i]))
            if not keep_flags:
                sbs[i].cb_crc[:] = 0
        txs.append((descs, es, want, np.stack([s.buf[0] for s in sbs])))
    wrapped = [RI.wrapped_sums(K, hist[i]) for i, K in enumerate(TI.CB_SIZES)]
    return txs, wrapped


def test_harq_inputs_cover():
    """On the oracle.  With the CB CRC flags left alone, 24 sizes skip the later transmissions: after one
    half-iteration on the few LLRs of a first sparse-mid transmission at rv 2 the decisions are all zero, whose CRC
    is zero, so the reference marks the block decoded (sch.c:385) -- the skip is part of what is compared.  With the
    flags cleared after every transmission, all four transmissions combine and an int16 sum wraps at every size."""
    _txs, natural = _harq(True)
    assert 10 <= sum(w == 0 for w in natural) <= 40, [K for K, w in zip(TI.CB_SIZES, natural) if w == 0]
    _txs, cleared = _harq(False)
    assert min(cleared) >= 1, [(K, w) for K, w in zip(TI.CB_SIZES, cleared) if w < 1]


def _clear_cb_crc(pool: SoftbufferPool):
    L = lib()
    p = C.c_void_p()
    L.mi355_softbuffer_cb_crc_dev.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
    assert L.mi355_softbuffer_cb_crc_dev(pool.h, 0, C.byref(p)) == 0
    L.mi355_device_sync()
    assert L.mi355_memset_dev(p, 0, pool.nof_sb * pool.max_cb) == 0
    L.mi355_device_sync()


@gpu
@pytest.mark.parametrize("keep_flags", [True, False], ids=["checked_each", "combined_unread"])
def test_harq_every_size(keep_flags):
    """Four transmissions per size into one softbuffer, rv orders of rm_inputs.HARQ_ORDERS round-robin over the sizes,
    E classes (sparse-mid, N / 3, N + 2, sparse-mid), full-range LLRs; return codes and iteration counts are the
    oracle's after every transmission.
    checked_each: the buffers are read back (and so materialized) after every transmission, the CB CRC flags left
    alone (the blocks the reference marks decoded skip the later transmissions).
    combined_unread: the flags are cleared after every transmission and the buffers read only after the last, so
    every size combines four times: the combining writes meet rows a fresh write left unwritten, the bitmap going
    dense, quads without a new LLR (the `any` skip) and wrapping sums (test_harq_inputs_cover)."""
    txs, _wrapped = _harq(keep_flags)
    n = len(TI.CB_SIZES)
    dl, pool = Dlsch(0, 1), SoftbufferPool(n, 1)
    dirty_pool(pool, dl)
    bad = []
    for tx, (descs, es, want, bufs) in enumerate(txs):
        pads, _ = _pads([e.size for e in es], [(3 * i + tx) % 8 for i in range(n)])
        rets, _d, its = dl.decode(pool, descs, es, e_pad=pads)
        assert rets == [w[0] for w in want], tx
        assert its == [w[2] for w in want], tx
        if not keep_flags:
            _clear_cb_crc(pool)
            if tx < 3:
                continue
        got = _slots(pool, n)
        for i, K in enumerate(TI.CB_SIZES):
            m = _mismatch(got[i], bufs[i], K)
            if m:
                bad.append((tx, K, descs[i]["rv"]) + m)
    dl.close()
    pool.close()
    assert not bad, (len(bad), bad[:10])


# ------------------------------------------------------------------ slot reuse

@gpu
def test_slot_reuse_after_reset():
    """One fresh sparse-mid transmission per size, buffers left as written (sparse bitmaps, K words); reset_all; then
    the size list reversed, so slot i held another K: the buffers equal the oracle's from zero -- no stale bitmap
    word, K word or LLR leaks."""
    n = len(TI.CB_SIZES)
    dl, pool = Dlsch(0, 1), SoftbufferPool(n, 1)
    dirty_pool(pool, dl)
    bad = []
    for rnd, sizes in enumerate((TI.CB_SIZES, TI.CB_SIZES[::-1])):
        descs, es = [], []
        for i, K in enumerate(sizes):
            rv = (i + rnd) % 4
            descs.append(dict(tbs=K - 24, Qm=2, rv=rv, softbuffer=i))
            es.append(RI.llrs(K, rv, "sparse_mid", RI.e_classes(K, rv)["sparse_mid"], "pm300", 8 + rnd))
        dl.decode(pool, descs, es)
        if rnd == 0:
            pool.reset_all()
            continue
        got = _slots(pool, n)
        for i, K in enumerate(sizes):
            m = _mismatch(got[i], oracle.rm_turbo_rx(es[i], K, descs[i]["rv"]), K)
            if m:
                bad.append((K, descs[i]["rv"]) + m)
    dl.close()
    pool.close()
    assert not bad, (len(bad), bad[:10])


# ------------------------------------------------------------------ transport blocks of several code blocks

@functools.lru_cache(maxsize=None)
def _multi_cases():
    """[(tbs, Qm, G, what)]: C in {2, 3, 5, 11, 13} of one size with gamma in {0, 1, C // 2, C - 1}; 14 TBs of two
    code-block sizes spread over 6,200 .. 120,000 bits; E ~ N / 3 and E > N of one K in one call, in both orders"""
    cases = []
    for Cn in (2, 3, 5, 11, 13):
        tbs = RI.one_size_tbs(Cn)
        K = oracle.cbsegm(tbs)["K1"]
        for gamma in sorted({0, 1, Cn // 2, Cn - 1}):
            cases.append((tbs, 2, 2 * (Cn * ((K + 4) // 2) + gamma), ("one", Cn, gamma)))
    two = RI.two_size_tbs()
    for j in range(14):
        tbs = two[j * (len(two) - 1) // 13]
        sg = oracle.cbsegm(tbs)
        gamma = (0, 1, sg["C"] - 1, sg["C"] // 2)[j % 4]
        cases.append((tbs, 2, 2 * (sg["C"] * ((sg["K2"] + 4) // 2) + gamma), ("two", sg["C"], gamma)))
    tbs = RI.one_size_tbs(3)
    K = oracle.cbsegm(tbs)["K1"]
    small, large = 2 * 3 * ((K + 4) // 2), 2 * (3 * ((3 * K + 52) // 2) + 1)
    for G in (small, large, large, small):
        cases.append((tbs, 2, G, ("mix", 3, (G // 2) % 3)))
    return cases


def test_multi_block_cases_cover():
    cases = _multi_cases()
    one = {(w[1], w[2]) for *_c, w in cases if w[0] == "one"}
    assert one == {(2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (5, 0), (5, 1), (5, 2), (5, 4), (11, 0), (11, 1), (11, 5),
                   (11, 10), (13, 0), (13, 1), (13, 6), (13, 12)}
    two = [oracle.cbsegm(t) for t, _q, _g, w in cases if w[0] == "two"]
    assert len(two) >= 12 and all(s["C2"] > 0 and s["C1"] > 0 and s["F"] == 0 for s in two)
    assert min(s["C"] for s in two) == 2 and max(s["C"] for s in two) >= 19
    # (both K groups of a two-size TB get code blocks with E and with E + Qm somewhere)
    assert {w[2] > 0 for *_c, w in cases if w[0] == "two"} == {False, True}
    for t, q, g, w in cases:
        assert (g // q) % oracle.cbsegm(t)["C"] == w[2]


@gpu
@pytest.mark.parametrize("shift", RI.RVS)
def test_multi_block_tbs(shift):
    """The cases of _multi_cases in one call, TB i at rv (i + shift) % 4, +-300 LLRs, e_offset % 8 cycling: gamma != 0
    (the reference's `cb > C - gamma`), cb_base[1] and the second K group of two-size TBs, fold2 from the larger E of
    a K group.  Return codes, payload bytes, iteration counts and every code block's buffer are the oracle's."""
    cases = _multi_cases()
    n = len(cases)
    descs = [dict(tbs=t, Qm=q, rv=(i + shift) % 4, softbuffer=i) for i, (t, q, _g, _w) in enumerate(cases)]
    es = [RI.rand_llrs((7 << 40) | (shift << 32) | i, g, "pm300") for i, (_t, _q, g, _w) in enumerate(cases)]
    pads, _ = _pads([e.size for e in es], [(5 * i + shift) % 8 for i in range(n)])
    max_cb = max(oracle.cbsegm(t)["C"] for t, *_r in cases)
    dl, pool = Dlsch(0, 1), SoftbufferPool(n, max_cb)
    dirty_pool(pool, dl)
    rets, datas, its = dl.decode(pool, descs, es, e_pad=pads)
    got = _slots(pool, n * max_cb).reshape(n, max_cb, -1)
    dl.close()
    pool.close()
    bad = []
    for i, (tbs, q, _g, what) in enumerate(cases):
        sb = oracle.Softbuffer(max_cb)
        ret, data, it = oracle.dlsch_decode_tb(es[i], tbs, q, descs[i]["rv"], 1, sb)
        sg = oracle.cbsegm(tbs)
        nb = tbs // 8 + 6
        if rets[i] != ret or its[i] != it or not np.array_equal(datas[i][:nb], data[:nb]):
            bad.append((what, "result", rets[i], ret, its[i], it))
        for c in range(sg["C"]):
            m = _mismatch(got[i, c], sb.buf[c], sg["K1"] if c < sg["C1"] else sg["K2"])
            if m:
                bad.append((what, descs[i]["rv"], c) + m)
    assert not bad, (len(bad), bad[:10])


# ------------------------------------------------------------------ odd Qm

ODD_QM = [  # (tbs, Qm, G): odd E below N, odd E with wrap-around, odd per-block counts and offsets with gamma != 0
    (16, 1, 99), (16, 1, 2 * 132 + 17), (488, 1, 1001), (488, 3, 3 * 333), (1000, 1, 2049), (1000, 3, 3 * 1111),
    (6120, 3, 3 * 3333), (6120, 1, 18443), (6120, 1, 18445), (15840, 3, 3 * (3 * 1771 + 1)),
    (15840, 1, 3 * 5313 + 2), (15840, 3, 3 * (3 * 5317 + 2)), (6200, 1, 2 * 9999 + 1)]


@gpu
def test_odd_qm_matches_oracle():
    """Qm 1 and 3, which the reference's decode_tb accepts: the per-block LLR counts Qm (G' / C) (+ Qm) and offsets are
    odd, so the last LLR of a pass is half an int16 pair.  Two transmissions (rv 0, then 1 combined): return codes,
    iteration counts and buffers are the oracle's."""
    n = len(ODD_QM)
    odd = 0
    for t, q, g in ODD_QM:
        sg = oracle.cbsegm(t)
        odd += (q * (g // q // sg["C"])) % 2
    assert odd >= 10
    max_cb = 3
    dl, pool = Dlsch(0, 1), SoftbufferPool(n, max_cb)
    dirty_pool(pool, dl)
    sbs = [oracle.Softbuffer(max_cb) for _ in ODD_QM]
    bad = []
    for tx, rv in enumerate((0, 1)):
        descs = [dict(tbs=t, Qm=q, rv=rv, softbuffer=i) for i, (t, q, _g) in enumerate(ODD_QM)]
        es = [RI.rand_llrs((9 << 40) | (tx << 32) | i, g, "full") for i, (_t, _q, g) in enumerate(ODD_QM)]
        pads, _ = _pads([e.size for e in es], [(i + 3 * tx) % 8 for i in range(n)])
        rets, _d, its = dl.decode(pool, descs, es, e_pad=pads)
        got = _slots(pool, n * max_cb).reshape(n, max_cb, -1)
        for i, (t, q, g) in enumerate(ODD_QM):
            ret, _data, it = oracle.dlsch_decode_tb(es[i], t, q, rv, 1, sbs[i])
            sg = oracle.cbsegm(t)
            if rets[i] != ret or its[i] != it:
                bad.append((t, q, g, tx, "result", rets[i], ret, its[i], it))
            for c in range(sg["C"]):
                m = _mismatch(got[i, c], sbs[i].buf[c], sg["K1"] if c < sg["C1"] else sg["K2"])
                if m:
                    bad.append((t, q, g, tx, c) + m)
    dl.close()
    pool.close()
    assert not bad, (len(bad), bad[:10])


# ------------------------------------------------------------------ sparse buffers: the switch, and decoding through them

SPARSE_SIZES = tuple(K for K in TI.CB_SIZES if TI.nsb(K) == 16)
SPARSE_ITS = 4
SPARSE_SNR = 20.0


def _stale_rows(pool: SoftbufferPool, dl: Dlsch) -> int:
    """K = 6144, rv 0: a dense transmission of all -32768 (E = N), a reset, then a fresh sparse-mid transmission of
    zeros; the number of -32768 left in the slot's raw memory (the rows the second write left unwritten)"""
    K = 6144
    d = [dict(tbs=K - 24, Qm=2, rv=0, softbuffer=0)]
    dl.decode(pool, d, [RI.rand_llrs(0, RI.N_of(K), "min")])
    pool.reset(0)
    dl.decode(pool, d, [RI.rand_llrs(0, RI.e_classes(K, 0)["sparse_mid"], "zero")])
    raw = _slots(pool, 1, materialize=False)[0]
    return int((raw[RI.cols(K, 16)] == -32768).sum())


@gpu
def test_sparse_rows_left_unwritten_and_materialized():
    """MI355_RM_SPARSE (default on) and SB_ROWMASK at work: a fresh write leaves exactly the parity rows without an LLR
    unwritten (16 stale entries per such row), and mi355_softbuffer_pool_materialize zeroes them."""
    assert os.environ.get("MI355_RM_SPARSE", "1") != "0"
    dl, pool = Dlsch(0, 1), SoftbufferPool(1, 1)
    P0, P1 = RI.empty_rows(6144, 0, RI.e_classes(6144, 0)["sparse_mid"])
    assert P0 > 0 and P1 > 0
    assert _stale_rows(pool, dl) == 16 * (P0 + P1)
    got = _slots(pool, 1)[0]
    assert not got[RI.cols(6144, 16)].any()
    dl.close()
    pool.close()


@functools.lru_cache(maxsize=None)
def _sparse_decode_cases():
    """Per rv one call: the 110 16-window sizes x (sparse-mid, N / 3), real codewords at 20 dB, and the oracle's decode"""
    calls = []
    for rv in RI.RVS:
        rng = np.random.default_rng([110, rv])
        descs, es, want = [], [], []
        for K in SPARSE_SIZES:
            for ecls in ("sparse_mid", "third"):
                E = RI.e_classes(K, rv)[ecls]
                e = oracle.make_tb(rng, K - 24, 2, E, rv, SPARSE_SNR)[1]
                descs.append(dict(tbs=K - 24, Qm=2, rv=rv, softbuffer=len(descs)))
                es.append(e)
                want.append(oracle.dlsch_decode_tb(e, K - 24, 2, rv, SPARSE_ITS, oracle.Softbuffer(1)))
        calls.append((descs, es, want))
    return calls


def _sparse_decode(latency: int):
    """[(rets, datas, its)] of the calls of _sparse_decode_cases on one turbo path"""
    old = lib().mi355_dlsch_set_latency_path(latency)
    out = []
    try:
        dl, pool = Dlsch(0, SPARSE_ITS), SoftbufferPool(2 * len(SPARSE_SIZES), 1)
        dirty_pool(pool, dl)
        for descs, es, _want in _sparse_decode_cases():
            pool.reset_all()
            counters = (C.c_uint64 * 11)()
            assert lib().mi355_dlsch_latency_profile(1, None) == 0
            try:
                out.append(dl.decode(pool, descs, es))
            finally:
                assert lib().mi355_dlsch_latency_profile(0, C.addressof(counters)) == 0
            assert counters[10] == (len(descs) if latency else 0), (latency, counters[10])  # blocks tdec_win_lat decoded
        dl.close()
        pool.close()
    finally:
        lib().mi355_dlsch_set_latency_path(old)
    return out


def _sparse_check(results, what):
    bad = []
    for (descs, _es, want), (rets, datas, its) in zip(_sparse_decode_cases(), results):
        for i, d in enumerate(descs):
            ret, data, it = want[i]
            nb = d["tbs"] // 8 + 3
            if rets[i] != ret or its[i] != it or not np.array_equal(np.asarray(datas[i])[:nb], data[:nb]):
                bad.append((what, d["tbs"] + 24, d["rv"], i % 2, int(rets[i]), ret, float(its[i]), it))
    assert not bad, (len(bad), bad[:10])


def test_sparse_decode_cases_cover():
    """On the oracle: TBs that pass and TBs that fail, first checks and late ones, and rows without an LLR in every TB
    at sparse-mid."""
    rets, its = [], []
    for descs, es, want in _sparse_decode_cases():
        assert len(descs) == 220
        for d, e in zip(descs[::2], es[::2]):
            assert RI.features(d["tbs"] + 24, d["rv"], e.size, 0)["rows_mixed"]
        rets += [w[0] for w in want]
        its += [w[2] for w in want]
    assert rets.count(0) >= 50 and rets.count(-1) >= 400, (rets.count(0), rets.count(-1))
    assert {1.0, float(SPARSE_ITS)} <= set(its)


@gpu
@pytest.mark.parametrize("latency", [512, 0], ids=["latency", "throughput"])
def test_decode_through_sparse_buffers(latency):
    """The MAP kernels of both turbo paths read buffers whose empty parity rows were never written (the bitmap says
    zero): return codes, payload bytes and iteration counts are the oracle's, for the TBs that fail too."""
    _sparse_check(_sparse_decode(latency), latency)


def _child_main(out: str):
    """In a process of its own (the switch is read once): the same decodes on both paths and the stale-row count"""
    dl, pool = Dlsch(0, 1), SoftbufferPool(1, 1)
    res = {"stale": np.int64(_stale_rows(pool, dl))}
    dl.close()
    pool.close()
    for latency in (512, 0):
        for c, (rets, datas, its) in enumerate(_sparse_decode(latency)):
            res[f"r{latency}_{c}"] = np.array(rets, np.int32)
            res[f"i{latency}_{c}"] = np.array(its, np.float64)
            res[f"d{latency}_{c}"] = np.concatenate([np.asarray(d, np.uint8) for d in datas])
    np.savez(out, **res)


@gpu
def test_decode_with_dense_writes_in_child(tmp_path):
    """MI355_RM_SPARSE=0 in a fresh child process: fresh buffers are written whole (no stale entry survives), and the
    decodes of test_decode_through_sparse_buffers give the same results."""
    out = str(tmp_path / "dense.npz")
    env = {**os.environ, "MI355_RM_SPARSE": "0"}
    r = subprocess.run([sys.executable, os.path.join(HERE, "rm_child.py"), out], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    z = np.load(out)
    assert int(z["stale"]) == 0
    for latency in (512, 0):
        results = []
        for c, (descs, _es, _w) in enumerate(_sparse_decode_cases()):
            cut = np.cumsum([0] + [d["tbs"] // 8 + 6 for d in descs])
            flat = z[f"d{latency}_{c}"]
            results.append((z[f"r{latency}_{c}"].tolist(), [flat[cut[i]: cut[i + 1]] for i in range(len(descs))],
                            z[f"i{latency}_{c}"].tolist()))
        _sparse_check(results, ("dense", latency))


# ------------------------------------------------------------------ the 8-bit forms

@gpu
@pytest.mark.parametrize("rv", RI.RVS)
def test_rm_turbo_rx_8bit_every_size(rv):
    """mi355_rm_turbo_rx_8bit_dev at all 188 sizes x this rv x {N / 3, N, 2N + 18}, full-range int8 LLRs, into a zeroed
    buffer and then a second accumulation at (rv + 2) % 4, against rm_inputs.rm_rx8 (pinned to the reference's
    srslte_rm_turbo_rx_lut_8bit by tests/test_rm_sweep_oracle.py); whole buffers, the gaps of the layout included."""
    dec = Tdec8Batch()
    bmax = RI.buflen(6144, 32)
    emax = 2 * RI.N_of(6144) + 18
    d_out, d_e = DeviceBuffer(bmax), DeviceBuffer(emax)
    zeros = np.zeros(bmax, np.int8)
    bad = []
    layouts = set()
    for K in TI.CB_SIZES:
        bl = RI.buflen(K, RI.nsb8_layout(K))
        layouts.add(RI.nsb8_layout(K))
        ec = RI.e_classes(K, rv)
        for ecls in RI.E_CLASSES8:
            E = ec[ecls]
            want = np.zeros(bl, np.int8)
            d_out.upload(zeros)
            for tx, r in enumerate((rv, (rv + 2) % 4)):
                e = RI.llrs8(K, rv, ecls, E, tx)
                d_e.upload(e)
                assert dec.rm_rx_dev(d_e.ptr, E, E, d_out.ptr, bl, 1, K, r) == 0
                RI.rm_rx8(e, K, r, want)
                got = d_out.download(np.zeros(bmax, np.int8))
                if not np.array_equal(got[:bl], want) or got[bl:].any():
                    bad.append((K, rv, ecls, E, tx))
                    break
    dec.close()
    assert layouts == {0, 8, 16, 32}
    assert not bad, (len(bad), bad[:10])


SIZES_DLSCH8 = tuple(K for K in TI.CB_SIZES if K <= 400 or TI.nsb8(K) >= 16)  # dlsch_plan.h: dlsch_k_ok8


@gpu
def test_dlsch8_every_size():
    """mi355_dlsch_decode8_dev (dlsch_rm8_rx) at every size it accepts -- K <= 400 and the 16- / 32-window sizes --
    fresh and one combine ((rv + 2) % 4), E classes cycled over {N / 3, N, 2N + 18}, full-range int8 LLRs at every
    e_offset % 8: the code-bit positions of the int8 buffer at the start of the slot, and for K <= 400 the converted
    int16 copy at SB_CONV8."""
    n = len(SIZES_DLSCH8)
    assert n == 46 + 110 and {RI.nsb8_layout(K) for K in SIZES_DLSCH8} == {0, 16, 32}
    dl, pool = Dlsch(0, 1), SoftbufferPool(n, 1)
    want = [np.zeros(RI.buflen(K, RI.nsb8_layout(K)), np.int8) for K in SIZES_DLSCH8]
    bad = []
    for tx in range(2):
        descs, es = [], []
        for i, K in enumerate(SIZES_DLSCH8):
            rv = (i + 2 * tx) % 4
            ecls = RI.E_CLASSES8[(i + tx) % 3]
            e = RI.llrs8(K, i % 4, ecls, RI.e_classes(K, rv)[ecls], 4 + tx)
            descs.append(dict(tbs=K - 24, Qm=2, rv=rv, softbuffer=i))
            es.append(e)
            RI.rm_rx8(e, K, rv, want[i])
        pads, _ = _pads([e.size for e in es], [(i + tx) % 8 for i in range(n)])
        rets, _d, _its = dl.decode(pool, descs, es, llr8=True, e_pad=pads)
        assert all(r in (0, -1) for r in rets), (tx, rets)
        _clear_cb_crc(pool)  # (a block whose decisions happen to pass the CRC would skip the combine)
        raw = _slots(pool, n, materialize=False)
        for i, K in enumerate(SIZES_DLSCH8):
            bl = want[i].size
            c = RI.cols(K, RI.nsb8_layout(K))  # (the 8-bit decoder copies the tails into the pads of the streams)
            if not np.array_equal(raw[i].view(np.int8)[:bl][c], want[i][c]):
                bad.append((K, tx, descs[i]["rv"], "int8"))
            if K <= 400 and not np.array_equal(raw[i][RI.SB_CONV8: RI.SB_CONV8 + bl], want[i].astype(np.int16)):
                bad.append((K, tx, descs[i]["rv"], "int16 copy"))
    dl.close()
    pool.close()
    assert not bad, (len(bad), bad[:10])
