"""GPU parity of the batched DL-SCH decoder (rate dematching + turbo with CRC early stop + TB CRC)
against the oracle's restatement of decode_tb (sch.c:363-570), whose rate matcher, decoder and CRC are
pinned to the compiled reference by tests/golden/.  Bit-exact: return codes, payload bytes (including the
trailing CB-CRC bytes), average iteration counts, HARQ softbuffer evolution."""
import functools

import numpy as np
import pytest

import oracle
import tdec_inputs as TI
from srsran_amd import check, lib
from srsran_amd.dlsch import Dlsch, SoftbufferPool

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[512, 0], ids=["latency", "throughput"], autouse=True)
def dlsch_path(request):
    """Every test on both turbo paths: the latency path (tdec_win_lat: a wave per code block, all half-iterations in
    one launch, for calls of at most 512 code blocks) and the half-iteration-per-launch throughput path."""
    from srsran_amd import lib
    old = lib().mi355_dlsch_set_latency_path(request.param)
    yield
    lib().mi355_dlsch_set_latency_path(old)

# (tbs, Qm, G, snr_db): SISO QPSK MCS9 (C=3, K=5312), TM4 QAM256 MCS27 codeword (C=16, K=6144), a C=5 TB, one TB
# with gamma != 0 (75376: C=13, G' % C = 9; every other case has C = 1 or G' % C = 0, so gamma = 0 -- 6120 / 14402 only
# leaves G % Qm = 2 LLRs unused; gamma over C and two-size TBs are swept in test_rm_sweep_gpu.py), 16-window and
# 8-window and generic single-CB sizes
CASES = [(15840, 2, 30000, 3.0), (97896, 8, 115200, 9.0), (97896, 8, 115200, 5.5), (30576, 6, 36300, 4.5),
         (1000, 2, 3010, 1.0), (456, 2, 1500, 0.5), (40, 2, 200, -1.0), (6120, 4, 14402, 2.0),
         (75376, 6, 86400, 5.0), (2600, 2, 7800, 0.0),
         # E several times the circular buffer (rate-dematching wrap-around sums): the SIB sizes of the real signal
         (144, 2, 1080, 0.0), (256, 2, 1080, -2.0), (40, 2, 600, -3.0)]


def _oracle(llrs, cases, rvs, max_its, sbs):
    out = []
    for i, (tbs, Qm, G, _) in enumerate(cases):
        out.append(oracle.dlsch_decode_tb(llrs[i], tbs, Qm, rvs[i], max_its, sbs[i]))
    return out


def _check(got, want, cases):
    rets, datas, its = got
    for i, (tbs, *_r) in enumerate(cases):
        r, d, a = want[i]
        C = oracle.cbsegm(tbs)["C"]
        n = tbs // 8 + (6 if C > 1 else 3)
        assert rets[i] == r, (i, tbs)
        np.testing.assert_array_equal(datas[i][:n], d[:n], err_msg=f"tb {i} tbs={tbs}")
        assert abs(its[i] - a) < 1e-5, (i, its[i], a)


@pytest.mark.parametrize("max_its", [1, 4, 10])
def test_dlsch_batch_matches_oracle(max_its):
    rng = np.random.default_rng(100 + max_its)
    llrs = [oracle.make_tb(rng, t, q, g, 0, snr)[1] for (t, q, g, snr) in CASES]
    dl = Dlsch(0, max_its)
    pool = SoftbufferPool(len(CASES), 32)
    got = dl.decode(pool, [dict(tbs=t, Qm=q, rv=0, softbuffer=i) for i, (t, q, g, s) in enumerate(CASES)], llrs)
    want = _oracle(llrs, CASES, [0] * len(CASES), max_its, [oracle.Softbuffer() for _ in CASES])
    _check(got, want, CASES)
    assert any(r == 0 for r in got[0]) and any(r == -1 for r in got[0])


def test_dlsch_harq_retransmission_matches_oracle():
    rng = np.random.default_rng(7)
    cases = [(97896, 8, 115200, 4.0), (15840, 2, 30000, 0.0), (30576, 6, 36300, 2.5)]
    dl = Dlsch(0, 8)
    pool = SoftbufferPool(len(cases), 32)
    sbs = [oracle.Softbuffer() for _ in cases]
    payload_llr = []
    for t, q, g, snr in cases:
        bits = rng.integers(0, 2, t, dtype=np.uint8)
        payload_llr.append(bits)
    for rv in (0, 2, 3, 1):
        llrs = []
        for (t, q, g, snr), bits in zip(cases, payload_llr):
            coded = oracle.dlsch_encode_tb(bits, t, q, g, rv)
            y = np.where(coded.astype(bool), 1.0, -1.0) + 10 ** (-snr / 20) * rng.standard_normal(g)
            llrs.append(np.trunc(100 * y).clip(-32768, 32767).astype(np.int16))
        got = dl.decode(pool, [dict(tbs=t, Qm=q, rv=rv, softbuffer=i) for i, (t, q, g, s) in enumerate(cases)],
                        llrs)
        want = _oracle(llrs, cases, [rv] * len(cases), 8, sbs)
        _check(got, want, cases)


def test_dlsch_invalid_and_empty():
    dl = Dlsch(0, 4)
    pool = SoftbufferPool(2, 4)
    e = np.zeros(1000, np.int16)
    # tbs 97896 needs 16 CBs > max_cb 4 -> invalid; tbs 0 -> success with nothing decoded
    rets, _, _ = dl.decode(pool, [dict(tbs=97896, Qm=8, rv=0, softbuffer=0), dict(tbs=0, Qm=2, rv=0, softbuffer=1)],
                           [e, e])
    assert rets == [-2, 0]


@pytest.mark.parametrize("max_its", [2, 3, 6])
def test_dlsch_speculative_dec2_matches_oracle(max_its):
    """Speculative DEC2 half-iterations (dlsch_runtime.cpp spec_policy): the a-priori of the next DEC1 is written only
    by a rerun for the code blocks the check leaves unfinished, and the policy follows the previous batch.  Batches of
    the mixed cases alternate with all-high-SNR ones on one decoder, so the rerun runs with many, few and no blocks
    and the policy changes between calls; every batch must still be the oracle's."""
    dl = Dlsch(0, max_its)
    pool = SoftbufferPool(len(CASES), 32)
    hi = [(t, q, g, 30.0) for (t, q, g, _s) in CASES]
    for k, cases in enumerate((CASES, hi, hi, CASES, hi)):
        rng = np.random.default_rng(1000 * max_its + k)
        llrs = [oracle.make_tb(rng, t, q, g, 0, snr)[1] for (t, q, g, snr) in cases]
        pool.reset_all()
        got = dl.decode(pool, [dict(tbs=t, Qm=q, rv=0, softbuffer=i) for i, (t, q, g, s) in enumerate(cases)], llrs)
        want = _oracle(llrs, cases, [0] * len(cases), max_its, [oracle.Softbuffer() for _ in cases])
        _check(got, want, cases)


def test_dlsch_many_distinct_tb_sizes_one_call():
    """the TB epilogue's per-size CRC factor tables (dlsch_tables.h tb_crc_scales_table) must stay valid for
    every TB planned in a call.  530 distinct TB sizes (more than the old 512-entry cap) in one batch, then the first
    100 again in a second call; every TB passes its CRC with the transmitted payload.  Sizes: no filler bits and one
    code-block size per TB (the reference's TX orders mixed K+/K- blocks K- first and its RX K+ first, sch.c:255-265 vs
    :387, so mixed-size TBs do not decode in the reference either), 40 .. 275,608 bits, 1 to 46 code blocks."""
    sizes = []
    t = 40
    while len(sizes) < 530:
        sg = oracle.cbsegm(t)
        if sg["F"] == 0 and sg["C2"] == 0:
            sizes.append(t)
        t += 8
    rng = np.random.default_rng(512)
    dl = Dlsch(0, 6)
    pool = SoftbufferPool(len(sizes), 46)
    for call, sz in enumerate((sizes, sizes[:100])):
        pays, llrs = [], []
        for t in sz:
            p, e = oracle.make_tb(rng, t, 2, 3 * t + 120, 0, 20.0)
            pays.append(p)
            llrs.append(e)
        pool.reset_all()
        rets, datas, _its = dl.decode(pool, [dict(tbs=t, Qm=2, rv=0, softbuffer=i) for i, t in enumerate(sz)], llrs)
        assert rets == [0] * len(sz), (call, [i for i, r in enumerate(rets) if r != 0][:8])
        for i, t in enumerate(sz):
            np.testing.assert_array_equal(datas[i][: t // 8], pays[i][: t // 8], err_msg=f"call {call} tbs {t}")


@pytest.mark.parametrize("kind", ["reset", "reset_range", "reset_tbs_batch"])
def test_null_stream_reset_done_before_decode(kind):
    """dlsch.h: a softbuffer reset given stream NULL has completed when the call returns.  The null stream does not
    order against the decoder's own (non-blocking) stream, so a reset left pending there could land after the next
    decode's rate dematcher read the CB CRC flags: that decode would skip every code block as already passed and
    return the previous TB (profiles/r05/reset_race).  Each round: a clean TB decodes into softbuffer 0 (its flags
    set), the raw C reset with NULL (no device sync around it), then pure-noise LLRs decode into the same softbuffer
    at once; the result must be the oracle's decode of the noise from a fresh softbuffer (CRC failure)."""
    import ctypes as C
    L = lib()
    L.mi355_softbuffer_reset_range.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L.mi355_softbuffer_reset_tbs_batch.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                                   C.c_uint32, C.c_void_p]
    tbs, Qm, G = 15840, 2, 30000
    rng = np.random.default_rng(77)
    dl = Dlsch(0, 4)
    pool = SoftbufferPool(2, 32)
    desc = [dict(tbs=tbs, Qm=Qm, rv=0, softbuffer=0)]
    for rnd in range(6):
        pay, good = oracle.make_tb(rng, tbs, Qm, G, 0, 20.0)
        pool.reset(0)
        r, d, _ = dl.decode(pool, desc, [good])
        assert r == [0] and np.array_equal(d[0][: tbs // 8], pay[: tbs // 8]), rnd
        if kind == "reset":
            check(L.mi355_softbuffer_reset(pool.h, 0, None), "softbuffer_reset")
        elif kind == "reset_range":
            check(L.mi355_softbuffer_reset_range(pool.h, 0, 2, None), "softbuffer_reset_range")
        else:
            sbs, tb = (C.c_uint32 * 1)(0), (C.c_uint32 * 1)(tbs)
            check(L.mi355_softbuffer_reset_tbs_batch(pool.h, sbs, tb, 1, None), "softbuffer_reset_tbs_batch")
        noise = rng.integers(-300, 301, G).astype(np.int16)
        got = dl.decode(pool, desc, [noise])
        want = _oracle([noise], [(tbs, Qm, G, 0.0)], [0], 4, [oracle.Softbuffer()])
        _check(got, want, [(tbs, Qm, G, 0.0)])
        assert got[0] == [-1], (rnd, got[0])


def _decode_counted(dl, pool, desc, llrs, **kw):
    """One decode with tdec_win_lat's phase counters armed: (results, the 11 counters)."""
    import ctypes as C
    counters = (C.c_uint64 * 11)()
    check(lib().mi355_dlsch_latency_profile(1, None), "latency_profile")
    try:
        got = dl.decode(pool, desc, llrs, **kw)
    finally:
        check(lib().mi355_dlsch_latency_profile(0, C.addressof(counters)), "latency_profile")
    return got, list(counters)


def test_dlsch_latency_path_boundary():
    """The latency path's limit counts the call's code blocks, inclusively, and never applies to int8 LLRs.  One call of
    three single-block TBs -- K = 1024 (16 windows), K = 480 (8 windows), K = 64 (generic): 3 code blocks -- under a
    limit of 3 (the two window blocks decode on tdec_win_lat: its counters run, [10] counts them) and of 2 (none does:
    every counter stays zero); both results are the oracle's.  The same call with int8 LLRs (K = 280 in place of 480,
    which the 8-bit mode rejects) leaves the counters zero under a limit of 512."""
    cases = [(1000, 2, 3010, 1.0), (456, 2, 1500, 0.5), (40, 2, 200, -1.0)]
    assert [oracle.cbsegm(t)["K1"] for t, *_r in cases] == [1024, 480, 64]
    assert sum(oracle.cbsegm(t)["C"] for t, *_r in cases) == 3
    rng = np.random.default_rng(3)
    llrs = [oracle.make_tb(rng, t, q, g, 0, snr)[1] for (t, q, g, snr) in cases]
    desc = [dict(tbs=t, Qm=q, rv=0, softbuffer=i) for i, (t, q, g, s) in enumerate(cases)]
    want = _oracle(llrs, cases, [0] * 3, 6, [oracle.Softbuffer() for _ in cases])
    old = lib().mi355_dlsch_set_latency_path(-1)
    try:
        dl = Dlsch(0, 6)
        for limit in (3, 2):
            lib().mi355_dlsch_set_latency_path(limit)
            got, counters = _decode_counted(dl, SoftbufferPool(3, 2), desc, llrs)
            _check(got, want, cases)
            if limit == 3:
                assert counters[10] == 2 and any(counters[:5]), counters  # [0, 5): phase cycles
            else:
                assert counters == [0] * 11, counters
        lib().mi355_dlsch_set_latency_path(512)
        cases8 = [(1000, 2, 3010), (256, 2, 1080), (40, 2, 200)]
        bits = [rng.integers(0, 2, t, dtype=np.uint8) for t, _q, _g in cases8]
        llrs8 = []
        for b, (t, q, g) in zip(bits, cases8):
            y = np.where(oracle.dlsch_encode_tb(b, t, q, g, 0).astype(bool), 1.0, -1.0) + 0.25 * rng.standard_normal(g)
            llrs8.append(np.clip(np.round(20.0 * y), -127, 127).astype(np.int8))
        desc8 = [dict(tbs=t, Qm=q, rv=0, softbuffer=i) for i, (t, q, g) in enumerate(cases8)]
        (rets, datas, _its), counters = _decode_counted(dl, SoftbufferPool(3, 2), desc8, llrs8, llr8=True)
        assert counters == [0] * 11, counters
        assert rets == [0, 0, 0], rets
        for i, (t, _q, _g) in enumerate(cases8):
            np.testing.assert_array_equal(datas[i][: t // 8], np.packbits(bits[i]), err_msg=f"tbs={t}")
        dl.close()
    finally:
        lib().mi355_dlsch_set_latency_path(old)


# ------------------------------------------------------------------ every code-block size on both turbo paths

# channel SNR of each call: -1 / 0 / 1 dB, where blocks fail or converge late (at 1 dB every TB passes, none at its first
# check), and one call in which TBs do pass at the first check (3 dB for one block, 4 dB for two)
SWEEP_SNRS = {False: (-1.0, 0.0, 1.0, 3.0), True: (-1.0, 0.0, 1.0, 4.0)}
SWEEP_ITS = 4
TWO_BLOCK_SIZES = tuple(K for K in TI.CB_SIZES if K >= 3136)


@functools.lru_cache(maxsize=None)
def _sweep(two_block: bool):
    """Per channel SNR one call's worth of TBs, one per code-block size, and the oracle's decode of each from a
    fresh softbuffer: [(cases, llrs, oracle results)].  Computed once for both parametrisations of dlsch_path."""
    calls = []
    for si, snr in enumerate(SWEEP_SNRS[two_block]):
        rng = np.random.default_rng([188, int(two_block), si])
        cases = []
        for K in (TWO_BLOCK_SIZES if two_block else TI.CB_SIZES):
            size = (2 * K - 72) if two_block else (K - 24)
            sg = oracle.cbsegm(size)
            assert (sg["C"], sg["K1"], sg["C2"], sg["F"]) == (2 if two_block else 1, K, 0, 0), (K, sg)
            cases.append((size, 2, 3 * size + 120, snr))
        llrs = [oracle.make_tb(rng, t, q, g, 0, s)[1] for (t, q, g, s) in cases]
        want = _oracle(llrs, cases, [0] * len(cases), SWEEP_ITS, [oracle.Softbuffer(2) for _ in cases])
        calls.append((cases, llrs, want))
    return calls


def _regime_counts(calls, two_block):
    """{windows: [TBs that fail, that pass after more than one check, that pass at the first check]}"""
    cnt = {0: [0, 0, 0], 8: [0, 0, 0], 16: [0, 0, 0]}
    for cases, _llrs, want in calls:
        for (tbs, *_r), (ret, _d, its) in zip(cases, want):
            K = (tbs + 72) // 2 if two_block else tbs + 24
            cnt[TI.nsb(K)][0 if ret != 0 else (1 if its > 1 else 2)] += 1
    return cnt


def _run_sweep(two_block):
    import ctypes as C
    calls = _sweep(two_block)
    latency = lib().mi355_dlsch_set_latency_path(-1) > 0  # (a negative limit only reads the current one)
    dl = Dlsch(0, SWEEP_ITS)
    pool = SoftbufferPool(len(calls[0][0]), 2)
    for cases, llrs, want in calls:
        # every call within the default latency limit (and the fixture's): the latency parametrisation decodes
        # every window-size block of it on tdec_win_lat, the throughput one none -- counted by the kernel itself
        ncb = sum(oracle.cbsegm(t)["C"] for (t, *_r) in cases)
        nwin = sum(oracle.cbsegm(t)["C"] for (t, *_r) in cases if TI.nsb(oracle.cbsegm(t)["K1"]))
        assert ncb == len(cases) * (2 if two_block else 1) and ncb <= 256
        assert nwin == (96 if two_block else 142)
        pool.reset_all()
        counters = (C.c_uint64 * 11)()
        check(lib().mi355_dlsch_latency_profile(1, None), "latency_profile")
        desc = [dict(tbs=t, Qm=q, rv=0, softbuffer=i) for i, (t, q, g, s) in enumerate(cases)]
        try:
            got = dl.decode(pool, desc, llrs)
        finally:
            check(lib().mi355_dlsch_latency_profile(0, C.addressof(counters)), "latency_profile")
        assert counters[10] == (nwin if latency else 0), (counters[10], nwin, latency)  # [10]: code blocks it decoded
        _check(got, want, cases)
    dl.close()
    pool.close()


def test_dlsch_every_size_single_block():
    """All 188 sizes as single-block TBs (tbs = K - 24, CRC24A), one call of 188 code blocks per channel SNR of -1 /
    0 / 1 / 3 dB, 4 half-iterations at most: at every K the latency kernel (uneven halves for odd L, whole-byte DEC1
    decisions for L % 16 == 0, every length of the last output chunk) and the throughput kernels meet blocks that
    fail, that converge late and that pass at the first check.  Return codes, payload + CRC bytes and iteration counts
    are the oracle's.  Reference condition, on the oracle: in each regime at least 5 TBs of each kind; observed (fail,
    pass after more than one check, pass at the first): generic 20 / 104 / 60, 8 windows 27 / 79 / 22, 16 windows
    128 / 293 / 19.  (At -1 / 0 / 1 dB alone no window-size TB passes at its first check, hence the 3 dB call.)"""
    cnt = _regime_counts(_sweep(False), False)
    assert all(min(v) >= 5 for v in cnt.values()), cnt
    _run_sweep(False)


def test_dlsch_every_size_two_blocks():
    """Every K >= 3136 as a two-block TB (tbs = 2 K - 72: CRC24B per block and the TB's CRC24A), 96 code blocks per
    call, at -1 / 0 / 1 / 4 dB.  Observed on the oracle: 73 TBs fail, 101 pass after more than one check, 18 at the
    first check of both blocks."""
    assert len(TWO_BLOCK_SIZES) == 48
    cnt = _regime_counts(_sweep(True), True)
    assert cnt[0] == cnt[8] == [0, 0, 0] and min(cnt[16]) >= 5, cnt
    _run_sweep(True)
