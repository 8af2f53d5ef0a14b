"""GPU parity of the decision bytes the window MAP kernel (tdec_kernels.hip) collects in its LDS bitmap.

bm_set ORs every decision into the code block's bitmap word with an operand that is zero for a clear bit, so what can
go wrong is the operand: a set bit lost, a clear bit set, or a bit at the wrong place of its byte.  Payloads of all
zeros, all ones, 0xAA and 0x55 bytes and one random one, over LLRs clean enough that every half-iteration decides the
payload itself (asserted on the oracle), put a clear and a set bit at each of the 8 positions of every byte; one noisy
block per K has decisions that are not the payload and change from one half-iteration to the next.

Sizes, the smallest that reach each bitmap path, and K = 6144:
  512   8 windows, L = 64: DEC2 through the bitmap
  832   16 windows, L = 52 (L % 8 = 4, K % 64 = 0): windows not byte-aligned, so DEC1 writes through the bitmap too
  1024  16 windows, L = 64: DEC1 packs bytes in registers, DEC2 through the bitmap; 16-byte loads for a full wave
  1056  16 windows, L = 66, K % 64 = 32: the decision bytes do not split over the lanes' 8-byte stores, so this size
        keeps the D array and the decide pass (tdec_runtime.cpp `fuse`) and pins that the bitmap is not taken here
  6144  16 windows, L = 384
8 blocks are one full wave of 16-window blocks (the 16-byte-load body), 11 a full wave and a partial one (both bodies
in one launch).  The decision bytes after half-iterations 1, 2 and 3 (DEC1 without a-priori, DEC2, DEC1 with a-priori)
must equal the oracle's, byte for byte, on an output buffer preset to 0xA5.

Through the DL-SCH (throughput path): 11 single-block TBs per K.  A first call at 2 dB, where the oracle's blocks pass
their CRC at the first DEC2, makes the decoder's policy take that DEC2 speculatively in the next call (K = 1024 and
6144: tdec_win_spec_ok; the other sizes run the same two calls without speculation); the second call at 0 dB has
blocks that fail that check, so the speculative DEC2 and its redo both run.  Return codes, payload and CRC bytes and
iteration counts are the oracle's in both calls."""
import functools

import numpy as np
import pytest

import oracle
import tdec_inputs as TI

gpu = pytest.mark.gpu

KS = (512, 832, 1024, 1056, 6144)
NCB = (8, 11)
NHALF = 3
PAD_OUT = 768  # a multiple of 8: decisions packed in the kernel
PAYLOADS = ("zeros", "ones", "aa", "55", "rand")
EBNO_CLEAN, EBNO_NOISY = 12.0, 1.0


def payload_bits(K, kind):
    if kind == "rand":
        return np.random.default_rng([29, K]).integers(0, 2, K, dtype=np.uint8)
    byte = {"zeros": 0x00, "ones": 0xFF, "aa": 0xAA, "55": 0x55}[kind]
    return np.unpackbits(np.full(K // 8, byte, np.uint8))


@functools.lru_cache(maxsize=None)
def inputs(K):
    """[(payload bytes, decoder buffer, (NHALF, K/8) oracle decisions)]: the five clean payloads, then the noisy block"""
    out = []
    for k, kind in enumerate(PAYLOADS + ("rand",)):
        bits = payload_bits(K, kind)
        rng = np.random.default_rng([31, K, k])
        lin = oracle.awgn_llrs(rng, oracle.tcod_encode(bits, K), EBNO_CLEAN if k < len(PAYLOADS) else EBNO_NOISY)
        buf = oracle.tdec_pack_input(lin, K)
        tr = oracle.tdec_run(buf, K, NHALF, trace=True)[1]
        for v in (buf, tr):
            v.setflags(write=False)
        out.append((np.packbits(bits), buf, tr))
    return out


def test_inputs_are_what_they_are_chosen_for():
    geo = {K: (TI.nsb(K), K // TI.nsb(K)) for K in KS}
    assert geo == {512: (8, 64), 832: (16, 52), 1024: (16, 64), 1056: (16, 66), 6144: (16, 384)}
    fuse = {K: TI.features(K)["fuse_capable"][1] for K in KS}
    full = {K: TI.features(K)["full"][1] for K in KS}
    assert fuse == {512: True, 832: True, 1024: True, 1056: False, 6144: True}
    assert full == {512: True, 832: False, 1024: True, 1056: False, 6144: True}  # 832: DEC1 through the bitmap too
    for K in (512, 832, 1024, 1056):  # (6144 behaves alike and is left to the GPU test's own oracle run)
        blocks = inputs(K)
        for want, _buf, tr in blocks[: len(PAYLOADS)]:
            for h in range(NHALF):
                np.testing.assert_array_equal(tr[h], want, err_msg=f"K={K} half {h + 1}")
        want, _buf, tr = blocks[-1]
        assert all(not np.array_equal(tr[h], want) for h in range(NHALF)), K
        assert not np.array_equal(tr[0], tr[1]) and not np.array_equal(tr[1], tr[2]), K


@pytest.fixture(scope="module")
def dev():
    from srsran_amd.tdec import DeviceBuffer, TdecBatch
    d = dict(dec=TdecBatch(0), d_in=DeviceBuffer(max(NCB) * TI.SB_STRIDE * 2), d_out=DeviceBuffer(max(NCB) * PAD_OUT))
    yield d
    d["dec"].close()


@gpu
@pytest.mark.parametrize("K", KS)
def test_decision_bytes_match_oracle(dev, K):
    from srsran_amd import lib
    blocks = inputs(K)
    host = np.zeros((max(NCB), TI.SB_STRIDE), np.int16)
    for i in range(max(NCB)):
        buf = blocks[i % len(blocks)][1]
        host[i, : buf.size] = buf
    dev["d_in"].upload(host)
    bad = []
    for ncb in NCB:
        lib().mi355_memset_dev(dev["d_out"].ptr, 0xA5, dev["d_out"].nbytes)
        for h in range(NHALF):
            dev["dec"].halfit_dev(dev["d_in"].ptr, TI.SB_STRIDE, ncb, K, h, dev["d_out"].ptr, PAD_OUT)
            got = dev["d_out"].download(np.zeros((max(NCB), PAD_OUT), np.uint8))[:ncb, : K // 8]
            for i in range(ncb):
                want = blocks[i % len(blocks)][2][h]
                if not np.array_equal(got[i], want):
                    w = int(np.flatnonzero(got[i] != want)[0])
                    bad.append((ncb, h + 1, i, w, hex(got[i][w]), hex(want[w])))
    assert not bad, (K, bad[:8])  # (blocks, half-iteration, block, first byte that differs, got, want)


# ------------------------------------------------------------------ through the DL-SCH

MAX_ITS = 6
NTB = 11
SNR_FIRST, SNR_SECOND = 2.0, 0.0


@functools.lru_cache(maxsize=None)
def dlsch_calls(K):
    """The two calls' (LLRs, oracle results) of NTB single-block TBs with code-block size K"""
    tbs = K - 24
    sg = oracle.cbsegm(tbs)
    assert (sg["C"], sg["K1"], sg["F"]) == (1, K, 0), sg
    calls = []
    for c, snr in enumerate((SNR_FIRST, SNR_SECOND)):
        rng = np.random.default_rng([37, K, c])
        llrs = [oracle.make_tb(rng, tbs, 2, 3 * tbs + 120, 0, snr)[1] for _ in range(NTB)]
        want = [oracle.dlsch_decode_tb(e, tbs, 2, 0, MAX_ITS, oracle.Softbuffer(2)) for e in llrs]
        calls.append((llrs, want))
    return calls


@pytest.fixture()
def throughput_path():
    from srsran_amd import lib
    old = lib().mi355_dlsch_set_latency_path(0)  # a half-iteration per launch: tdec_kernels.hip
    yield
    lib().mi355_dlsch_set_latency_path(old)


@gpu
@pytest.mark.parametrize("K", KS)
def test_dlsch_speculative_dec2_and_redo(throughput_path, K):
    from srsran_amd.dlsch import Dlsch, SoftbufferPool
    tbs = K - 24
    (llrs1, want1), (llrs2, want2) = dlsch_calls(K)
    # dlsch_runtime.cpp spec_policy on the oracle's counts of the first call: half-iteration 1 (the first DEC2) is
    # speculative in the second when at most a tenth of the blocks that ran it went on
    its1 = [a for _r, _d, a in want1]
    run, fail = sum(a > 1.5 for a in its1), sum(a > 2.5 for a in its1)
    assert run and fail * 10 <= run, its1
    # the second call: TBs that pass, some of them only after the first DEC2 (they take the redo)
    assert any(r == 0 and a > 2.5 for r, _d, a in want2), [(r, a) for r, _d, a in want2]
    dl, pool = Dlsch(0, MAX_ITS), SoftbufferPool(NTB, 2)
    n = tbs // 8 + 3
    for llrs, want in ((llrs1, want1), (llrs2, want2)):
        pool.reset_all()
        got = dl.decode(pool, [dict(tbs=tbs, Qm=2, rv=0, softbuffer=i) for i in range(NTB)], llrs)
        for i, (r, d, a) in enumerate(want):
            assert got[0][i] == r, (K, i, got[0][i], r)
            np.testing.assert_array_equal(got[1][i][:n], d[:n], err_msg=f"K={K} tb {i}")
            assert abs(got[2][i] - a) < 1e-5, (K, i, got[2][i], a)
    dl.close()
    pool.close()
