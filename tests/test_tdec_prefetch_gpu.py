"""GPU parity of the window MAP kernel (tdec_kernels.hip) at the shapes where its segment prefetch can go wrong.

The kernel keeps loads in flight across segments: the forward pass prefetches segment min(t + 1, nseg - 1) from every
segment, the backward pass runs whole triples of segments that prefetch max(t - 2, 0) and then nseg % 3 segments
without a prefetch, and the 16-byte-load (TX) path reads the parity pieces of rows without an LLR from a zero block.
So the sizes here are the smallest with nseg = 7, 8, 9 (every nseg % 3 and nseg % 2) for 16 windows and for 8, one
ragged size (L % 8 != 0) per window count, and K = 6144; the block counts give a partial wave (4-byte loads only), one
full wave (16-byte loads), and both in one launch.  Decisions are compared with the oracle's after each of 3
half-iterations, so DEC1 without a-priori, DEC2 and DEC1 with a-priori (MODE 0, 2, 1) all run.

Through the DL-SCH (throughput path, K = 6144, 16 code blocks a TB): fresh buffers at code rate 0.85 (sparse parity-row
bitmaps), two blocks that finish early (their waves fall back to 4-byte loads), an rv 2 retransmission combined into
the buffers (all-ones bitmaps), and a grant so short that whole 32-row words of the P0 bitmap are empty."""
import numpy as np
import pytest

import oracle
import tdec_inputs as TI

gpu = pytest.mark.gpu  # (the test on the chosen sizes runs anywhere)

NHALF = 3
NCB = (1, 7, 8, 9, 17)
PAD_OUT = 768  # a multiple of 8: decisions packed in the kernel
# K: (windows, nseg, L % 8)
SIZES = {896: (16, 7, 0), 1024: (16, 8, 0), 1152: (16, 9, 0), 6144: (16, 48, 0),
         448: (8, 7, 0), 512: (8, 8, 0), 576: (8, 9, 0),
         416: (8, 7, 4), 1008: (16, 8, 7)}


def test_sizes_are_what_they_are_chosen_for():
    for K, (n, nseg, rem) in SIZES.items():
        L = K // TI.nsb(K)
        assert (TI.nsb(K), -(-L // TI.TDEC_SEG), L % TI.TDEC_SEG) == (n, nseg, rem), K
    assert {(n, nseg % 3) for n, nseg, rem in SIZES.values() if not rem} == {(n, r) for n in (8, 16) for r in range(3)}
    assert (2 * TI.SB_STRIDE) % 16 == 0  # the 16-byte-load path's input stride


@pytest.fixture(scope="module")
def dev():
    from srsran_amd.tdec import DeviceBuffer, TdecBatch
    d = dict(dec=TdecBatch(0), d_in=DeviceBuffer(max(NCB) * TI.SB_STRIDE * 2), d_out=DeviceBuffer(max(NCB) * PAD_OUT))
    yield d
    d["dec"].close()


@gpu
@pytest.mark.parametrize("K", sorted(SIZES))
def test_half_iterations_match_oracle(dev, K):
    """1, 7, 8, 9 and 17 blocks (the input classes of tests/tdec_inputs.py in turn) from softbuffer-slot strides: the
    decisions after half-iterations 1, 2 and 3 are the oracle's, bit for bit"""
    from srsran_amd import lib
    traces = TI.window_traces(K)
    host = np.zeros((max(NCB), TI.SB_STRIDE), np.int16)
    for i in range(max(NCB)):
        r = TI.block(K, TI.CLASSES[i % len(TI.CLASSES)])[2]
        host[i, : r.size] = r
    dev["d_in"].upload(host)
    bad = []
    for ncb in NCB:
        want = np.stack([traces[TI.CLASSES[i % len(TI.CLASSES)]] for i in range(ncb)], axis=1)  # (8, ncb, K/8)
        lib().mi355_memset_dev(dev["d_out"].ptr, 0xA5, dev["d_out"].nbytes)
        for h in range(NHALF):
            dev["dec"].halfit_dev(dev["d_in"].ptr, TI.SB_STRIDE, ncb, K, h, dev["d_out"].ptr, PAD_OUT)
            got = dev["d_out"].download(np.zeros((max(NCB), PAD_OUT), np.uint8))[:ncb, : K // 8]
            if not np.array_equal(got, want[h]):
                bad.append((ncb, h + 1, [i for i in range(ncb) if not np.array_equal(got[i], want[h][i])]))
                break
    assert not bad, (K, bad)


# ------------------------------------------------------------------ through the DL-SCH

TB = (97896, 8, 115200)  # TM4 MCS 27 codeword of the benchmark: C = 16, K = 6144, code rate 0.85
MAX_ITS = 4


@pytest.fixture()
def throughput_path():
    from srsran_amd import lib
    old = lib().mi355_dlsch_set_latency_path(0)  # a half-iteration per launch: tdec_kernels.hip
    yield
    lib().mi355_dlsch_set_latency_path(old)


def p0_rows(K, E, rv):
    """The rows (steps j of the 16 windows) of the first parity stream that the first E LLRs of redundancy version rv
    reach, from the oracle's dematching table"""
    t = oracle.rm_turbo_table(K, rv)[:E].astype(np.int64)
    p = t[(t >= K + 32) & (t < 2 * K + 32)] - (K + 32)
    return np.unique(p // 16)


def _decode_and_check(dl, pool, sbs, tbs, Qm, rv, llrs):
    got = dl.decode(pool, [dict(tbs=tbs, Qm=Qm, rv=rv, softbuffer=i) for i in range(len(llrs))], llrs)
    want = [oracle.dlsch_decode_tb(llrs[i], tbs, Qm, rv, MAX_ITS, sbs[i]) for i in range(len(llrs))]
    C = oracle.cbsegm(tbs)["C"]
    n = tbs // 8 + (6 if C > 1 else 3)
    for i, (r, d, a) in enumerate(want):
        assert got[0][i] == r, (i, got[0][i], r)
        np.testing.assert_array_equal(got[1][i][:n], d[:n], err_msg=f"tb {i}")
        assert abs(got[2][i] - a) < 1e-5, (i, got[2][i], a)
    return want


def _two_noise_levels(seed, tbs, Qm, G, E):
    """One TB's LLRs at 7 dB, and the same with the noise of code blocks 3 and 12 at 30 dB"""
    rng = np.random.default_rng(seed)
    coded = oracle.dlsch_encode_tb(rng.integers(0, 2, tbs, dtype=np.uint8), tbs, Qm, G, 0)
    noise = rng.standard_normal(G)
    out = []
    for quiet in ((), (3, 12)):
        sigma = np.full(G, 10 ** (-7.0 / 20))
        for cb in quiet:
            sigma[cb * E: (cb + 1) * E] = 10 ** (-30.0 / 20)
        y = np.where(coded.astype(bool), 1.0, -1.0) + sigma * noise
        out.append(np.trunc(100 * y).clip(-32768, 32767).astype(np.int16))
    return out


@gpu
def test_dlsch_fresh_sparse_rows_and_early_blocks(throughput_path):
    """Fresh buffers at the benchmark's rate: 7 of 8 parity rows hold no LLR (asserted from the dematching table).  TB 0
    as received; in TB 1 code blocks 3 and 12 have almost no noise, so these two pass their CRC before the blocks
    around them (the oracle's average iteration count drops) and both waves of the TB go on with 4-byte loads."""
    from srsran_amd.dlsch import Dlsch, SoftbufferPool
    tbs, Qm, G = TB
    E = G // 16
    rows = p0_rows(6144, E, 0)
    assert 0 < rows.size <= 384 // 8 + 1
    base, clean = _two_noise_levels(41, tbs, Qm, G, E)
    dl, pool = Dlsch(0, MAX_ITS), SoftbufferPool(2, 16)
    want = _decode_and_check(dl, pool, [oracle.Softbuffer() for _ in range(2)], tbs, Qm, 0, [base, clean])
    assert 1.0 < want[1][2] < want[0][2]  # (the two clean blocks stopped earlier, the others went on)
    dl.close()
    pool.close()


@gpu
def test_dlsch_rv2_combined_all_rows(throughput_path):
    """A first transmission too noisy to decode, then rv 2 combined into the same buffers: every parity row may hold an
    LLR now (all-ones bitmaps), on buffers whose rows the first decode left unwritten"""
    from srsran_amd.dlsch import Dlsch, SoftbufferPool
    tbs, Qm, G = TB
    rng = np.random.default_rng(43)
    bits = rng.integers(0, 2, tbs, dtype=np.uint8)
    dl, pool = Dlsch(0, MAX_ITS), SoftbufferPool(1, 16)
    sbs = [oracle.Softbuffer()]
    rets = []
    for rv in (0, 2):
        coded = oracle.dlsch_encode_tb(bits, tbs, Qm, G, rv)
        y = np.where(coded.astype(bool), 1.0, -1.0) + 10 ** (-4.0 / 20) * rng.standard_normal(G)
        llr = np.trunc(100 * y).clip(-32768, 32767).astype(np.int16)
        rets.append(_decode_and_check(dl, pool, sbs, tbs, Qm, rv, [llr])[0][0])
    assert rets == [-1, 0]  # (the second decode needed the first one's LLRs)
    dl.close()
    pool.close()


@gpu
def test_dlsch_empty_bitmap_words(throughput_path):
    """A grant of E = 5780 LLRs a code block: rv 0 starts at the third column of the systematic stream and reaches only
    the first rows of the first parity column, so the P0 bitmap has set bits in its first words and words without any
    (asserted from the dematching table).  Nothing decodes at this rate; the decisions, return codes and iteration
    counts are still the oracle's."""
    from srsran_amd.dlsch import Dlsch, SoftbufferPool
    tbs, Qm, G = TB[0], 2, 16 * 5780
    words = np.bincount(p0_rows(6144, G // 16, 0) // 32, minlength=12)
    assert words[0] > 0 and (words == 0).any(), words
    rng = np.random.default_rng(47)
    llrs = [oracle.make_tb(rng, tbs, Qm, G, 0, 30.0)[1]]
    dl, pool = Dlsch(0, MAX_ITS), SoftbufferPool(1, 16)
    _decode_and_check(dl, pool, [oracle.Softbuffer()], tbs, Qm, 0, llrs)
    dl.close()
    pool.close()
