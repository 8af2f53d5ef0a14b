"""The oracle's turbo rate dematcher at every code-block size, redundancy version and class of E against the compiled
reference's own (srslte_rm_turbo_rx_lut and srslte_rm_turbo_rx_lut_8bit through oracle/_ref): tests/golden/rm_turbo.npz
holds the reference's results at 6 of the 188 sizes, and the product's table generator (csrc/rm_tables.h) is the same
restatement as the oracle's (oracle/orc_sch.c), so a shared mistake in the dummy-bit count, in R or in the float ceilf of
k0 at one of the other 182 sizes would pass every GPU comparison with the oracle.  Bit-exact, whole buffers (so a write
outside the code-bit positions shows too).  The host-side coverage tests need no reference and no GPU."""
import collections

import numpy as np
import pytest

import oracle
import rm_inputs as RI
import tdec_inputs as TI
from golden_io import rm_init_softbuffer

needs_ref = pytest.mark.skipif(not oracle.ref_available(), reason="needs oracle/_ref (built where the reference is)")


@needs_ref
@pytest.mark.parametrize("init", ["zeroed", "filled"])
def test_oracle_rm_every_size_rv_E_matches_reference(init):
    """188 K x 4 rv x the 7 E classes (5,264 cases per parametrisation, LLR classes cycled), into zeroed buffers and
    into rm_init_softbuffer() contents (wrapping sums)."""
    R = oracle.ref()
    start = np.zeros(oracle.SOFTBUFFER_SIZE, np.int16) if init == "zeroed" else rm_init_softbuffer()
    bad, n = [], 0
    for K in RI.CB_SIZES:
        for rv in RI.RVS:
            for ei, (ecls, E) in enumerate(RI.e_classes(K, rv).items()):
                e = RI.llrs(K, rv, ecls, E, RI.LLR_CLASSES[(n + ei) % 4])
                want = start.copy()
                assert R.ref_rm_turbo_rx(np.array(e), E, want, K, rv) == 0
                got = oracle.rm_turbo_rx(e, K, rv, start.copy())
                if not np.array_equal(got, want):
                    bad.append((K, rv, ecls, E))
                n += 1
    assert n == 188 * 4 * 7
    assert not bad, (len(bad), bad[:10])


@needs_ref
def test_int8_restatement_matches_reference():
    """rm_inputs.rm_rx8 (the 16-bit table in the 8-bit layout, wrapping int8 sums) against srslte_rm_turbo_rx_lut_8bit:
    188 K x 4 rv x {third, N, 2N + 18} into a zeroed buffer, then a second accumulation at (rv + 2) % 4."""
    R = oracle.ref()
    bad, n = [], 0
    for K in RI.CB_SIZES:
        for rv in RI.RVS:
            ec = RI.e_classes(K, rv)
            for ecls in RI.E_CLASSES8:
                E = ec[ecls]
                want = np.zeros(2 * oracle.SOFTBUFFER_SIZE, np.int8)
                got = want.copy()
                for tx, r in enumerate((rv, (rv + 2) % 4)):
                    e = RI.llrs8(K, rv, ecls, E, tx)
                    assert R.ref_rm_turbo_rx_8bit(np.array(e), E, want, K, r) == 0
                    RI.rm_rx8(e, K, r, got)
                    if not np.array_equal(got, want):
                        bad.append((K, rv, ecls, E, tx))
                        break
                n += 1
    assert n == 188 * 4 * 3
    assert not bad, (len(bad), bad[:10])


# ------------------------------------------------------------------ host-side coverage (no reference, no GPU)

def test_sparse_interval_exists_at_every_16_window_size():
    """Every 16-window size has, at every rv, E <= N for which some parity row holds an LLR and some row holds none;
    the sparse-mid class lies inside that interval, and the interval ends between 0.05 N and 0.98 N."""
    ratios = []
    for K in TI.CB_SIZES:
        for rv in RI.RVS:
            iv = RI.sparse_interval(K, rv)
            assert (iv is not None) == (TI.nsb(K) == 16)
            E = RI.e_classes(K, rv)["sparse_mid"]
            assert E % 2 == 0
            if iv is None:
                continue
            lo, hi = iv
            assert lo <= E <= hi <= RI.N_of(K), (K, rv, lo, hi, E)
            f = RI.features(K, rv, E, 0)
            assert f["rows_mixed"], (K, rv, E, f)
            ratios.append(hi / RI.N_of(K))
    assert len(ratios) == 110 * 4  # 13 sizes of 816 .. 1008, 32 of 1024 .. 2016, 65 of 2048 .. 6144
    assert 0.04 < min(ratios) < 0.06 and 0.97 < max(ratios) < 0.99, (min(ratios), max(ratios))


def test_sweep_covers_every_choice():
    """Over (K, rv, E class) with e_offset % 8 cycling as the GPU sweep does: every value of every size-dependent
    choice of the rate dematchers occurs, per window-count class where it depends on the layout."""
    seen = collections.defaultdict(set)
    for rv in RI.RVS:
        i = 0
        for K in TI.CB_SIZES:
            assert RI.nd(K) in (4, 12, 20, 28)
            seen["nd"].add(RI.nd(K))
            seen["nsb8"].add(RI.nsb8_layout(K))
            for ecls, E in RI.e_classes(K, rv).items():
                f = RI.features(K, rv, E, i % 8)
                seen["load"].add((f["nsb"], ecls, f["load"]))
                seen["wraps"].add((f["nsb"], f["wraps"]))
                seen["tail_quads"].add(f["tail_quads"])
                seen["passes"].add(f["passes"])
                seen["sparse"].add((f["nsb"], ecls, f["sparse"]))
                seen["eqrm_ok"].add((ecls, f["eqrm_ok"]))
                i += 1
    assert seen["nd"] == {4, 12, 20, 28}
    assert seen["nsb8"] == {0, 8, 16, 32}
    assert seen["load"] == {(n, c, k) for n in (0, 8, 16) for c in RI.E_CLASSES for k in ("e16", "e4", "unaligned")}
    assert seen["wraps"] == {(n, w) for n in (0, 8, 16) for w in (0, 1, 2, 4)}
    # (K is a multiple of 8: the last 16-byte store of every buffer is partial, two pairs)
    assert seen["tail_quads"] == {2} and seen["passes"] == set(range(1, 6)), (seen["tail_quads"], seen["passes"])
    # rows are left unwritten at sparse-mid at every 16-window size, at N / 3 at some; never from N - 2 on
    assert {(16, "sparse_mid", True), (16, "third", True), (16, "third", False), (16, "N-2", False),
            (0, "sparse_mid", False), (8, "sparse_mid", False)} <= seen["sparse"]
    assert (16, "sparse_mid", False) not in seen["sparse"] and (16, "N", True) not in seen["sparse"]
    assert seen["eqrm_ok"] == {("sparse_mid", True), ("third", True), ("N-2", True), ("N", False), ("N+2", False),
                               ("2N+18", False), ("4N+6", False)}


def test_harq_orders_meet_every_window_class():
    """The HARQ sweep's round-robin of rv orders over the sizes: every order meets generic, 8- and 16-window sizes."""
    met = {(i % len(RI.HARQ_ORDERS), TI.nsb(K)) for i, K in enumerate(TI.CB_SIZES)}
    assert met == {(o, n) for o in range(len(RI.HARQ_ORDERS)) for n in (0, 8, 16)}


def test_segmentation_helpers():
    assert len(RI.two_size_tbs()) == 1532
    for C in (2, 3, 5, 11, 13):
        sg = oracle.cbsegm(RI.one_size_tbs(C))
        assert (sg["C"], sg["C2"], sg["F"]) == (C, 0, 0)
