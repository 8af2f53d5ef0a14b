"""CPU pin of the oracle's convolutional-decoder chain (orc_rm_conv_rx -> orc_viterbi_quant ->
orc_viterbi37_tb_decode_us -> orc_crc16_bits, oracle/orc_pdcch.c) against the reference's own code (oracle/_ref:
srslte_rm_conv_rx, srslte_viterbi_decode_f of the AVX2 build, srslte_crc_checksum) at EVERY block length -- payloads of
1..128 bits, E = 72 / 144 / 288 / 576 / 1920, every input class of tests/conv_inputs.py -- and in the PBCH's scaled
form.  tests/golden/pdcch.npz pins the restatement only at the lengths recorded there; the GPU sweep
(tests/test_conv_decode_gpu.py) compares the device with this oracle, so this is the link to the reference."""
import numpy as np
import pytest

import conv_inputs as CI
import oracle

pytestmark = pytest.mark.skipif(not oracle.ref_available(), reason="oracle/_ref not built")


def _mismatches(cases, scale_of):
    bad = []
    for c in cases:
        nbits, llr = c[0], c[3]
        got = CI.oracle_decode(llr, nbits, scale_of(c))
        ref = CI.oracle_decode(llr, nbits, scale_of(c), use_ref=True)
        if not (np.array_equal(got[0], ref[0]) and got[1] == ref[1]):
            bad.append(c[:3])
    return bad


def test_unscaled_chain_matches_reference_at_every_length():
    cases = CI.sweep(CI.SWEEP_E + (CI.PBCH_E,))
    assert len(cases) == 128 * 5 * len(CI.CLASSES)
    bad = _mismatches(cases, lambda c: None)
    assert not bad, (len(bad), bad[:20])


def test_scaled_chain_matches_reference():
    cases = CI.scaled_jobs()
    assert len(cases) == (10 * 4 + len(CI.SCALED_NBITS)) * len(CI.CLASSES)
    bad = _mismatches(cases, lambda c: c[2])
    assert not bad, (len(bad), bad[:20])


def test_clean_blocks_decode_on_the_reference():
    """The sweep is not vacuous: the reference itself recovers every clean block that is not punctured."""
    n = 0
    for nbits, E, cls, llr, d in CI.sweep(CI.SWEEP_E + (CI.PBCH_E,)):
        if cls == "clean" and E >= 3 * (nbits + 16):
            bits, rem = CI.oracle_decode(llr, nbits, use_ref=True)
            assert np.array_equal(bits, d) and rem == 0, (nbits, E)
            n += 1
    assert n == 248 + 128
