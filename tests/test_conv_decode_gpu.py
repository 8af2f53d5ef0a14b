"""GPU parity of the convolutional-decoder wave (srsran_amd/csrc/conv_decode.h: rate dematching, quantisation,
tail-biting Viterbi in the rotating lane layout, chainback, CRC16) at EVERY block length the API admits, through
mi355_debug_conv_decode_batch -- the same gate_pass / decode_cand<false> the PDCCH blind search runs (mode 0) and the
same decode_cand<true> the PBCH decoder runs (mode 1), one wave per job.

The product's two callers produce about a dozen of the 128 lengths; here every payload size 1..128 (F = 17..144) meets
E = 72 / 144 / 288 / 576 and every input class of tests/conv_inputs.py, and status, CRC remainder and payload must
equal the oracle's (oracle/orc_pdcch.c) bit for bit.  tests/test_conv_decode_oracle.py pins that oracle to the
reference's own code over the same inputs.  Each test is one launch."""
import numpy as np
import pytest

import conv_inputs as CI
from oracle import pdcch_chain as P

gpu = pytest.mark.gpu  # (the tests on the generator, the oracle and the entry's argument checks run anywhere)


def _payload_words(bits, nbits):
    """bits[4] of a candidate record: the payload MSB first in 32-bit words, zero past nbits"""
    b = np.zeros(128, np.uint8)
    b[:nbits] = bits[:nbits]
    return np.packbits(b).view(">u4").astype(np.uint32)


@pytest.fixture(scope="module")
def sweep_reference():
    """P.decode_candidate (gate + decode chain) for every case of the sweep, computed once"""
    ref = []
    for nbits, E, _cls, llr, _d in CI.sweep():
        L = {72: 0, 144: 1, 288: 2, 576: 3}[E]
        ref.append(P.decode_candidate(llr, L, 0, nbits))
    return ref


def test_sweep_covers_every_path():
    """Every value of every length-dependent path of decode_cand occurs in the sweep (computed from F and E alone)."""
    seen = {k: set() for k in CI.FEATURE_VALUES}
    for nbits in range(1, 129):
        for E in CI.SWEEP_E:
            for k, v in CI.features(nbits, E).items():
                seen[k].add(v)
    assert seen == CI.FEATURE_VALUES
    # every row count of the dematcher runs both punctured and not
    both = {(f["nrows"], f["punctured"]) for f in (CI.features(n, E) for n in range(1, 129) for E in CI.SWEEP_E)}
    assert both == {(r, p) for r in range(1, 6) for p in (False, True)}


def test_reference_conditions(sweep_reference):
    """Asserted on the oracle alone, so the comparison below cannot pass vacuously: clean unpunctured blocks decode
    to what was sent; 0.25 and the float32 below 0.3 are gated out, float32(0.3) (0.30000001192... in double) and the
    signal / noise classes pass the gate."""
    clean = 0
    for (nbits, E, cls, _llr, d), (ok, bits, rem) in zip(CI.sweep(), sweep_reference):
        if cls in ("gate_0.25", "gate_below_0.3f", "zeros", "tiny"):
            assert not ok, (nbits, E, cls)
        if cls in ("gate_0.3f", "clean", "noisy", "noise", "ties", "sat", "huge", "halfsteps"):
            assert ok, (nbits, E, cls)
        if cls == "clean" and E >= 3 * (nbits + 16):
            assert np.array_equal(bits, d[:nbits]) and rem == 0, (nbits, E)
            clean += 1
    assert clean == 248
    assert float(CI.BELOW_03) < 0.3 < float(np.float32(0.3))


@gpu
def test_mode0_every_length_matches_oracle(sweep_reference):
    """6,144 jobs in one launch: nbits 1..128 x E in {72, 144, 288, 576} x 12 input classes."""
    from srsran_amd import pdcch as D
    cases = CI.sweep()
    assert len(cases) == 128 * 4 * 12
    got = D.conv_decode_debug([(llr, nbits, 0, 1.0) for nbits, _E, _c, llr, _d in cases])
    bad = []
    for (nbits, E, cls, _llr, _d), (ok, bits, rem), g in zip(cases, sweep_reference, got):
        if ok:
            want = (2, rem, _payload_words(bits, nbits).tolist())
        else:
            want = (1, 0, [0, 0, 0, 0])
        have = (int(g["status"]), int(g["crc_rem"]), g["bits"].tolist())
        if have != want or (int(g["L"]), int(g["ncce"])) != (0, 0):
            bad.append((nbits, E, cls, have, want))
    assert not bad, (len(bad), sorted({b[0] for b in bad}), bad[:10])


@gpu
def test_mode1_scaled_matches_oracle():
    """The PBCH's form, 564 jobs in one launch: F = 40 over all 10 decode_frame windows x 4 scales x 12 classes, then
    nbits 1 / 47 / 48 / 64 / 112 / 113 / 128 at E = 1920 and scale 0.25.  No gate in this mode: every job decodes."""
    from srsran_amd import pdcch as D
    cases = CI.scaled_jobs()
    assert len(cases) == 10 * 4 * 12 + 7 * 12
    got = D.conv_decode_debug([(llr, nbits, 1, scale) for nbits, _label, scale, llr, _d in cases])
    bad, clean = [], 0
    for (nbits, label, scale, llr, d), g in zip(cases, got):
        bits, rem = CI.oracle_decode(llr, nbits, scale)
        if label.startswith("clean"):  # every window of the clean block carries >= 3F values of it
            assert np.array_equal(bits, d) and rem == 0, (nbits, label)
            clean += 1
        want = (2, rem, _payload_words(bits, nbits).tolist())
        have = (int(g["status"]), int(g["crc_rem"]), g["bits"].tolist())
        if have != want:
            bad.append((nbits, label, scale, have, want))
    assert clean == 10 * 4 + 7
    assert not bad, (len(bad), bad[:10])


def test_entry_rejects_bad_jobs():
    """nbits = 0, nbits > 128, E = 0, E > 1920 in mode 1, an unknown mode: refused on the host, nothing launched"""
    from srsran_amd import pdcch as D
    x = np.ones(2000, np.float32)
    for llr, nbits, mode in ((x[:72], 0, 0), (x[:72], 129, 0), (x[:0], 24, 0), (x[:1921], 24, 1), (x[:72], 24, 2)):
        with pytest.raises(RuntimeError):
            D.conv_decode_debug([(llr, nbits, mode, 1.0)])
