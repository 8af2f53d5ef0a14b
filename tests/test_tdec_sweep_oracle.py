"""CPU pin of the oracle's turbo decoders (oracle/orc_tdec.c: the 8- / 16-window decoder and the generic one) against
the reference's own (oracle/_ref: srslte_tdec_iteration of the AVX2 build in AUTO mode, and the GENERIC manual decoder
with force_not_sb) at EVERY code-block size, on every input class of tests/tdec_inputs.py, after each of 8
half-iterations.  tests/golden/tdec_auto.npz and tdec_generic.npz pin the restatement at 12 and 2 sizes; the GPU sweep
(tests/test_tdec_sweep_gpu.py) compares the device with this oracle at all 188, so this is the link to the reference.
Also the pin of tests/golden/tdec8_sweep.npz (digests of the reference's 8-bit decoder at its 110 sizes) to the
reference as compiled here."""
import numpy as np
import pytest

import oracle
import tdec_inputs as TI
from golden_io import load

pytestmark = pytest.mark.skipif(not oracle.ref_available(), reason="oracle/_ref not built")


def test_window_decoder_matches_reference_at_every_window_size():
    ref = oracle.RefTdec()
    bad = []
    for K in TI.WINDOW_SIZES:
        want = TI.window_traces(K)
        for c in TI.CLASSES:
            _, tr = ref.run(TI.block(K, c)[2], K, TI.NHALF, trace=True)
            for h in range(TI.NHALF):
                if not np.array_equal(tr[h], want[c][h]):
                    bad.append((K, c, h + 1))
                    break
    assert not bad, (len(bad), bad[:20])


def test_generic_decoder_matches_reference_at_every_size():
    ref = oracle.RefTdec(generic=True)
    bad = []
    for K in TI.CB_SIZES:
        want = TI.generic_traces(K)
        for c in TI.CLASSES:
            buf = np.zeros(3 * (K + 32) + 12, np.int16)  # (the harness copies this many from the buffer it is given)
            buf[: 3 * K + 12] = TI.block(K, c)[1]
            _, tr = ref.run(buf, K, TI.NHALF, trace=True)
            for h in range(TI.NHALF):
                if not np.array_equal(tr[h], want[c][h]):
                    bad.append((K, c, h + 1))
                    break
    assert not bad, (len(bad), bad[:20])


def test_tdec8_sweep_digests_match_reference():
    """The inputs regenerated, the reference's 8-bit decoder run on them: the committed digests"""
    z = load("tdec8_sweep.npz")
    Ks, cls, dig = z["K"], z["cls"], z["digest"]
    assert dig.shape == (len(TI.SIZES8) * len(TI.CLASSES8), TI.NHALF, 16)
    bad, i = [], 0
    for K in TI.SIZES8:
        tr = TI.ref_tdec8_traces(K)
        for c in TI.CLASSES8:
            assert (int(Ks[i]), str(cls[i])) == (K, c)
            for h in range(TI.NHALF):
                if not np.array_equal(TI.digest(tr[c][h]), dig[i, h]):
                    bad.append((K, c, h + 1))
                    break
            i += 1
    assert not bad, (len(bad), bad[:20])
