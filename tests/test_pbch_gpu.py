"""GPU: the PBCH receiver (include/srsran_amd/pbch.h) against the restatement of srslte_pbch_decode in
tests/pbch_ref.py -- the real recording, synthetic frames for every port count / bandwidth / cell_id % 3, soft
combining and the history in SEQUENCE mode, degenerate inputs, a caller's stream and a fresh host thread."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

from oracle import ue_dl_chain as uc

import pbch_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MIB_BITS = "000010101001000000000000"
PAYLOAD = R.bits_of("011010101001000000110100")


class DevFrames:
    """Frames (grid, ce (ports, G), noise) uploaded as the jobs of a PBCH call."""

    def __init__(self, frames):
        from srsran_amd.tdec import DeviceBuffer
        from srsran_amd.ue_dl import ChestRes, DlSfJob
        n, G, nports = len(frames), frames[0][0].size, frames[0][1].shape[0]
        host = np.zeros((n, 1 + nports, G), np.complex64)
        for i, (g, ce, _nz) in enumerate(frames):
            host[i, 0], host[i, 1:] = g, ce
        self.buf = DeviceBuffer(host.nbytes).upload(host)
        self.jobs = []
        self.chest = (ChestRes * n)()
        for i in range(n):
            j = DlSfJob()
            j.tti = 0
            j.sf_symbols[0] = self.buf.ptr + (i * (1 + nports)) * G * 8
            for p in range(nports):
                j.ce[p][0] = self.buf.ptr + (i * (1 + nports) + 1 + p) * G * 8
            self.jobs.append(j)
            self.chest[i].noise_estimate = frames[i][2]

    def sub(self, lo, hi):
        from srsran_amd.ue_dl import ChestRes
        return self.jobs[lo:hi], (ChestRes * (hi - lo))(*[self.chest[i] for i in range(lo, hi)])


def _tuple(r):
    return (r.ret, r.nof_tx_ports, r.sfn_offset, "".join(map(str, r.bits())) if r.ret == 1 else None)


def _ref_tuple(t):
    return (t[0], t[1], t[2], "".join(map(str, t[3])) if t[0] == 1 else None)


# ------------------------------------------------------------------ 4. the real recording

@pytest.mark.parametrize("nof_ports", [0, 1])
def test_real_signal(nof_ports):
    """All ten subframes of the recording through UeDl.fft_estimate, then one INDEPENDENT PBCH batch: subframe 0 gives
    the known MIB, nothing passes in the other nine (as the restatement says), and the cell built from the MIB is the
    one tests/test_real_signal.py writes by hand."""
    from srsran_amd import lib
    from srsran_amd import pbch as B
    from srsran_amd import pdsch as P
    from srsran_amd.tdec import DeviceBuffer
    from srsran_amd.ue_dl import DlSfJob, UeDl, default_chest_cfg

    NPRB, CELL = 6, 1
    iq_all = np.fromfile(os.path.join(HERE, "golden", "signal_1.92M_amar.c64"), np.complex64)
    SF_LEN = 15 * uc.symbol_sz(NPRB)
    est = 4 if nof_ports == 0 else 1
    ue = UeDl(P.make_cell(NPRB, est, CELL), 1)
    G, n = 14 * 12 * NPRB, 10
    d_iq, d_grid, d_ce = DeviceBuffer(n * SF_LEN * 8), DeviceBuffer(n * G * 8), DeviceBuffer(n * est * G * 8)
    jobs = []
    for sf in range(n):
        iq = np.ascontiguousarray(iq_all[sf * SF_LEN:(sf + 1) * SF_LEN])
        lib().mi355_memcpy_h2d(d_iq.ptr + sf * SF_LEN * 8, iq.ctypes.data, iq.nbytes)
        j = DlSfJob()
        j.tti = sf
        j.in_buffer[0] = d_iq.ptr + sf * SF_LEN * 8
        j.sf_symbols[0] = d_grid.ptr + sf * G * 8
        for p in range(est):
            j.ce[p][0] = d_ce.ptr + (sf * est + p) * G * 8
        jobs.append(j)
    chest = ue.fft_estimate(jobs, default_chest_cfg())
    want = []
    for sf in range(n):
        grid = uc.ofdm_rx_sf(iq_all[sf * SF_LEN:(sf + 1) * SF_LEN], NPRB)[None, :]
        ce, res = uc.chest_estimate(grid, NPRB, est, CELL, sf)
        want.append(_ref_tuple(R.PbchRef(NPRB, CELL, nof_ports).decode(grid[0], ce, res["noise_estimate"])))
    assert want[0] == (1, 1, 0, MIB_BITS) and all(w[0] == 0 for w in want[1:])
    q = B.Pbch(P.make_cell(NPRB, nof_ports, CELL))
    got = [_tuple(r) for r in q.decode(jobs, chest, B.INDEPENDENT)]
    assert got == want
    res0 = q.decode(jobs[:1], chest, B.INDEPENDENT)[0]
    cell, sfn = B.mib_unpack(res0.bits())
    assert sfn == 656
    mine = P.make_cell(cell.nof_prb, res0.nof_tx_ports, CELL, phich_length=cell.phich_length,
                       phich_resources=cell.phich_resources)
    hand = P.make_cell(NPRB, 1, CELL, phich_resources=2)
    assert bytes(mine) == bytes(hand)
    q.close()
    ue.close()


# ------------------------------------------------------------------ 5. parity, synthetic

@pytest.mark.parametrize("cell_id", [300, 1, 503])
@pytest.mark.parametrize("nof_prb", [6, 15])
def test_parity_synthetic(nof_prb, cell_id):
    """Ports {1, 2, 4} x search-all / fixed: four frames (frame_idx 0..3, one of them noisy) decoded INDEPENDENTly
    equal the restatement's first-call results, and the LLRs of every hypothesis agree within 1e-5 max|ref| (the
    tolerance of the PDCCH LLR tests)."""
    from srsran_amd import pbch as B
    from srsran_amd import pdsch as P
    rng = np.random.default_rng(1000 * nof_prb + cell_id)
    for nof_ports in (1, 2, 4):
        for cfgp in (0, nof_ports):
            est = 4 if cfgp == 0 else cfgp
            frames = [R.synth_frame(nof_prb, cell_id, nof_ports, est, PAYLOAD, fi, 1.2 if fi == 2 else 0.3, rng)
                      for fi in range(4)]
            dev = DevFrames(frames)
            q = B.Pbch(P.make_cell(nof_prb, cfgp, cell_id))
            got = q.decode(dev.jobs, dev.chest, B.INDEPENDENT)
            for i, (g, ce, nz) in enumerate(frames):
                ref = R.PbchRef(nof_prb, cell_id, cfgp)
                want = _ref_tuple(ref.decode(g, ce, nz))
                assert _tuple(got[i]) == want, (nof_ports, cfgp, i)
                if i != 2:
                    assert want == (1, nof_ports, i, "".join(map(str, PAYLOAD)))
                for nant in ref.hyps:
                    if nant not in ref.last_llr:  # (the search stopped before this hypothesis)
                        l = ref.equalize(g, ce, nant, nz)
                    else:
                        l = ref.last_llr[nant]
                    d = np.abs(q.llr(i, nant) - l).max()
                    assert d <= 1e-5 * np.abs(l).max(), (nof_ports, cfgp, i, nant, d)
            q.close()


# ------------------------------------------------------------------ 6. soft combining and the history

# (tx ports, configured ports, sigma, seed): found by scanning sigma in {0.7 .. 2.5} x seeds 0..3 with the restatement on
# 6 PRB, cell id 2 -- four frames (frame_idx 0..3) where the first call fails and a later one succeeds only by combining:
#   (4, 0, 1.3, 1)  search-all, 4 ports: calls 1-3 fail, call 4 combines all four frames (nb 3, dst 0, src 0)
#   (4, 0, 1.1, 0)  search-all: call 2 combines two frames, reset, call 3 fails, call 4 combines again (dst 2)
#   (2, 2, 1.5, 0)  2 ports fixed: call 3 combines three frames
#   (2, 2, 1.8, 3)  2 ports fixed: call 4 combines frames 2-4 (nb 2, dst 1, src 1)
#   (1, 1, 2.5, 0)  1 port fixed: call 4 combines frames 3-4 (nb 1, dst 2, src 2)
SEQ_CASES = [(4, 0, 1.3, 1), (4, 0, 1.1, 0), (2, 2, 1.5, 0), (2, 2, 1.8, 3), (1, 1, 2.5, 0)]


def _sequence(nof_ports, cfgp, sigma, seed, nframes, signal=True):
    rng = np.random.default_rng(seed)
    return [R.synth_frame(6, 2, nof_ports, 4 if cfgp == 0 else cfgp, PAYLOAD, fi, sigma, rng, signal=signal)
            for fi in range(nframes)]


def _ref_sequence(frames, cfgp, reset_at=()):
    ref, out, hits = R.PbchRef(6, 2, cfgp), [], []
    for i, (g, ce, nz) in enumerate(frames):
        if i in reset_at:
            ref.reset()
        out.append(_ref_tuple(ref.decode(g, ce, nz)))
        hits.append(ref.last_hit)
    return out, hits


@pytest.mark.parametrize("case", SEQ_CASES)
def test_sequence_soft_combining(case):
    """Eight frames (frame_idx 0..7) in SEQUENCE mode: every job's result equals the restatement's -- the first
    success needs combining (a condition on the inputs, checked here), the history restarts after it and slides
    after four failures -- whether fed as one batch, as batches of one, or split 3 + 5 with the state carried; and a
    mi355_pbch_decode_reset in the middle matches the restatement's.

    Outcome of the CPU scan that chose SEQ_CASES (restatement, 6 PRB, cell id 2, (ret, ports, sfn_offset) per call
    and the (nant, nb, dst, src) of each hit):
      (4, 0, 1.3, 1): 0 0 0 (1,4,3) 0 0 (1,4,2) 0      hits (4,3,0,0), (4,1,1,1)
      (4, 0, 1.1, 0): 0 (1,4,1) 0 (1,4,3) 0 (1,4,1) 0 (1,4,3)   hits (4,1,0,0), (4,1,2,0), (4,0,1,1), (4,1,2,0)
      (2, 2, 1.5, 0): 0 0 (1,2,2) 0 0 0 0 (1,2,3)      hits (2,2,0,0), (2,1,2,2)
      (2, 2, 1.8, 3): 0 0 0 (1,2,3) 0 0 0 0            hit  (2,2,1,1)
      (1, 1, 2.5, 0): 0 0 0 (1,1,3) 0 0 0 0            hit  (1,1,2,2)
    At sigma 0.7 the first call already succeeds for every seed tried; at sigma >= 3 (1 port) nothing decodes in four
    frames."""
    from srsran_amd import pbch as B
    from srsran_amd import pdsch as P
    nof_ports, cfgp, sigma, seed = case
    frames = _sequence(nof_ports, cfgp, sigma, seed, 8)
    want, hits = _ref_sequence(frames, cfgp)
    first = next(i for i, w in enumerate(want) if w[0] == 1)
    assert want[0][0] == 0 and 1 <= first <= 3 and hits[first][1] >= 1, (want, hits)  # succeeds only by combining
    assert all(w[3] == "".join(map(str, PAYLOAD)) for w in want if w[0] == 1)
    dev = DevFrames(frames)
    q = B.Pbch(P.make_cell(6, cfgp, 2))
    n = len(frames)
    assert [_tuple(r) for r in q.decode(dev.jobs, dev.chest, B.SEQUENCE)] == want
    q.reset()
    assert [_tuple(q.decode(*dev.sub(i, i + 1), B.SEQUENCE)[0]) for i in range(n)] == want
    q.reset()
    got = [_tuple(r) for r in q.decode(*dev.sub(0, 3), B.SEQUENCE)]
    # an INDEPENDENT call in between neither reads nor writes the history
    assert _tuple(q.decode(*dev.sub(0, 1), B.INDEPENDENT)[0]) == want[0]
    got += [_tuple(r) for r in q.decode(*dev.sub(3, n), B.SEQUENCE)]
    assert got == want
    # reset in the middle (before frame 2, where the restatement's history holds two frames)
    want_r, _ = _ref_sequence(frames, cfgp, reset_at=(2,))
    q.reset()
    got = [_tuple(r) for r in q.decode(*dev.sub(0, 2), B.SEQUENCE)]
    q.reset()
    got += [_tuple(r) for r in q.decode(*dev.sub(2, n), B.SEQUENCE)]
    assert got == want_r
    q.close()


@pytest.mark.parametrize("cfgp", [0, 2])
def test_sequence_history_slides(cfgp):
    """Eight frames carrying CRS and noise but no PBCH, which the restatement never decodes: the history fills, then
    slides by one frame per call; every result is 0 in one batch, in batches of one and split 5 + 3."""
    from srsran_amd import pbch as B
    from srsran_amd import pdsch as P
    frames = _sequence(2, cfgp, 1.0, 100, 8, signal=False)
    want, _ = _ref_sequence(frames, cfgp)
    assert all(w[0] == 0 for w in want)
    dev = DevFrames(frames)
    q = B.Pbch(P.make_cell(6, cfgp, 2))
    assert [_tuple(r) for r in q.decode(dev.jobs, dev.chest, B.SEQUENCE)] == want
    q.reset()
    assert [_tuple(q.decode(*dev.sub(i, i + 1), B.SEQUENCE)[0]) for i in range(8)] == want
    q.reset()
    got = [_tuple(r) for r in q.decode(*dev.sub(0, 5), B.SEQUENCE)] + \
          [_tuple(r) for r in q.decode(*dev.sub(5, 8), B.SEQUENCE)]
    assert got == want
    q.close()


def test_sequence_slide_then_success():
    """Five noise-only frames (the history slides twice), then the (4, 0, 1.1, 0) frames: windows that mix old noise
    frames with the new ones are part of the search, so this compares the slid history's content, not only zeros."""
    from srsran_amd import pbch as B
    from srsran_amd import pdsch as P
    frames = _sequence(4, 0, 1.0, 101, 5, signal=False) + _sequence(4, 0, 1.1, 0, 6)
    want, _ = _ref_sequence(frames, 0)
    assert any(w[0] == 1 for w in want[5:])
    dev = DevFrames(frames)
    q = B.Pbch(P.make_cell(6, 0, 2))
    assert [_tuple(r) for r in q.decode(dev.jobs, dev.chest, B.SEQUENCE)] == want
    q.reset()
    got = []
    for lo, hi in ((0, 2), (2, 6), (6, 7), (7, 11)):
        got += [_tuple(r) for r in q.decode(*dev.sub(lo, hi), B.SEQUENCE)]
    assert got == want
    q.close()


# ------------------------------------------------------------------ 7. degenerate input

def test_degenerate_inputs():
    """An all-zero grid with non-zero estimates: every LLR is finite (zero), the quantiser's max = 1e-9 floor holds and
    the all-zero payload, whose CRC passes under the 1-port mask, is rejected -- in both modes.  A grid scaled by 1e4
    decodes to the same MIB: the quantiser normalises by the maximum."""
    from srsran_amd import pbch as B
    from srsran_amd import pdsch as P
    rng = np.random.default_rng(5)
    frames = [R.synth_frame(6, 1, 1, 4, PAYLOAD, fi, 0.3, rng) for fi in range(4)]
    zero = [(np.zeros_like(g), ce, nz) for (g, ce, nz) in frames]
    q = B.Pbch(P.make_cell(6, 0, 1))
    dz = DevFrames(zero)
    for mode in (B.INDEPENDENT, B.SEQUENCE):
        assert [_tuple(r) for r in q.decode(dz.jobs, dz.chest, mode)] == [(0, 0, 0, None)] * 4
        for i in range(4):
            for nant in (1, 2, 4):
                l = q.llr(i, nant)
                assert np.isfinite(l).all() and not l.any()
    ref = R.PbchRef(6, 1, 0)
    assert [ref.decode(*f)[0] for f in zero] == [0] * 4
    q.reset()
    big = [((g * np.float32(1e4)).astype(np.complex64), ce, nz) for (g, ce, nz) in frames]
    db = DevFrames(big)
    got = [_tuple(r) for r in q.decode(db.jobs, db.chest, B.INDEPENDENT)]
    assert got == [(1, 1, fi, "".join(map(str, PAYLOAD))) for fi in range(4)]
    assert got == [_ref_tuple(R.PbchRef(6, 1, 0).decode(*f)) for f in big]
    q.close()


def test_large_batch_after_small():
    """One job, then 1,400 (four frames tiled): the scratch and both stagings grow between the calls, and the
    descriptors (48 B per job) cross the staging's 64 KB limit for uploads in line on the caller's stream."""
    from srsran_amd import pbch as B
    from srsran_amd import pdsch as P
    from srsran_amd.ue_dl import ChestRes
    rng = np.random.default_rng(11)
    frames = [R.synth_frame(6, 0, 2, 4, PAYLOAD, fi, 0.4, rng) for fi in range(4)]
    want = [_ref_tuple(R.PbchRef(6, 0, 0).decode(*f)) for f in frames]
    dev = DevFrames(frames)
    q = B.Pbch(P.make_cell(6, 0, 0))
    assert _tuple(q.decode(*dev.sub(0, 1), B.INDEPENDENT)[0]) == want[0]
    n = 1400
    jobs = [dev.jobs[i % 4] for i in range(n)]
    chest = (ChestRes * n)(*[dev.chest[i % 4] for i in range(n)])
    got = q.decode(jobs, chest, B.INDEPENDENT)
    assert all(_tuple(got[i]) == want[i % 4] for i in range(n))
    assert np.array_equal(q.llr(n - 1, 4), q.llr(3, 4))
    q.close()


# ------------------------------------------------------------------ 8. device selection / stream

def test_callers_stream_and_fresh_thread():
    """A call on a caller's stream (here another object's non-blocking stream) returns the results of a call on the
    object's own stream, and the object works from a host thread that never selected a device."""
    from srsran_amd import lib
    from srsran_amd import pbch as B
    from srsran_amd import pdsch as P
    from srsran_amd.ue_dl import UeDl
    rng = np.random.default_rng(9)
    frames = [R.synth_frame(6, 2, 2, 4, PAYLOAD, fi, 0.4, rng) for fi in range(4)]
    want = [_ref_tuple(R.PbchRef(6, 2, 0).decode(*f)) for f in frames]
    dev = DevFrames(frames)
    q = B.Pbch(P.make_cell(6, 0, 2))
    ue = UeDl(P.make_cell(6, 1, 2), 1)
    got = [_tuple(r) for r in q.decode(dev.jobs, dev.chest, B.INDEPENDENT, stream=ue.stream())]
    assert lib().mi355_device_sync() == 0
    assert got == want
    out = {}

    def worker():
        out["res"] = [_tuple(r) for r in q.decode(dev.jobs, dev.chest, B.INDEPENDENT)]
        out["llr"] = q.llr(3, 2)

    t = threading.Thread(target=worker)
    t.start()
    t.join()
    assert out["res"] == want
    assert np.array_equal(out["llr"], q.llr(3, 2))
    q.close()
    ue.close()
