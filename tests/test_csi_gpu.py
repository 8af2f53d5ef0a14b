"""GPU: mi355_ue_dl_csi_batch (include/srsran_amd/csi.h) against the recorded reference answers of
tests/golden/csi_feedback.npz and the restatement in tests/csi_ref.py -- every fixture case at 6 PRB (40 of 64 lanes
and the cn-only tail samples), 15 PRB (a partial second pass) and 100 PRB, batches of 1, 5 and 67 subframes mixing
channels and noise values, the estimate-row mode behind mi355_ue_dl_decode_batch, a closed loop from generated
subframes to the reported PMI and rank, a caller's stream and a fresh thread, invalid inputs, the degenerate cases and
run-to-run identity.

Tolerances against the recorded reference (tests/csi_ref.tolerances; none derived from the GPU's output): sinr_1l
1e-5 mean ||H||_F^2 / noise, sinr_2l 1.5e-3 (ref + 2), cn 1e-3 dB, cn_count exact; the decisions exact unless the
recorded values lie within twice the tolerance of a tie or threshold (tests/csi_ref.excluded: 5 of the 118 cases)."""
import ctypes as C
import threading

import numpy as np
import pytest

import csi_ref as R

pytestmark = pytest.mark.gpu

CASES = R.load_cases()
BY_PRB = {prb: [c for c in CASES if c["nof_prb"] == prb] for prb in (6, 15, 100)}
DECISIONS = ("pmi_1l", "pmi_2l", "ri", "pmi", "ri_cn", "cqi")


def _cell(nof_prb, nof_ports=2, cell_id=5):
    from srsran_amd import pdsch as P
    return P.make_cell(nof_prb, nof_ports, cell_id)


class DevCases:
    """The estimates of a list of fixture cases in HBM (POISON between the samples) as the sfjobs / chest of a call."""

    def __init__(self, cases):
        from srsran_amd.tdec import DeviceBuffer
        from srsran_amd.ue_dl import ChestRes, DlSfJob
        n = len(cases)
        self.jobs, self.chest, self.keep = (DlSfJob * n)(), (ChestRes * n)(), {}
        for i, c in enumerate(cases):
            if id(c) not in self.keep:
                g = np.ascontiguousarray(R.grid_of(c))
                self.keep[id(c)] = (DeviceBuffer(g.nbytes).upload(g), g.shape[2] * 8)
            buf, stride = self.keep[id(c)]
            for p in range(2):
                for r in range(2):
                    self.jobs[i].ce[p][r] = buf.ptr + (2 * p + r) * stride
            self.chest[i].noise_estimate = float(c["noise"])


def _sums_ok(r, c, what):
    tol = R.tolerances(c)
    got = dict(sinr_1l=np.array(r.sinr_1l[:], np.float32), sinr_2l=np.array(r.sinr_2l[:], np.float32), cn=r.cn)
    for k in ("sinr_1l", "sinr_2l", "cn"):
        assert R.same_class(got[k], c[k], tol[k]), (what, c["name"], k, got[k], c[k], tol[k])
    assert r.cn_count == c["cn_count"], (what, c["name"], r.cn_count, c["cn_count"])


def _check(r, c, what=None):
    """one CsiRes against its own fixture case"""
    _sums_ok(r, c, what)
    ex = R.excluded(c)
    for k in DECISIONS:
        if k not in ex:
            assert getattr(r, k) == c[k], (what, c["name"], k, getattr(r, k), c[k])
    if not ex & {"ri", "pmi"}:
        assert R.same_class(r.sinr_db, c["sinr_db"], R.sinr_db_tol(c)), (what, c["name"], r.sinr_db, c["sinr_db"])


def _run(ue, cases, **kw):
    from srsran_amd import csi
    dev = DevCases(cases)
    offs = {float(c["offset"]) for c in cases}
    assert len(offs) == 1  # one SNR -> CQI offset per call
    return csi.csi_batch(ue, dev.jobs, dev.chest, offs.pop(), **kw)


def _by_offset(cases):
    out = {}
    for c in cases:
        out.setdefault(float(c["offset"]), []).append(c)
    return out


@pytest.mark.parametrize("nof_prb", [6, 15, 100])
def test_every_fixture_case(nof_prb):
    """Every recorded case of the bandwidth, all cases of one CQI offset in one call (6 PRB: 40 of 64 lanes carry SINR
    samples, lanes 40 and 41 the cn-only tail; 15 PRB: 104 + 1 samples, a second pass of 41 lanes; 100 PRB: 11
    passes), each result against its own case."""
    from srsran_amd.ue_dl import UeDl
    ue = UeDl(_cell(nof_prb), 2)
    seen = 0
    for off, cases in sorted(_by_offset(BY_PRB[nof_prb]).items()):
        res = _run(ue, cases)
        for i, c in enumerate(cases):
            _check(res[i], c, (nof_prb, off, i))
        seen += len(cases)
    assert seen == len(BY_PRB[nof_prb]) > 0
    ue.close()


@pytest.mark.parametrize("n", [1, 5, 67])
def test_batch_sizes_mix_channels_and_noise(n):
    """Batches of 1, 5 and 67 subframes (four per workgroup: partial last blocks) drawn from the 6 PRB cases of one
    offset in a stride that interleaves the constant, random, rank-1 and degenerate channels and their noise values;
    every result is its own case's -- a job or lane mix-up would not be."""
    from srsran_amd.ue_dl import UeDl
    pool = _by_offset(BY_PRB[6])[0.0]
    assert len(pool) > 40
    pick = [pool[(7 * i + n) % len(pool)] for i in range(n)]
    ue = UeDl(_cell(6), 2)
    res = _run(ue, pick)
    for i, c in enumerate(pick):
        _check(res[i], c, (n, i))
    ue.close()


def test_one_job_100_prb_and_five_at_15():
    from srsran_amd.ue_dl import UeDl
    for prb, n in ((100, 1), (15, 5)):
        pool = _by_offset(BY_PRB[prb])[0.0]
        pick = [pool[(3 * i + 1) % len(pool)] for i in range(n)]
        ue = UeDl(_cell(prb), 2)
        res = _run(ue, pick)
        for i, c in enumerate(pick):
            _check(res[i], c, (prb, i))
        ue.close()


def test_ce_rows_reads_row_zero_only():
    """mi355_ue_dl_set_ce_rows(1) on 15 PRB estimates whose rows 1..13 hold NaNs: sample j is read at j % 180 (180 is
    no multiple of 24, so the wrapped samples are other subcarriers of row 0) -- the restatement on row 0 tiled 14
    times, within the tolerances (exact divisions on both sides), and no NaN comes back."""
    from srsran_amd import csi
    from srsran_amd.tdec import DeviceBuffer
    from srsran_amd.ue_dl import CE_ROWS_FIRST, ChestRes, DlSfJob, UeDl
    nre, n = 12 * 15, 3
    rng = np.random.default_rng(77)
    jobs, chest, keep, refs = (DlSfJob * n)(), (ChestRes * n)(), [], []
    for i in range(n):
        row = ((rng.standard_normal((2, 2, 1)) + 1j * rng.standard_normal((2, 2, 1))) +
               0.3 * (rng.standard_normal((2, 2, nre)) + 1j * rng.standard_normal((2, 2, nre)))).astype(np.complex64)
        g = np.full((2, 2, 14 * nre), np.nan + 1j * np.nan, np.complex64)
        g[:, :, :nre] = row
        buf = DeviceBuffer(g.nbytes).upload(np.ascontiguousarray(g))
        keep.append(buf)
        for p in range(2):
            for r in range(2):
                jobs[i].ce[p][r] = buf.ptr + (2 * p + r) * 14 * nre * 8
        chest[i].noise_estimate = 0.02 * (i + 1)
        samples = np.tile(row, (1, 1, 14))[:, :, ::R.STEP]
        s = R.sums(samples, 15, chest[i].noise_estimate)
        refs.append(dict(name=f"row0_{i}", nof_prb=15, noise=np.float32(chest[i].noise_estimate), samples=samples, **s))
    assert nre % R.STEP != 0
    ue = UeDl(_cell(15), 2)
    ue.set_ce_rows(CE_ROWS_FIRST)
    res = csi.csi_batch(ue, jobs, chest, 0.0)
    for i in range(n):
        _sums_ok(res[i], refs[i], "row0")
    ue.close()


def _tm4_source(cell, nsf, H, snr_db, seed):
    from srsran_amd import synth
    plans = synth.phy_dl_test_plans(cell, 3, 7, False, nof_subframes=nsf)
    nbytes = max(max(synth.tb_bytes(p.cfg)) for p in plans)
    src = synth.DlSource(cell, 2, nsf, nbytes, H=H)
    src.generate(0, plans, snr_db, seed)
    return src, nbytes


def test_ce_rows_behind_decode_batch():
    """Estimates written by mi355_ue_dl_decode_batch (AVERAGE estimator, 6 PRB, TM4 subframes from the eNB generator
    through a flat 2x2 channel) under set_ce_rows(1) -- rows 1..13 keep a NaN pattern -- and under the default: the two
    feedback results are equal byte for byte, and both are the restatement's on the downloaded row 0 within the
    tolerances (exact divisions on both sides; the sums differ in order only)."""
    from srsran_amd import csi, lib, synth
    cell = _cell(6, 2, 1)
    B = 3
    H = np.array([[0.9 + 0.2j, -0.3 + 0.6j], [0.4 - 0.7j, 0.8 + 0.1j]], np.complex64)
    src, nbytes = _tm4_source(cell, B, H, 25.0, 11)
    outs = []
    for rows in (0, 1):
        rx = synth.DlReceiver(cell, 2, B, nbytes, ce_rows=rows)
        lib().mi355_memset_dev(rx.d_ce.ptr, 0xFF, rx.d_ce.nbytes)
        bound = rx.bind(src, 0, B)
        rx.step(bound)
        res = csi.csi_batch(rx.ue, bound[0], rx.chest, 0.0)
        ce = rx.d_ce.download(np.zeros(rx.d_ce.nbytes // 8, np.complex64)).reshape(B, 2, 2, 14, 72)
        noise = [rx.chest[k].noise_estimate for k in range(B)]
        outs.append((bytes(res), ce, noise, [res[k] for k in range(B)]))
        rx.close()
    src.close()
    assert outs[0][0] == outs[1][0]
    assert np.isnan(outs[1][1][:, :, :, 1:].view(np.float32)).all() and outs[0][2] == outs[1][2]
    _raw, ce, noise, res = outs[1]
    for k in range(B):
        samples = np.tile(ce[k, :, :, 0], (1, 1, 14))[:, :, ::R.STEP]
        s = R.sums(samples, 6, noise[k])
        ref = dict(name=f"sf{k}", nof_prb=6, noise=np.float32(noise[k]), offset=np.float32(0), samples=samples, **s)
        _sums_ok(res[k], ref, ("decode_batch", k))


def test_closed_loop_pmi_and_rank():
    """6 PRB TM4 subframes from the eNB generator through four flat rank-1 channels H = u w_i^H matched to the
    codebook vectors w_i = (1, {1, -1, j, -j}) / sqrt 2, at 12 dB: after OFDM and estimation the reported pmi_1l is i
    and ri = 0 (the 2-layer SINR stays below 20 dB and below the 1-layer one).  Through the scaled unitary channel
    [[1, 1], [1, -1]] at 35 dB: ri = 1, and the condition number reports rank 2 as well."""
    from srsran_amd import csi, synth
    from srsran_amd.ue_dl import default_chest_cfg
    cell = _cell(6, 2, 1)
    u = np.array([1.0, 1.0j], np.complex64)
    chans = [(np.outer(u, np.conj(np.array([1, w2]) / np.sqrt(2))), 12.0) for w2 in (1, -1, 1j, -1j)]
    chans.append((np.array([[1, 1], [1, -1]], np.complex64), 35.0))
    got = []
    for k, (H, snr) in enumerate(chans):
        src, nbytes = _tm4_source(cell, 2, H, snr, 20 + k)
        rx = synth.DlReceiver(cell, 2, 2, nbytes)
        jobs = rx.bind(src, 0, 2)[0]
        chest = rx.ue.fft_estimate(list(jobs), default_chest_cfg())
        res = csi.csi_batch(rx.ue, jobs, chest, 0.0)
        got.append([(r.pmi_1l, r.ri, r.ri_cn, r.cn, r.sinr_db) for r in (res[0], res[1])])
        rx.close()
        src.close()
    for i in range(4):
        for (pmi_1l, ri, _ri_cn, _cn, _db) in got[i]:
            assert (pmi_1l, ri) == (i, 0), (i, got[i])
    for (_p, ri, ri_cn, cn, db) in got[4]:
        assert ri == 1 and ri_cn == 1 and cn < 3.0 and db > 20.0, got[4]


def test_callers_stream_and_fresh_thread():
    """A call on a caller's stream (another object's non-blocking stream) and a call from a host thread that never
    selected a device return what a call on the object's own stream returns."""
    from srsran_amd import csi, lib
    from srsran_amd.ue_dl import UeDl
    cases = _by_offset(BY_PRB[6])[0.0][:9]
    dev = DevCases(cases)
    ue, other = UeDl(_cell(6), 2), UeDl(_cell(6), 2)
    want = bytes(csi.csi_batch(ue, dev.jobs, dev.chest, 0.0))
    got = csi.csi_batch(ue, dev.jobs, dev.chest, 0.0, stream=other.stream())
    assert lib().mi355_device_sync() == 0
    assert bytes(got) == want
    out = {}

    def worker():
        out["res"] = bytes(csi.csi_batch(ue, dev.jobs, dev.chest, 0.0))

    t = threading.Thread(target=worker)
    t.start()
    t.join()
    assert out["res"] == want
    for i, c in enumerate(cases):
        _check(got[i], c, ("stream", i))
    ue.close()
    other.close()


def test_invalid_inputs():
    """A 1-port or 1-rx object returns MI355_ERROR_INVALID_INPUTS (the reference computes the three quantities for
    2x2 only); so does a 2x2 object of an extended-CP cell, whose 12-symbol grids the 14-symbol sample counts would
    overrun (the grids given here are 14 symbols long, so even a call that went ahead would stay inside them, and the
    results stay untouched); so do null arrays and a null estimate pointer; nsf = 0 returns 0 without reading anything."""
    from srsran_amd import csi
    from srsran_amd import pdsch as P
    from srsran_amd.ue_dl import UeDl
    cases = _by_offset(BY_PRB[6])[0.0][:2]
    dev = DevCases(cases)
    L = csi._declare()
    for ports, nrx in ((1, 2), (2, 1), (1, 1), (4, 2)):
        ue = UeDl(_cell(6, ports), nrx)
        rc, _res = csi.csi_batch(ue, dev.jobs, dev.chest, 0.0, check_rc=False)
        assert rc == csi.ERROR_INVALID_INPUTS, (ports, nrx, rc)
        ue.close()
    ue = UeDl(P.make_cell(6, 2, 5, cp=1), 2)  # MI355_CP_EXT
    rc, res = csi.csi_batch(ue, dev.jobs, dev.chest, 0.0, check_rc=False)
    assert rc == csi.ERROR_INVALID_INPUTS and bytes(res) == bytes(len(bytes(res)))
    assert L.mi355_ue_dl_csi_batch(ue.h, None, None, 0, 0.0, None, None) == csi.ERROR_INVALID_INPUTS
    ue.close()
    ue = UeDl(_cell(6), 2)
    assert L.mi355_ue_dl_csi_batch(ue.h, None, None, 0, 0.0, None, None) == 0
    assert L.mi355_ue_dl_csi_batch(None, dev.jobs, dev.chest, 2, 0.0, (csi.CsiRes * 2)(), None) == csi.ERROR_INVALID_INPUTS
    assert L.mi355_ue_dl_csi_batch(ue.h, dev.jobs, dev.chest, 2, 0.0, None, None) == csi.ERROR_INVALID_INPUTS
    dev.jobs[1].ce[1][0] = None
    rc, _res = csi.csi_batch(ue, dev.jobs, dev.chest, 0.0, check_rc=False)
    assert rc == csi.ERROR_INVALID_INPUTS
    ue.close()


def test_degenerate_cases():
    """All-zero estimates with zero noise (the noise bound 1e-9 acts: sinr_1l = 0, sinr_2l ~ 2e8 from the clamped
    determinant, cn = -inf) and a NaN in one sampled estimate (every SINR NaN, that sample left out of cn): the
    results are in the recorded class -- NaN for NaN, infinities by sign -- beside a sound job that is untouched."""
    from srsran_amd.ue_dl import UeDl
    pool = _by_offset(BY_PRB[6])[0.0]
    zero = next(c for c in pool if c["name"] == "all_zero")
    nan = next(c for c in pool if c["name"] == "nan_sample")
    sound = next(c for c in pool if c["name"] == "gold3")
    assert np.isneginf(zero["cn"]) and np.isnan(nan["sinr_1l"]).all() and np.isnan(nan["sinr_2l"]).all()
    ue = UeDl(_cell(6), 2)
    res = _run(ue, [zero, sound, nan, sound])
    assert np.isneginf(res[0].cn) and res[0].cn_count == 42 and res[0].sinr_1l[:] == [0.0] * 4
    assert (res[0].ri, res[0].ri_cn, res[0].cqi) == (1, 1, 15)
    assert np.isnan(np.array(res[2].sinr_1l[:])).all() and np.isnan(np.array(res[2].sinr_2l[:])).all()
    assert res[2].cn_count == 41 and np.isfinite(res[2].cn)
    assert (res[2].pmi_1l, res[2].pmi_2l, res[2].ri, res[2].pmi, res[2].cqi) == (0, 0, 0, 0, 0) and np.isneginf(res[2].sinr_db)
    for i, c in enumerate((zero, sound, nan, sound)):
        _check(res[i], c, ("degenerate", i))
    assert bytes(res[1]) == bytes(res[3])
    ue.close()


def test_two_identical_calls_are_bit_identical():
    """The wave reduction is a fixed shuffle tree: the same call twice, and the same subframe at two places of a
    batch, give the same bytes (NaNs included)."""
    from srsran_amd import csi
    from srsran_amd.ue_dl import UeDl
    pool = _by_offset(BY_PRB[15])[0.0]
    cases = (pool + pool)[:2 * len(pool) - 1]
    dev = DevCases(cases)
    ue = UeDl(_cell(15), 2)
    a = csi.csi_batch(ue, dev.jobs, dev.chest, 0.0)
    b = csi.csi_batch(ue, dev.jobs, dev.chest, 0.0)
    assert bytes(a) == bytes(b)
    n = len(pool)
    for i in range(n - 1):
        assert bytes(a[i]) == bytes(a[n + i]), i
    assert C.sizeof(a) == 60 * len(cases)
    ue.close()
