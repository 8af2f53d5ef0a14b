"""GPU: cell search (include/srsran_amd/sync.h) against the float64 restatement of srslte_sync_find in
tests/sync_ref.py -- the real recording, synthetic frames over cell ids / CP / frame type / CFO / SSS algorithm, peaks
on tile and window edges, short windows, SEQUENCE mode and its state, degenerate inputs, a caller's stream and a fresh
host thread, and acquisition end to end: I/Q -> cell id and timing -> MIB.

Decision fields are compared exactly and float fields within the tolerances of sync_ref.py (four times the compiled
reference's measured deviation from the restatement).  A result whose restatement has a decision inside the tolerance
band (sync_ref.safe) is compared on peak_abs alone; at most 5 % of the results of a comparison may be of that kind.
The recording is also compared with the compiled reference's own results in tests/golden/sync_find.npz."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import sync_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RECORDING = os.path.join(HERE, "golden", "signal_1.92M_amar.c64")


class DevIq:
    """frames (complex64 arrays) resident in HBM, 1024 zero samples behind each"""

    def __init__(self, frames):
        from srsran_amd.tdec import DeviceBuffer
        self.frames = [np.ascontiguousarray(f, np.complex64) for f in frames]
        offs = np.cumsum([0] + [f.size + 1024 for f in self.frames])
        host = np.zeros(int(offs[-1]), np.complex64)
        for f, o in zip(self.frames, offs):
            host[o:o + f.size] = f
        self.buf = DeviceBuffer(host.nbytes).upload(host)
        self.ptrs = [self.buf.ptr + int(o) * 8 for o in offs[:-1]]


def _hyps(cfg):
    return (0, 1, 2) if cfg.get("n_id_2", 3) == 3 else (cfg["n_id_2"],)


def _ref_objs(cfg):
    kw = {k: v for k, v in cfg.items() if k != "n_id_2"}
    return [R.SyncRef(n_id_2=h, **kw) for h in _hyps(cfg)]


def gpu_find(cfg, dev, offs=0, mode=0, q=None, stream=None):
    from srsran_amd import sync as S
    own = q is None
    if own:
        q = S.Sync(S.sync_cfg(**cfg))
    res = q.find(dev.ptrs, offs, mode, stream)
    if own:
        q.close()
    return [[r.as_dict() for r in job] for job in res]


def ref_find(cfg, dev, offs=0, seq=False, objs=None):
    n = len(dev.frames)
    offs = [offs] * n if isinstance(offs, int) else offs
    objs = objs or _ref_objs(cfg)
    out = []
    for f, o in zip(dev.frames, offs):
        x = np.concatenate([f, np.zeros(1024, np.complex64)])
        row = []
        for q in objs:
            if not seq:
                q.reset()
            row.append(q.find(x, o))
        out.append(row)
    return out


def check(got, want, what=""):
    """compare every result; one whose restatement is not safe() is compared on peak_abs alone and counted: at most
    5 % of the results of this comparison"""
    unsafe, total = 0, 0
    for i, (gj, wj) in enumerate(zip(got, want)):
        for g, w in zip(gj, wj):
            total += 1
            tag = f"{what} job {i} n_id_2 {w['n_id_2']}"
            if R.safe(w):
                R.compare(g, w, tag)
            else:
                unsafe += 1
                print(f"{tag}: a decision inside the tolerance band, margins {w['margin']}")
                for f in ("peak_abs",):
                    assert abs(g[f] - w[f]) <= R.TOL[f][0] * abs(w[f]), (tag, f, g[f], w[f])
    assert len(got) == len(want) and unsafe <= 0.05 * total, (what, unsafe, total)
    return unsafe


def lib_put(cell_id, cp, nof_prb=6):
    """the generator's opt-in helper as synth_frame's put callback"""
    from srsran_amd import enb_dl as E
    from srsran_amd import pdsch as P
    cell = P.make_cell(nof_prb, 1, cell_id, cp=cp)
    return lambda grids, sf_idx: E.put_sync(cell, sf_idx, grids)


def pss_end(cp, ft, lead, M=128):
    nsymb = 7 if cp == R.CP_NORM else 6
    sym = M + R.cp_sz(M, cp)
    first = R.cp_len(M, 160) if cp == R.CP_NORM else R.cp_len(M, 512)
    k = (nsymb - 1) if ft == R.FDD else (2 * nsymb + 2)
    return lead + (k // nsymb) * (15 * M // 2) + first + (k % nsymb) * sym + M


# ------------------------------------------------------------------ 1. the recording

def test_recording():
    """Both 5 ms halves, all three hypotheses, threshold 2.0, INDEPENDENT and as one 2-job SEQUENCE: N_id_2 = 1 is
    FOUND with cell id 1, subframes 0 and 5, normal CP, FDD; every field of every hypothesis is the restatement's."""
    iq = np.fromfile(RECORDING, np.complex64)
    dev = DevIq([iq[:9600 + 128], iq[9600:19200 + 128]])
    cfg = dict(fft_size=128, max_offset=9600, threshold=2.0, cfo_pss_enable=True)
    for seq in (False, True):
        got = gpu_find(cfg, dev, mode=int(seq))
        want = ref_find(cfg, dev, seq=seq)
        for half, sf in ((0, 0), (1, 5)):
            g = got[half][1]
            assert (g["ret"], g["peak_pos"], g["cell_id"], g["sf_idx"], g["cp"], g["frame_type"]) == \
                (R.FOUND, 960, 1, sf, R.CP_NORM, R.FDD)
            assert R.safe(want[half][1])
        check(got, want, f"recording seq={seq}")


def test_recording_against_fixture():
    """The 2-job SEQUENCE over the recording's halves against the compiled reference's own results
    (tests/golden/sync_find.npz, cases 0 .. 2: one reference object per N_id_2, threshold 2.0): N_id_2 = 1 FOUND with
    cell id 1 and subframes 0 / 5, the other two hypotheses what the fixture says, every field within the tolerances.
    m0, m1, N_id_1 and their values are compared where the SSS was detected (the reference leaves the previous call's
    or an uninitialised N_id_1 otherwise, this stage the reset values)."""
    import json
    z = np.load(os.path.join(HERE, "golden", "sync_find.npz"))
    meta = json.loads(str(z["meta"]))
    ivf, fvf = [str(f) for f in z["iv_fields"]], [str(f) for f in z["fv_fields"]]
    iq = np.fromfile(RECORDING, np.complex64)
    dev = DevIq([iq[:9600 + 128], iq[9600:19200 + 128]])
    cfg = dict(fft_size=128, max_offset=9600, threshold=2.0, cfo_pss_enable=True)
    got = gpu_find(cfg, dev, mode=1)
    seen = 0
    for i, m in enumerate(meta):
        if m["case"] > 2:
            continue
        assert m["src"]["kind"] == "recording" and m["cfg"]["n_id_2"] == m["case"] and m["cfg"]["threshold"] == 2.0
        half = m["src"]["start"] // 9600
        ref = dict(zip(ivf, (int(v) for v in z["iv"][i])))
        ref.update(zip(fvf, (float(v) for v in z["fv"][i])))
        g = dict(got[half][m["case"]])
        if m["case"] == 1:
            assert (ref["ret"], ref["cell_id"], ref["sf_idx"]) == (R.FOUND, 1, 5 * half)
        if not ref["sss_detected"]:
            for f in ("m0", "m1", "n_id_1", "cell_id", "m0_value", "m1_value"):
                ref[f] = g[f]
        if not ref["sss_available"]:
            ref["sss_corr"] = g["sss_corr"]
        assert m["safe"], m
        R.compare(g, ref, f"fixture n_id_2 {m['case']} half {half}")
        seen += 1
    assert seen == 6


# ------------------------------------------------------------------ 2. synthetic frames

CELLS = [(0, 0), (4, 5), (89, 0), (90, 5), (502, 0), (503, 5)]  # N_id_1 0, 1, 29, 30, 167, 167 over all N_id_2


@pytest.mark.parametrize("cp", [R.CP_NORM, R.CP_EXT])
@pytest.mark.parametrize("alg", [R.FULL, R.PARTIAL_3, R.DIFF])
def test_synthetic_cells(cp, alg):
    """Cell ids over all three N_id_2 and N_id_1 in {0, 1, 29, 30, 167}, subframes 0 and 5, the CP given and detected
    (no CFO), every SSS algorithm, at 20 dB and 3 dB: one 12-job batch with all hypotheses.  The frames come from the
    generator's put_sync helper.  The matching hypothesis acquires the cell at 20 dB."""
    frames, truth = [], []
    for k, (cid, sf) in enumerate(CELLS):
        for snr in (20.0, 3.0):
            lead = 300 + 211 * k
            frames.append(R.synth_frame(cid, sf, cp, lead=lead, snr_db=snr, seed=100 * cp + k, put=lib_put(cid, cp)))
            truth.append((cid, sf, pss_end(cp, R.FDD, lead), snr))
    dev = DevIq(frames)
    cfg = dict(fft_size=128, max_offset=9600, threshold=2.0, sss_alg=alg, cp=cp)
    got, want = gpu_find(cfg, dev), ref_find(cfg, dev)
    for g, (cid, sf, pos, snr) in zip(got, truth):
        if snr == 20.0:
            h = g[cid % 3]
            assert (h["ret"], h["peak_pos"], h["cell_id"], h["sf_idx"], h["cp"], h["frame_type"]) == \
                (R.FOUND, pos, cid, sf, cp, R.FDD), (cid, h)
    check(got, want, f"cells cp={cp} alg={alg}")


@pytest.mark.parametrize("filt", [False, True])
@pytest.mark.parametrize("cfo_en", [False, True])
def test_synthetic_cfo_and_tdd(cfo_en, filt):
    """A CFO of +-0.3 subcarriers with the PSS-based estimate and the PSS filter on and off (the CP given: its metric
    needs the CP-based correction, which is out of scope), FDD and a TDD placement built in numpy, both CPs."""
    frames, truth, cps = [], [], []
    for cp in (R.CP_NORM, R.CP_EXT):
        for ft in (R.FDD, R.TDD):
            for k, (cid, sf) in enumerate(CELLS[:4]):
                cfo = 0.3 if k % 2 else -0.3
                frames.append(R.synth_frame(cid, sf, cp, ft, lead=500 + 97 * k, cfo=cfo, snr_db=15.0, seed=7 * k + ft))
                truth.append((cid, sf, ft, cfo))
                cps.append(cp)
    for cp in (R.CP_NORM, R.CP_EXT):
        sel = [i for i in range(len(frames)) if cps[i] == cp]
        dev = DevIq([frames[i] for i in sel])
        cfg = dict(fft_size=128, max_offset=9600, threshold=2.0, cfo_pss_enable=cfo_en, pss_filt_enable=filt,
                   detect_cp=False, cp=cp)
        got, want = gpu_find(cfg, dev), ref_find(cfg, dev)
        if cfo_en:
            for g, i in zip(got, sel):
                cid, sf, ft, cfo = truth[i]
                h = g[cid % 3]
                assert (h["ret"], h["cell_id"], h["frame_type"], h["sf_idx"]) == (R.FOUND, cid, ft, sf + ft), (cid, h)
                assert abs(h["cfo_pss"] - cfo) < 0.05
        check(got, want, f"cfo en={cfo_en} filt={filt} cp={cp}")


# ------------------------------------------------------------------ 3. tile and window edges

def test_tile_edges_find_offset_nospace():
    """The peak on the first and on the last output of a 256-output tile, on the last output whose window lies wholly
    inside the search window (max_offset), inside the partial-overlap tail behind it, the same frames read through
    find_offset != 0, and a peak too early for the SSS: FOUND_NOSPACE with the SSS fields at their reset values.
    This departs from the issue's list: in the long form output 0 is a single tap and output max_offset + fft - 3 two
    taps of the window, so no PSS can peak there; the first and the last valid output carry a peak only in the
    short-window form (test_short_window, outputs 0 and 30)."""
    cid = 301
    base = pss_end(R.CP_NORM, R.FDD, 0)  # 960
    leads = [1024 - base, 1279 - base, 2048 + 255 - base, 9600 - base, 9600 + 40 - base]
    frames = [R.synth_frame(cid, 0, lead=l, seed=i, tail=700) for i, l in enumerate(leads)]
    early = R.synth_frame(cid, 0, lead=0, seed=9)[base - 200:]  # the PSS ends at sample 200 < 2 (128 + 32)
    dev = DevIq(frames + [early])
    cfg = dict(fft_size=128, max_offset=9600, n_id_2=cid % 3, threshold=2.0, cfo_pss_enable=True)
    got, want = gpu_find(cfg, dev), ref_find(cfg, dev)
    assert [g[0]["peak_pos"] for g in got] == [1024, 1279, 2303, 9600, 9640, 200]
    assert [g[0]["ret"] for g in got] == [R.FOUND] * 5 + [R.FOUND_NOSPACE]
    e = got[5][0]
    assert (e["sss_available"], e["sss_detected"], e["m0"], e["m1"], e["n_id_1"], e["cell_id"], e["sss_corr"]) == \
        (0, 0, 0, 0, R.N_ID_1_NONE, -1, 0.0)
    check(got, want, "edges")
    offs = [0, 77, 256, 300, 1, 0]
    got, want = gpu_find(cfg, dev, offs), ref_find(cfg, dev, offs)
    assert [g[0]["peak_pos"] for g in got[:4]] == [1024, 1279 - 77, 2303 - 256, 9300]
    assert got[1][0]["cell_id"] == cid
    check(got, want, "find_offset")


# ------------------------------------------------------------------ 4. short windows

def test_short_window():
    """max_offset 32 with fft 128: the sliding dot product of pss.c:491-496, whose position adds fft_size; the PSS
    symbol starts on the first output, in the middle and on the last valid output (30) of the window; find_offset
    leaves room for the SSS in front."""
    cid = 151
    start = pss_end(R.CP_NORM, R.FDD, 0) - 128
    frames = [R.synth_frame(cid, 5, lead=0, seed=i) for i in range(3)]
    dev = DevIq(frames)
    offs = [start, start - 17, start - 30]
    # threshold 0 accepts every peak (a peak on the first outputs has itself as its left side lobe: PSR <= 1)
    cfg = dict(fft_size=128, max_offset=32, n_id_2=cid % 3, threshold=0.0, cfo_pss_enable=True)
    got, want = gpu_find(cfg, dev, offs), ref_find(cfg, dev, offs)
    assert [g[0]["peak_pos"] for g in got] == [128, 145, 158]
    assert all(g[0]["ret"] == R.FOUND and g[0]["cell_id"] == cid and g[0]["sf_idx"] == 5 for g in got)
    check(got, want, "short")
    cfg["threshold"] = 1.2
    got, want = gpu_find(cfg, dev, offs), ref_find(cfg, dev, offs)
    assert got[0][0]["ret"] == R.NOFOUND and got[0][0]["peak_value"] <= 1.0
    check(got, want, "short psr")


def test_fft256_window512():
    """fft 256 (15 PRB) with max_offset 512: the tap loop runs over two LDS replicas of 128 taps, three tiles."""
    cid = 77
    end = pss_end(R.CP_NORM, R.FDD, 0, 256)
    frames = [R.synth_frame(cid, 0, nof_prb=15, lead=0, seed=i, nsf=1) for i in range(3)]
    dev = DevIq(frames)
    offs = [end - 256, end - 400, end - 511]
    cfg = dict(fft_size=256, max_offset=512, threshold=2.0, cfo_pss_enable=True, pss_filt_enable=True)
    got, want = gpu_find(cfg, dev, offs), ref_find(cfg, dev, offs)
    assert [g[cid % 3]["peak_pos"] for g in got] == [256, 400, 511]
    assert all(g[cid % 3]["cell_id"] == cid for g in got)
    check(got, want, "fft256")


# ------------------------------------------------------------------ 5. SEQUENCE

def _raw(q, dev, lo, hi, mode):
    from srsran_amd import sync as S
    res = q.find(dev.ptrs[lo:hi], 0, mode)
    return [bytes(r) for job in res for r in job]


@pytest.mark.parametrize("alpha", [0.2, 1.0])
def test_sequence_equals_the_parts(alpha):
    """Eight frames of one extended-CP cell on a normal-CP object (the CP is detected on the way), with a frame whose
    CFO estimate exceeds 7 kHz in the middle: one 8-job SEQUENCE batch is bit-equal to 8 batches of 1 and to 3 + 5;
    mi355_sync_reset in between restores the first run; the restatement agrees, its cfo_pss_mean unmoved by the
    7 kHz frame."""
    from srsran_amd import sync as S
    cid = 200
    cfos = [0.1, 0.12, 0.08, 0.1, 0.5, 0.1, 0.11, 0.09]
    frames = [R.synth_frame(cid, 5 * (i % 2), R.CP_EXT, lead=400, cfo=c, snr_db=12.0, seed=40 + i)
              for i, c in enumerate(cfos)]
    dev = DevIq(frames)
    cfg = dict(fft_size=128, max_offset=9600, threshold=1.25, ema_alpha=alpha, cfo_pss_enable=True)
    q = S.Sync(S.sync_cfg(**cfg))
    whole = _raw(q, dev, 0, 8, S.SEQUENCE)
    q.reset()
    ones = sum((_raw(q, dev, i, i + 1, S.SEQUENCE) for i in range(8)), [])
    q.reset()
    split = _raw(q, dev, 0, 3, S.SEQUENCE) + _raw(q, dev, 3, 8, S.SEQUENCE)
    assert whole == ones and whole == split
    indep = _raw(q, dev, 0, 8, S.INDEPENDENT)  # neither reads nor writes the state
    assert indep[:3] == whole[:3]
    q.reset()
    got = gpu_find(cfg, dev, mode=S.SEQUENCE, q=q)
    assert [bytes(S.SyncRes(**r)) for g in got for r in g] == whole
    q.close()
    want = ref_find(cfg, dev, seq=True)
    h = cid % 3
    assert abs(want[4][h]["cfo_pss"]) * 15000 > 7000 and want[4][h]["cfo_pss_mean"] == want[3][h]["cfo_pss_mean"]
    assert got[4][h]["cfo_pss_mean"] == got[3][h]["cfo_pss_mean"] != got[5][h]["cfo_pss_mean"]
    assert got[7][h]["cp"] == R.CP_EXT and got[7][h]["cell_id"] == cid
    check(got, want, f"sequence alpha={alpha}")


# ------------------------------------------------------------------ 6. degenerate inputs

def test_degenerate_inputs():
    """An all-zero frame: NOFOUND under a positive threshold (the PSR is 0 / 0), only ret is compared.  Pure noise stays
    under the threshold.  njobs = 0 is a success that touches nothing.  Every flag of the out-of-scope list is refused
    at create, so nothing is ever launched for it."""
    from srsran_amd import sync as S
    rng = np.random.default_rng(3)
    noise = (rng.standard_normal(9728) + 1j * rng.standard_normal(9728)).astype(np.complex64)
    dev = DevIq([np.zeros(9728, np.complex64), noise])
    cfg = dict(fft_size=128, max_offset=9600, threshold=3.0)
    for mode in (S.INDEPENDENT, S.SEQUENCE):
        got = gpu_find(cfg, dev, mode=mode)
        assert [h["ret"] for h in got[0]] == [R.NOFOUND] * 3
        assert [h["ret"] for h in got[1]] == [R.NOFOUND] * 3
    want = ref_find(cfg, dev)
    check(got[1:], want[1:], "noise")
    q = S.Sync(S.sync_cfg(**cfg))
    assert q.find([], 0) == []
    q.close()
    for bit in (S.CFO_I_ENABLE, S.CFO_CP_ENABLE, S.DECIMATE, S.KNOWN_N_ID_1, S.SSS_CHANNEL_EQUALIZE):
        with pytest.raises(RuntimeError):
            S.Sync(S.sync_cfg(unsupported=bit))
    for bad in (dict(fft_size=100), dict(fft_size=4096), dict(n_id_2=4), dict(sss_alg=3)):
        with pytest.raises(RuntimeError):
            S.Sync(S.sync_cfg(**bad))


# ------------------------------------------------------------------ 7. device selection / stream

def test_callers_stream_and_fresh_thread():
    """A call on a caller's stream returns the results of a call on the object's own stream, and the object works from
    a host thread that never selected a device."""
    from srsran_amd import lib
    from srsran_amd import pdsch as P
    from srsran_amd import sync as S
    from srsran_amd.ue_dl import UeDl
    dev = DevIq([R.synth_frame(33, 0, lead=100 * i, seed=i) for i in range(4)])
    cfg = dict(fft_size=128, max_offset=9600, cfo_pss_enable=True)
    q = S.Sync(S.sync_cfg(**cfg))
    want = _raw(q, dev, 0, 4, S.INDEPENDENT)
    ue = UeDl(P.make_cell(6, 1, 2), 1)
    res = q.find(dev.ptrs, 0, S.INDEPENDENT, stream=ue.stream())
    assert lib().mi355_device_sync() == 0
    assert [bytes(r) for job in res for r in job] == want
    out = {}

    def worker():
        out["res"] = _raw(q, dev, 0, 4, S.INDEPENDENT)

    t = threading.Thread(target=worker)
    t.start()
    t.join()
    assert out["res"] == want
    q.close()
    ue.close()


# ------------------------------------------------------------------ 8. acquisition end to end

def test_acquisition_end_to_end():
    """Four 5 ms frames of one cell (CRS of two ports, PBCH, PSS / SSS from the generator's helper, OFDM, noise):
    cell_search finds the id, the CP and the timing; UeDl.fft_estimate at that timing and mi355_pbch_decode_batch give
    the MIB that was encoded and the port count -- none of them passed in."""
    from oracle import ue_dl_chain as uc
    from srsran_amd import enb_dl as E
    from srsran_amd import pbch as B
    from srsran_amd import pdsch as P
    from srsran_amd import sync as S
    from srsran_amd.tdec import DeviceBuffer
    from srsran_amd.ue_dl import DlSfJob, UeDl, default_chest_cfg
    NPRB, CID, PORTS, LEAD = 6, 271, 2, 333
    cell = P.make_cell(NPRB, PORTS, CID, phich_resources=2)
    payload = B.mib_pack(cell, 4 * 37)
    rng = np.random.default_rng(8)
    G = 14 * 12 * NPRB
    sig = []
    for sf in range(20):
        grids = np.zeros((PORTS, G), np.complex64)
        E.put_refs(cell, sf % 10, grids)
        if sf % 10 == 0:
            B.pbch_encode_host(cell, payload, grids, sf // 10)
        E.put_sync(cell, sf % 10, grids)
        sig.append(sum(uc.ofdm_tx_sf(grids[p], NPRB).astype(np.complex128) for p in range(PORTS)))
    x = np.concatenate([np.zeros(LEAD), np.concatenate(sig), np.zeros(2048)])
    sigma = np.sqrt(np.mean(np.abs(x) ** 2) / 2 * 10 ** (-15.0 / 10))
    x = (x + sigma * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))).astype(np.complex64)
    d_iq = DeviceBuffer(x.nbytes).upload(x)
    cells, res = S.cell_search([d_iq.ptr + 8 * 9600 * i for i in range(4)])
    found = cells[CID % 3]
    assert found is not None and (found.cell_id, found.cp, found.frame_type) == (CID, S.CP_NORM, S.FDD)
    assert found.mode == 1.0
    first = res[0][CID % 3]
    assert first.sf_idx == 0
    sf_start = first.peak_pos - 960  # the PSS symbol ends slot 0 of its subframe
    assert sf_start == LEAD
    ue = UeDl(P.make_cell(NPRB, 4, found.cell_id, cp=found.cp), 1)
    d_grid, d_ce = DeviceBuffer(G * 8), DeviceBuffer(4 * G * 8)
    j = DlSfJob()
    j.tti = first.sf_idx
    j.in_buffer[0] = d_iq.ptr + 8 * sf_start
    j.sf_symbols[0] = d_grid.ptr
    for p in range(4):
        j.ce[p][0] = d_ce.ptr + p * G * 8
    chest = ue.fft_estimate([j], default_chest_cfg())
    q = B.Pbch(P.make_cell(NPRB, 0, found.cell_id, cp=found.cp))
    r = q.decode([j], chest, B.INDEPENDENT)[0]
    assert r.ret == 1 and r.nof_tx_ports == PORTS and np.array_equal(r.bits(), payload)
    got_cell, sfn = B.mib_unpack(r.bits())
    assert (got_cell.nof_prb, got_cell.phich_resources, sfn + r.sfn_offset) == (NPRB, 2, 4 * 37)
    q.close()
    ue.close()

