"""CPU: the host functions of include/srsran_amd/sync.h (PSS / SSS generation, the put_slot functions, the cell-search
vote) and the float64 restatement of the stage (tests/sync_ref.py) on the real recording and on synthetic frames."""
import os

import numpy as np
import pytest

import sync_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
RECORDING = os.path.join(HERE, "golden", "signal_1.92M_amar.c64")


# ------------------------------------------------------------------ sequences

@pytest.mark.parametrize("n_id_2", [0, 1, 2])
def test_pss_generate(n_id_2):
    """The library's PSS is the Zadoff-Chu sequence of 36.211 6.11.1.1 (roots 25, 29, 34), unit modulus, and equals
    the restatement's within the float32 rounding of cosf / sinf."""
    from srsran_amd import sync as S
    got = S.pss_generate(n_id_2)
    u = (25, 29, 34)[n_id_2]
    n = np.arange(62)
    zc = np.where(n < 31, np.exp(-1j * np.pi * u * n * (n + 1) / 63), np.exp(-1j * np.pi * u * (n + 1) * (n + 2) / 63))
    # the reference rounds the argument to float32; it reaches 34 pi 62 = 6.6e3, where half an ulp is 2.44e-4
    assert np.abs(got - zc).max() < 2.5e-4
    assert np.abs(got - R.pss_generate(n_id_2)).max() < 3e-7
    assert np.abs(np.abs(got) - 1).max() < 3e-7
    with pytest.raises(RuntimeError):
        S.pss_generate(3)


def test_sss_generate_all_cells():
    """Every cell id: +-1 values, equal to the restatement's; subframes 0 and 5 differ; the 504 x 2 sequences are
    pairwise distinct; (m0, m1) of N_id_1 = 0, 1, 29, 30, 167 are the entries of 36.211 table 6.11.2.1-1."""
    from srsran_amd import sync as S
    seen = set()
    for cid in range(504):
        s0, s5 = S.sss_generate(cid)
        r0, r5 = R.sss_generate(cid)
        assert np.array_equal(s0, r0) and np.array_equal(s5, r5)
        assert set(np.unique(s0)) == {-1.0, 1.0} and not np.array_equal(s0, s5)
        seen.add(s0.tobytes())
        seen.add(s5.tobytes())
    assert len(seen) == 1008
    assert [R.m0m1(i) for i in (0, 1, 29, 30, 167)] == [(0, 1), (1, 2), (29, 30), (0, 2), (2, 9)]
    with pytest.raises(RuntimeError):
        S.sss_generate(504)


def test_sequences_against_fixture():
    """The library's PSS (three N_id_2) and SSS (subframes 0 and 5 of ten cell ids over all N_id_2 and N_id_1 0, 29, 30,
    167) are the compiled reference's srslte_pss_generate / srslte_sss_generate output recorded in the fixture, value
    for value."""
    from srsran_amd import sync as S
    z = np.load(os.path.join(HERE, "golden", "sync_find.npz"))
    for i in range(3):
        assert np.array_equal(S.pss_generate(i), z["pss"][i])
    assert len(z["sss_ids"]) == 10
    for k, cid in enumerate(z["sss_ids"]):
        s0, s5 = S.sss_generate(int(cid))
        assert np.array_equal(s0, z["sss"][k, 0]) and np.array_equal(s5, z["sss"][k, 1]), cid


def test_sss_m_sequences_are_the_standard_ones():
    """s~, c~, z~ from their 36.211 recurrences: balanced m-sequences (16 ones) with the two-valued autocorrelation"""
    for seq in R.m_sequences():
        assert (seq == -1).sum() == 16
        for sh in range(1, 31):
            assert np.dot(seq, np.roll(seq, sh)) == -1


@pytest.mark.parametrize("cp", [R.CP_NORM, R.CP_EXT])
@pytest.mark.parametrize("nof_prb", [6, 15, 100])
def test_put_slot(nof_prb, cp):
    """Positions (last / second last symbol of the slot, 62 REs around DC) and the five nulled REs on either side;
    everything else untouched."""
    from srsran_amd import sync as S
    nsymb, nre = (7 if cp == R.CP_NORM else 6), 12 * nof_prb
    k = nre // 2 - 31
    pss = S.pss_generate(1)
    sss = S.sss_generate(151)[1]
    fill = np.complex64(3 + 4j)
    slot = np.full(nsymb * nre, fill, np.complex64)
    S.pss_put_slot(pss, slot, nof_prb, cp)
    S.sss_put_slot(sss, slot, nof_prb, cp)
    g = slot.reshape(nsymb, nre)
    assert np.array_equal(g[nsymb - 1, k:k + 62], pss) and np.array_equal(g[nsymb - 2, k:k + 62], sss.astype(np.complex64))
    for row in (nsymb - 1, nsymb - 2):
        assert not g[row, k - 5:k].any() and not g[row, k + 62:k + 67].any()
        assert (g[row, :k - 5] == fill).all() and (g[row, k + 67:] == fill).all()
    assert (g[:nsymb - 2] == fill).all()
    # the numpy helper of the restatement places them in the same REs
    ref = np.full((2 * nsymb, nre), fill, np.complex128)
    R.put_sync(ref, nof_prb, 151, 5, cp)
    assert np.abs(ref[:nsymb].reshape(-1) - slot).max() < 3e-7


# ------------------------------------------------------------------ the vote

def _cand(cell_id, cp=0, ft=0, peak=1.0, psr=3.0, cfo=0.0):
    from srsran_amd import sync as S
    r = S.SyncRes()
    r.ret, r.cell_id, r.cp, r.frame_type, r.peak_abs, r.peak_value, r.cfo_pss_mean = 1, cell_id, cp, ft, peak, psr, cfo
    return r


def test_cellsearch_pick():
    from srsran_amd import sync as S
    # a single candidate
    o = S.cellsearch_pick([_cand(7, 1, 1, 2.5, 4.0, 0.25)])
    assert (o.cell_id, o.cp, o.frame_type, o.peak, o.mode, o.psr, o.cfo) == (7, 1, 1, 2.5, 1.0, 4.0, 0.25)
    # a majority id with a minority CP and frame type; psr and cfo from the last candidate, peak averaged over all
    c = [_cand(10, 0, 0, 1.0), _cand(11, 1, 1, 2.0), _cand(10, 1, 0, 3.0), _cand(10, 0, 1, 4.0), _cand(12, 1, 1, 6.0, 9.0, -0.5)]
    o = S.cellsearch_pick(c)
    assert (o.cell_id, o.cp, o.frame_type) == (10, R.CP_NORM, R.FDD)
    assert o.peak == pytest.approx(16.0 / 5) and o.mode == pytest.approx(3 / 5) and (o.psr, o.cfo) == (9.0, -0.5)
    # a tie between two ids: the first one met wins (strict >)
    o = S.cellsearch_pick([_cand(5), _cand(6), _cand(6), _cand(5)])
    assert o.cell_id == 5 and o.mode == 0.5
    # an even split of the CP among the winner's candidates is not a majority: extended, and likewise TDD
    o = S.cellsearch_pick([_cand(5, 0, 0), _cand(5, 1, 1)])
    assert (o.cp, o.frame_type) == (R.CP_EXT, R.TDD)
    with pytest.raises(RuntimeError):
        S.cellsearch_pick([])


# ------------------------------------------------------------------ the restatement

def test_recording_correlation_peaks():
    """The recording's correlation against the N_id_2 = 1 replica peaks where windows end at samples 959 and 10559
    (outputs 960 and 10560, one past the window's last sample) far above the median; the other two replicas do not."""
    iq = np.fromfile(RECORDING, np.complex64).astype(np.complex128)
    ratios = []
    for id2 in range(3):
        q = R.SyncRef(128, 9600, id2)
        c = np.abs(np.convolve(iq[:19200], q.h)) ** 2
        ratios.append(c.max() / np.median(c))
        if id2 == 1:
            assert int(np.argmax(c[:9600])) - 1 == 959 and int(np.argmax(c[9600:19200])) + 9600 - 1 == 10559
    assert ratios[1] > 1000 and ratios[0] < 500 and ratios[2] < 500, ratios


def test_recording_restatement():
    """First 5 ms with N_id_2 = 1: cell id 1, subframe 0, normal CP, FDD; second 5 ms: subframe 5."""
    iq = np.fromfile(RECORDING, np.complex64)
    for half, sf in ((0, 0), (1, 5)):
        for alg in (R.FULL, R.PARTIAL_3, R.DIFF):
            q = R.SyncRef(128, 9600, 1, cfo_pss_enable=True, sss_alg=alg)
            r = q.find(iq[half * 9600:half * 9600 + 9600 + 128])
            assert (r["ret"], r["peak_pos"], r["cell_id"], r["sf_idx"], r["cp"], r["frame_type"]) == \
                (R.FOUND, 960, 1, sf, R.CP_NORM, R.FDD), (half, alg, r)
            assert R.safe(r)
    for id2 in (0, 2):
        r = R.SyncRef(128, 9600, id2).find(iq[:9600 + 128])
        assert r["cell_id"] != 1


def _pss_end(cp, ft, lead):
    """the correlation output at which a synthetic frame's PSS peaks: the end of its PSS symbol"""
    nsymb = 7 if cp == R.CP_NORM else 6
    sym = 128 + R.cp_sz(128, cp)
    first = R.cp_len(128, 160) if cp == R.CP_NORM else 32
    pss_sym = (nsymb - 1) if ft == R.FDD else (2 * nsymb + 2)
    return lead + (pss_sym // nsymb) * 960 + first + (pss_sym % nsymb) * sym + 128


@pytest.mark.parametrize("cp", [R.CP_NORM, R.CP_EXT])
@pytest.mark.parametrize("ft", [R.FDD, R.TDD])
def test_restatement_synthetic(cp, ft):
    """Synthetic frames of the numpy generator are acquired by the restatement.  With a CFO of +-0.3 subcarriers the
    CP is given (the CP metric is the real part of a correlation that such a CFO turns negative; the reference corrects
    the CFO from the CP first, which is out of scope): id, subframe, frame type, peak position and CFO.  Without CFO
    the CP is detected: a normal-CP object finds an extended-CP cell's CP on the first call and, the SSS then being
    looked for in the right place, its id on the second."""
    for k, (cid, sf) in enumerate(((0, 0), (4, 5), (89, 0), (92, 5), (503, 0))):
        lead, cfo = 700 + 37 * k, 0.3 if k % 2 else -0.3
        x = R.synth_frame(cid, sf, cp, ft, lead=lead, cfo=cfo, seed=k)
        r = R.SyncRef(128, 9600, cid % 3, cfo_pss_enable=True, detect_cp=False, cp=cp).find(x)
        assert (r["ret"], r["cell_id"], r["cp"], r["frame_type"]) == (R.FOUND, cid, cp, ft), (cid, r)
        assert r["sf_idx"] == sf + (1 if ft == R.TDD else 0)
        assert abs(r["cfo_pss"] - cfo) < 0.05
        assert r["peak_pos"] == _pss_end(cp, ft, lead)
        x = R.synth_frame(cid, sf, cp, ft, lead=lead, seed=k)
        q = R.SyncRef(128, 9600, cid % 3)
        r = q.find(x)
        assert (r["ret"], r["cp"]) == (R.FOUND, cp)
        r = q.find(x)
        assert (r["ret"], r["cell_id"], r["cp"], r["frame_type"]) == (R.FOUND, cid, cp, ft), (cid, r)


def test_restatement_against_fixture():
    """tests/golden/sync_find.npz (the compiled reference's srslte_sync_find with a double-precision DFT standing in for
    FFTW, tests/golden/make_golden_sync.py): the restatement gives the reference's decisions for every call whose
    margins are safe, and its float fields within the tolerances of sync_ref.py.  m0 / m1 / n_id_1 are compared where
    the SSS was detected (the reference leaves an uninitialised N_id_1 otherwise)."""
    import json
    z = np.load(os.path.join(HERE, "golden", "sync_find.npz"))
    meta, iv, fv = json.loads(str(z["meta"])), z["iv"], z["fv"]
    ivf, fvf = [str(f) for f in z["iv_fields"]], [str(f) for f in z["fv_fields"]]
    objs, unsafe, frames = {}, 0, {}
    for i, m in enumerate(meta):
        if m["case"] not in objs:
            objs[m["case"]] = R.SyncRef(**m["cfg"])
        key = json.dumps(m["src"], sort_keys=True)
        if key not in frames:
            src = m["src"]
            frames = {key: np.fromfile(RECORDING, np.complex64)[src["start"]:src["start"] + src["len"]]
                      if src["kind"] == "recording" else R.synth_frame(**src["args"])}
        x = np.concatenate([frames[key], np.zeros(1024, np.complex64)])
        w = objs[m["case"]].find(x, m["find_offset"])
        if not R.safe(w):
            unsafe += 1
            continue
        got = dict(zip(ivf, (int(v) for v in iv[i])))
        got.update(zip(fvf, (float(v) for v in fv[i])))
        if not w["sss_detected"]:
            for f in ("m0", "m1", "n_id_1", "cell_id", "m0_value", "m1_value"):
                got[f] = w[f]
        if not w["sss_available"]:
            got["sss_corr"] = w["sss_corr"]
        R.compare(got, w, f"fixture call {i}")
    assert unsafe <= 0.05 * len(meta)
