"""GPU: PHICH decoding and the UL grants of the UE receiver (include/srsran_amd/phich.h) against the restatements in
tests/phich_ref.py -- every group x sequence of cells of every port / antenna count, PHICH duration and cell_id % 3,
all ten subframe indices, partial waves, invalid jobs, the estimate-row mode, a caller's stream and a fresh thread, the
degenerate all-zero estimate; format-0 DCIs through the blind search; and the chain from a UL grant to its PHICH."""
import threading

import numpy as np
import pytest

from oracle import pdcch_chain as pd

import phich_ref as R

pytestmark = pytest.mark.gpu

# fixed flat gains per (tx port, rx antenna): transmit diversity assumes the channel constant over a symbol pair
FLAT_H = np.array([[0.9 + 0.3j, -0.4 + 0.8j], [-0.5 + 0.7j, 0.7 + 0.2j], [0.6 - 0.6j, -0.3 - 0.9j],
                   [-0.8 - 0.2j, 0.5 + 0.6j]], np.complex64)


def _cell(nof_prb, nof_ports, cell_id, res=2, ext=0):
    from srsran_amd import pdsch as P
    return P.make_cell(nof_prb, nof_ports, cell_id, phich_length=ext, phich_resources=res)


def _dev(arr):
    from srsran_amd.tdec import DeviceBuffer
    a = np.ascontiguousarray(arr)
    return DeviceBuffer(a.nbytes).upload(a)


class DevSubframes:
    """Subframes (tti, grids (rx, G), ce (ports, rx, G), noise) uploaded as the sfjobs / chest of a control-stage call."""

    def __init__(self, subs):
        from srsran_amd.ue_dl import ChestRes, DlSfJob
        self.keep, self.jobs = [], []
        self.chest = (ChestRes * len(subs))()
        for i, (tti, y, h, noise) in enumerate(subs):
            j = DlSfJob()
            j.tti = tti
            for r in range(y.shape[0]):
                b = _dev(y[r])
                self.keep.append(b)
                j.sf_symbols[r] = b.ptr
                for p in range(h.shape[0]):
                    b = _dev(h[p, r])
                    self.keep.append(b)
                    j.ce[p][r] = b.ptr
            self.jobs.append(j)
            self.chest[i].noise_estimate = noise


def _through_channel(tx, nrx, rng, sigma, ce_sigma=0.0):
    """tx (ports, G) through FLAT_H plus noise: (grids (rx, G), ce (ports, rx, G) = the gains plus estimation error)."""
    ports, G = tx.shape
    h = np.repeat(FLAT_H[:ports, :nrx, None], G, axis=2).astype(np.complex64)
    y = np.einsum("prg,pg->rg", h, tx).astype(np.complex64)
    if sigma:
        y = (y + sigma * (rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape))).astype(np.complex64)
    if ce_sigma:
        h = (h + ce_sigma * (rng.standard_normal(h.shape) + 1j * rng.standard_normal(h.shape))).astype(np.complex64)
    return y, h


def _grant_of(nof_prb, ngroups):
    """(ngroup, nseq) -> a grant (n_prb_lowest, n_dmrs) that srslte_phich_calc maps there"""
    m = {}
    for lo in range(nof_prb):
        for dm in range(8):
            m.setdefault(R.phich_calc(ngroups, lo, dm, 0), (lo, dm))
    assert len(m) == 8 * ngroups
    return m


def _phich_subframe(cell, rg, nrx, tti, rng, sigma, ce_sigma=0.0):
    """Every (group, sequence) of the cell loaded with a random ACK: (grids, ce, acks (groups, 8))"""
    from srsran_amd import phich as H
    acks = rng.integers(0, 2, (rg.phich.shape[0], R.NSEQ))
    tx = np.zeros((cell.nof_ports, 14 * 12 * cell.nof_prb), np.complex64)
    for g in range(acks.shape[0]):
        for s in range(R.NSEQ):
            assert H.phich_encode_host(cell, tti, g, s, int(acks[g, s]), tx) == 0
    y, h = _through_channel(tx, nrx, rng, sigma, ce_sigma)
    return y, h, acks


def _bits(x):
    return np.array([np.float32(x)]).view(np.uint32)[0]


def _res(r):
    return (r.ret, r.ack_value, _bits(r.distance))


# (nof_prb, phich_resources, phich_length, cell_id, subframe indices): one group / two groups at 6 PRB, 15 PRB, 25 groups
# at 100 PRB; both durations; cell_id % 3 = 0, 1, 2; all ten subframe indices in the first cell
CELLS = [(6, 0, 0, 300, tuple(range(10))), (6, 3, 1, 1, (0, 7)), (15, 2, 0, 503, (4, 9)), (15, 1, 1, 149, (5, 2)),
         (100, 3, 0, 77, (8, 1))]


@pytest.mark.parametrize("nof_ports", [1, 2, 4])
@pytest.mark.parametrize("case", CELLS, ids=[f"prb{c[0]}_ng{c[1]}_ext{c[2]}" for c in CELLS])
def test_parity(case, nof_ports):
    """Every group x all 8 sequences with random ACKs, rx 1 and 2, jobs of all subframes interleaved in one batch.
    Even subframes are noise-free (perfect estimates): every ACK comes back.  Odd ones carry noise and estimation
    error: ack_value and distance equal the restatement's, distance bit for bit."""
    from srsran_amd import phich as H
    from srsran_amd.ue_dl import UeDl
    nof_prb, res, ext, cell_id, sfs = case
    cell = _cell(nof_prb, nof_ports, cell_id, res, ext)
    rg = R.regs(nof_prb, nof_ports, cell_id, res, ext)
    ngroups = rg.phich.shape[0]
    assert ngroups == H.ngroups(cell)
    grant_of = _grant_of(nof_prb, ngroups)
    rng = np.random.default_rng(cell_id * 10 + nof_ports)
    for nrx in (1, 2):
        subs, acks = [], []
        for k, sf_idx in enumerate(sfs):
            noisy = k % 2 == 1
            y, h, a = _phich_subframe(cell, rg, nrx, 20 + sf_idx, rng, 0.25 if noisy else 0.0, 0.05 if noisy else 0.0)
            subs.append((20 + sf_idx, y, h, 0.07 if noisy else 0.0))
            acks.append(a)
        dev = DevSubframes(subs)
        jobs = [(k, *grant_of[(g, s)], 0) for g in range(ngroups) for s in range(R.NSEQ) for k in range(len(sfs))]
        ue = UeDl(cell, nrx)
        got = H.decode_phich(ue, dev.jobs, dev.chest, jobs)
        for i, (k, lo, dm, _ip) in enumerate(jobs):
            g, s = R.phich_calc(ngroups, lo, dm, 0)
            tti, y, h, noise = subs[k]
            ack, dist = R.phich_decode(y, h, rg.phich[g], cell_id, tti % 10, s, noise)
            assert _res(got[i]) == (0, ack, _bits(dist)), (nrx, k, g, s, got[i].distance, dist)
            if k % 2 == 0:
                assert got[i].ack_value == acks[k][g, s], (nrx, k, g, s)
        ue.close()


def _small_case(nof_ports=2, nrx=2, nsf=3, ext=0, seed=5):
    """A 15-PRB Ng = 1 cell (two groups), noisy subframes, every (subframe, group, sequence) as a job."""
    from srsran_amd import phich as H
    nof_prb, cell_id = 15, 23
    cell = _cell(nof_prb, nof_ports, cell_id, 2, ext)
    rg = R.regs(nof_prb, nof_ports, cell_id, 2, ext)
    rng = np.random.default_rng(seed)
    subs = []
    for k in range(nsf):
        y, h, _a = _phich_subframe(cell, rg, nrx, 3 * k + 1, rng, 0.3, 0.05)
        subs.append((3 * k + 1, y, h, 0.1))
    grant_of = _grant_of(nof_prb, 2)
    jobs = [(k, *grant_of[(g, s)], 0) for s in range(R.NSEQ) for k in range(nsf) for g in range(2)]
    want = []
    for (k, lo, dm, _ip) in jobs:
        g, s = R.phich_calc(2, lo, dm, 0)
        ack, dist = R.phich_decode(subs[k][1], subs[k][2], rg.phich[g], cell_id, subs[k][0] % 10, s, subs[k][3])
        want.append((0, ack, _bits(dist)))
    return cell, rg, subs, jobs, want, H


def test_partial_waves_and_empty_batch():
    """1, 15, 16, 17 and 65 jobs (16 jobs fill a wave, 64 a workgroup) and the whole list of 48, then jobs tiled to
    65: each equals the restatement.  njobs = 0 succeeds."""
    from srsran_amd.ue_dl import UeDl
    cell, _rg, subs, jobs, want, H = _small_case()
    dev = DevSubframes(subs)
    ue = UeDl(cell, 2)
    assert H._declare().mi355_ue_dl_decode_phich_batch(ue.h, None, None, None, 0, None, 0, None, None) == 0
    assert len(H.decode_phich(ue, dev.jobs, dev.chest, [])) == 1  # (the wrapper's placeholder element, untouched)
    for n in (1, 15, 16, 17, 48, 65):
        jj = [jobs[i % len(jobs)] for i in range(n)]
        got = H.decode_phich(ue, dev.jobs, dev.chest, jj)
        assert [_res(got[i]) for i in range(n)] == [want[i % len(jobs)] for i in range(n)], n
    ue.close()


def test_invalid_jobs_between_valid_ones():
    """I_phich = 1 (ngroup >= ngroups in FDD) and sf >= nsf: those jobs get MI355_ERROR_INVALID_INPUTS on the host,
    their neighbours the results of a run without them."""
    from srsran_amd.ue_dl import UeDl
    cell, _rg, subs, jobs, want, H = _small_case(nof_ports=1, nrx=1)
    dev = DevSubframes(subs)
    ue = UeDl(cell, 1)
    mixed, expect = [], []
    bad = [(0, 3, 1, 1), (len(subs), 0, 0, 0), (0xFFFFFFFF, 2, 2, 0), (1, 14, 7, 1)]
    for i, j in enumerate(jobs[:20]):
        if i % 3 == 1:
            mixed.append(bad[(i // 3) % len(bad)])
            expect.append((H.ERROR_INVALID_INPUTS, 0, _bits(0.0)))
        mixed.append(j)
        expect.append(want[i])
    got = H.decode_phich(ue, dev.jobs, dev.chest, mixed)
    assert [_res(got[i]) for i in range(len(mixed))] == expect
    only_bad = H.decode_phich(ue, dev.jobs, dev.chest, bad)
    assert all(only_bad[i].ret == H.ERROR_INVALID_INPUTS for i in range(len(bad)))
    ue.close()


def test_ce_rows_first_only():
    """mi355_ue_dl_set_ce_rows(1): only row 0 of every estimate is valid (time-invariant estimates), so the extended
    PHICH's REs in symbols 1 and 2 are equalised with row 0 -- the restatement on estimates tiled from row 0."""
    from srsran_amd.ue_dl import CE_ROWS_FIRST, UeDl
    cell, rg, subs, jobs, _want, H = _small_case(nof_ports=2, nrx=2, nsf=2, ext=1, seed=8)
    assert (rg.phich // (12 * cell.nof_prb)).max() == 2  # the groups do reach symbols 1 and 2
    row = 12 * cell.nof_prb
    rng = np.random.default_rng(3)
    tiled, poisoned = [], []
    for (tti, y, h, nz) in subs:
        h0 = (h[:, :, :row] + 0.1 * rng.standard_normal(h[:, :, :row].shape)).astype(np.complex64)
        tiled.append((tti, y, np.tile(h0, (1, 1, 14)), nz))
        p = np.full(h.shape, 1e6 + 1e6j, np.complex64)
        p[:, :, :row] = h0
        poisoned.append((tti, y, p, nz))
    dev = DevSubframes(poisoned)
    ue = UeDl(cell, 2)
    ue.set_ce_rows(CE_ROWS_FIRST)
    got = H.decode_phich(ue, dev.jobs, dev.chest, jobs)
    for i, (k, lo, dm, _ip) in enumerate(jobs):
        g, s = R.phich_calc(2, lo, dm, 0)
        ack, dist = R.phich_decode(tiled[k][1], tiled[k][2], rg.phich[g], cell.id, tiled[k][0] % 10, s, tiled[k][3])
        assert _res(got[i]) == (0, ack, _bits(dist)), i
    ue.close()


def test_callers_stream_and_fresh_thread():
    """A call on a caller's stream (another object's non-blocking stream) and a call from a host thread that never
    selected a device return what a call on the object's own stream returns."""
    from srsran_amd import lib
    from srsran_amd.ue_dl import UeDl
    cell, _rg, subs, jobs, want, H = _small_case(nof_ports=4, nrx=1, nsf=2)
    dev = DevSubframes(subs)
    ue, other = UeDl(cell, 1), UeDl(cell, 1)
    got = H.decode_phich(ue, dev.jobs, dev.chest, jobs, stream=other.stream())
    assert lib().mi355_device_sync() == 0
    assert [_res(got[i]) for i in range(len(jobs))] == want
    out = {}

    def worker():
        r = H.decode_phich(ue, dev.jobs, dev.chest, jobs)
        out["res"] = [_res(r[i]) for i in range(len(jobs))]

    t = threading.Thread(target=worker)
    t.start()
    t.join()
    assert out["res"] == want
    ue.close()
    other.close()


def test_all_zero_estimates():
    """1 port, zero estimates and zero noise: every soft bit is 0 / 0.  srslte_phich_ack_decode then exceeds its -9999
    start value with neither correlation and leaves distance unwritten (the restatement: None); the documented result
    is ack_value 0, distance 0, ret MI355_SUCCESS -- and a sound job beside it is untouched."""
    from srsran_amd.ue_dl import UeDl
    cell, rg, subs, jobs, want, H = _small_case(nof_ports=1, nrx=1, nsf=1)
    tti, y, h, _nz = subs[0]
    zero = (tti, y, np.zeros_like(h), 0.0)
    assert R.phich_decode(y, zero[2], rg.phich[0], cell.id, tti % 10, 0, 0.0) == (0, None)
    dev = DevSubframes([zero, subs[0]])
    ue = UeDl(cell, 1)
    j0 = jobs[0]
    got = H.decode_phich(ue, dev.jobs, dev.chest, [(0, *j0[1:]), (1, *j0[1:]), (0, *jobs[5][1:])])
    assert _res(got[0]) == (0, 0, _bits(0.0)) and _res(got[2]) == (0, 0, _bits(0.0))
    assert _res(got[1]) == want[0]
    ue.close()


# ------------------------------------------------------------------ UL grants

def _ul_dci(D, H, cell, rnti, L_crb, rb_start, n_dmrs, mcs=11):
    d = H.DciUl()
    d.rnti, d.format = rnti, D.FORMAT0
    d.freq_hop_fl = H.HOP_DISABLED
    d.type2_alloc.riv = D._declare().mi355_ra_type2_to_riv(L_crb, rb_start, cell.nof_prb)
    d.tb.mcs_idx, d.tb.ndi, d.tpc_pusch, d.n_dmrs, d.cqi_request = mcs, 1, 1, n_dmrs, 1
    return d


def _dl_1a(D, cell, rnti):
    d = D.DciDl()
    d.rnti, d.format, d.alloc_type = rnti, D.FORMAT1A, D.ALLOC_TYPE2
    d.type2_alloc.riv = D._declare().mi355_ra_type2_to_riv(4, 2, cell.nof_prb)
    d.tb[0].mcs_idx, d.tb[0].rv, d.tb[0].ndi = 7, 0, 1
    d.tb[1].mcs_idx, d.tb[1].rv = 0, 1
    return d


UL_CASES = ["lone_ue_space", "with_dl_dci", "two_levels", "common_space", "none"]


def _ul_subframe(D, H, cell, case, sf_idx, cfi, rnti, rng, nrx):
    """One control region for a UL-grant case: (tti, grids, ce, noise)"""
    ncce = D.nof_cce(cell, cfi)
    locs = D.ue_locations(ncce, sf_idx, rnti)
    l2 = next(lv for lv in locs if lv[0] == 2)
    l3 = next(lv for lv in locs if lv[0] == 3 and (lv[1] + 8 <= l2[1] or l2[1] + 4 <= lv[1]))
    com = D.DciCfg()
    com.is_not_ue_ss = 1
    msgs = []

    def place(m, loc):
        m.location, m.rnti = D.DciLocation(*loc), rnti
        msgs.append(m)

    ul = _ul_dci(D, H, cell, rnti, 3 + sf_idx, 2 * sf_idx, sf_idx % 8)
    if case == "lone_ue_space":
        place(H.pack_pusch(cell, ul), l2)
    elif case == "with_dl_dci":
        place(H.pack_pusch(cell, ul), l2)
        place(D.pack(cell, _dl_1a(D, cell, rnti), sf_idx), l3)
    elif case == "two_levels":
        place(H.pack_pusch(cell, ul), l2)
        place(H.pack_pusch(cell, ul), l3)
    elif case == "common_space":
        c4 = next(lv for lv in D.common_locations(ncce) if lv[0] == 2 and lv not in locs)
        place(H.pack_pusch(cell, ul, com), c4)
    else:
        place(D.pack(cell, _dl_1a(D, cell, rnti), sf_idx), l2)
    tx = np.zeros((cell.nof_ports, 14 * 12 * cell.nof_prb), np.complex64)
    D.encode_ctrl_host(cell, sf_idx, cfi, msgs, tx)
    y, h = _through_channel(tx, nrx, rng, 0.05)
    return (sf_idx, y, h, 0.005), msgs


@pytest.mark.parametrize("case", UL_CASES)
def test_find_ul_dci(case):
    """Subframes synthesised with mi355_pdcch_encode_host from mi355_dci_msg_pack_pusch: find_ul_dci_batch returns the
    restated search's pending format-0 messages field by field and in order (a grant seen at two aggregation levels
    once), the DL results stay those of pdcch_chain.find_dl_dci, and a second call returns nothing."""
    from srsran_amd import pdcch as D
    from srsran_amd import phich as H
    from srsran_amd.ue_dl import UeDl
    nof_prb, ports, nrx, cell_id, rnti, cfi = 50, 2, 2, 11, 0x4602, 3
    cell = _cell(nof_prb, ports, cell_id, 0)
    rng = np.random.default_rng(UL_CASES.index(case))
    sf_idxs = (1, 4, 7)
    subs = [_ul_subframe(D, H, cell, case, sf, cfi, rnti, rng, nrx)[0] for sf in sf_idxs]
    dev = DevSubframes(subs)
    ucfg = D.UeDlCfg()
    ucfg.tm, ucfg.dci_common_ss = 0, int(case == "common_space")
    ue = UeDl(cell, nrx)
    n = len(subs)
    cfis, ctrl, dl = D.find_dl_dci(ue, dev.jobs, [rnti] * n, [ucfg] * n, dev.chest)
    ul = H.find_ul_dci(ue, list(sf_idxs), [rnti] * n, [ucfg] * n)
    rg = pd.regs(nof_prb, ports, cell_id, 0)
    for i, (tti, y, h, nz) in enumerate(subs):
        assert cfis[i] == cfi
        llr = pd.pdcch_llr(y, h, rg, cfi, cell_id, tti, nz)
        assert np.array_equal(D.last_llr(ue, i), llr)
        want_dl, want_ul = R.find_dci(llr, rg.nof_cce(cfi), tti, rnti, nof_prb, ports, 0, None, case == "common_space")
        plain = pd.find_dl_dci(llr, rg.nof_cce(cfi), tti, rnti, nof_prb, ports, tm=0, dci_common_ss=case == "common_space")
        assert [(m["format"], m["L"], m["ncce"]) for m in plain] == [(m["format"], m["L"], m["ncce"]) for m in want_dl]
        assert [(d.format, d.location.L, d.location.ncce) for d in dl[i]] == [(m["format"], m["L"], m["ncce"]) for m in plain]
        assert len(want_ul) == (0 if case == "none" else 1), (case, i, want_ul)
        assert len(want_dl) == (1 if case in ("with_dl_dci", "none") else 0)
        assert len(ul[i]) == len(want_ul)
        for d, m in zip(ul[i], want_ul):
            assert (d.rnti, d.format, d.location.L, d.location.ncce) == (rnti, D.FORMAT0, m["L"], m["ncce"])
            assert H.ul_fields(d) == m["dci"]
            assert (d.n_dmrs, d.tb.mcs_idx, d.cqi_request, d.freq_hop_fl) == (tti % 8, 11, 1, H.HOP_DISABLED)
            assert pd.type2_from_riv(d.type2_alloc.riv, nof_prb, nof_prb) == (3 + tti, 2 * tti)
    again = H.find_ul_dci(ue, list(sf_idxs), [rnti] * n, [ucfg] * n)
    assert all(len(a) == 0 for a in again)
    # rnti = 0 returns nothing (and the next control-stage call starts the lists empty)
    D.find_dl_dci(ue, dev.jobs, [rnti] * n, [ucfg] * n, dev.chest)
    assert all(len(a) == 0 for a in H.find_ul_dci(ue, list(sf_idxs), [0] * n, [ucfg] * n))
    ue.close()


def test_ul_grant_to_phich_chain():
    """A UL grant decoded in TTI n gives RB_start and n_dmrs; the PUSCH goes out in n + 4 and its HARQ indicator comes
    back in n + 8 on the resource mi355_phich_calc derives from them -- among the other UEs' PHICHs of that subframe."""
    from srsran_amd import pdcch as D
    from srsran_amd import phich as H
    from srsran_amd.ue_dl import UeDl
    nof_prb, ports, nrx, cell_id, rnti, cfi = 50, 2, 2, 11, 0x4602, 3
    cell = _cell(nof_prb, ports, cell_id, 2)
    rg = R.regs(nof_prb, ports, cell_id, 2, 0)
    rng = np.random.default_rng(21)
    ue = UeDl(cell, nrx)
    ucfg = D.UeDlCfg()
    for n_tti, sent in ((1, 1), (4, 0), (7, 1)):
        sub, _msgs = _ul_subframe(D, H, cell, "lone_ue_space", n_tti, cfi, rnti, rng, nrx)
        dev = DevSubframes([sub])
        D.find_dl_dci(ue, dev.jobs, [rnti], [ucfg], dev.chest)
        (grants,) = H.find_ul_dci(ue, [n_tti], [rnti], [ucfg])
        assert len(grants) == 1
        _L, rb_start = pd.type2_from_riv(grants[0].type2_alloc.riv, nof_prb, nof_prb)
        g, s = H.calc(cell, rb_start, grants[0].n_dmrs)
        assert (g, s) == R.phich_calc(rg.phich.shape[0], 2 * n_tti, n_tti % 8, 0)
        # the eNodeB's subframe n + 8: this UE's indicator and every other sequence of every group, random
        tti = n_tti + 8
        tx = np.zeros((ports, 14 * 12 * nof_prb), np.complex64)
        for gg in range(rg.phich.shape[0]):
            for ss in range(R.NSEQ):
                a = sent if (gg, ss) == (g, s) else int(rng.integers(0, 2))
                assert H.phich_encode_host(cell, tti, gg, ss, a, tx) == 0
        y, h = _through_channel(tx, nrx, rng, 0.05)
        dv = DevSubframes([(tti, y, h, 0.005)])
        got = H.decode_phich(ue, dv.jobs, dv.chest, [(0, rb_start, grants[0].n_dmrs, 0)])
        assert (got[0].ret, got[0].ack_value) == (0, sent)
        assert got[0].distance > 0.5
    ue.close()
