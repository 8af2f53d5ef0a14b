"""GPU parity of the downlink control path (PCFICH, PDCCH LLRs, blind search, DCI -> grant -> PDSCH) through the
product's C ABI against the oracle (oracle/orc_pdcch.c, oracle/pdcch_chain.py) and the reference goldens.

Bars: CFI, PDCCH LLRs, candidate CRC remainders / payloads and the blind-search result bit-exact with the oracle;
LLRs within 1e-5 of the range of the reference's own srslte_pdcch_extract_llr (goldens); end-to-end from I/Q every
subframe's DCI and PDSCH payload recovered with the TB CRC passing."""
import numpy as np
import pytest

from golden_io import load
from oracle import pdcch_chain as P
from oracle import pdsch_chain as pc
from oracle import ue_dl_chain as uc

pytestmark = pytest.mark.gpu


def _dev(arr):
    from srsran_amd.tdec import DeviceBuffer
    a = np.ascontiguousarray(arr)
    return DeviceBuffer(a.nbytes).upload(a)


def _host_job(y, h, sf, noise):
    """One control-channel job from host grids y (rx, G) and estimates h (ports, rx, G): (job, chest, buffers)"""
    from srsran_amd.ue_dl import ChestRes, DlSfJob
    nrx, ports = y.shape[0], h.shape[0]
    keep = [_dev(y[r]) for r in range(nrx)] + [_dev(h[p, r]) for p in range(ports) for r in range(nrx)]
    j = DlSfJob()
    j.tti = sf
    for r in range(nrx):
        j.sf_symbols[r] = keep[r].ptr
        for p in range(ports):
            j.ce[p][r] = keep[nrx + p * nrx + r].ptr
    chest = (ChestRes * 1)()
    chest[0].noise_estimate = noise
    return j, chest, keep


def _region_jobs(k, Z):
    from srsran_amd import pdsch as S
    nprb, ports, nrx, cid, sf, cfi = (int(v) for v in Z[f"sf{k}_cfg"])
    glen = 14 * 12 * nprb
    y = np.zeros((nrx, glen), np.complex64)
    h = np.zeros((ports, nrx, glen), np.complex64)
    c = Z[f"sf{k}_y"].shape[1]
    y[:, :c], h[:, :, :c] = Z[f"sf{k}_y"], Z[f"sf{k}_h"]
    j, chest, keep = _host_job(y, h, sf, float(Z[f"sf{k}_noise"]))
    return S.make_cell(nprb, ports, cid), nrx, j, chest, keep, y, h


def _check_slots(cand, o_llr, ncce, sf, rnti, nb_ue, nb_com):
    """Every one of the 22 slots x 2 sizes of a subframe's raw candidate results against the oracle on the same LLRs.
    nb_ue / nb_com: the payload sizes tried per format slot in the UE-specific / common space (0: none; None: the
    space is not searched).  Slots 0-15 list P.ue_locations in order, slots 16-21 P.common_locations; a slot past its
    list, or a size not tried, has status 0; an occupied one carries its (L, ncce) and status 1 when the oracle's
    mean-|LLR| gate skips it, else status 2 with the oracle's CRC remainder and payload.  Returns the status counts."""
    ue = P.ue_locations(ncce, sf, rnti) if nb_ue else []
    com = P.common_locations(ncce) if nb_com else []
    count = [0, 0, 0]
    assert cand.shape == (22, 2)
    for s in range(22):
        locs, nb, k = (ue, nb_ue, s) if s < 16 else (com, nb_com, s - 16)
        for f in range(2):
            c = cand[s, f]
            if k >= len(locs) or not nb[f]:
                assert c["status"] == 0, (s, f)
                count[0] += 1
                continue
            L, n = locs[k]
            ok, bits, crc = P.decode_candidate(o_llr, L, n, nb[f])
            assert c["status"] == (2 if ok else 1) and (c["L"], c["ncce"]) == (L, n), (s, f)
            count[int(c["status"])] += 1
            if ok:
                assert c["crc_rem"] == crc, (s, f)
                got = np.unpackbits(c["bits"].astype(">u4").view(np.uint8))
                assert np.array_equal(got[: nb[f]], bits) and not got[nb[f]:].any(), (s, f)
    return count


@pytest.mark.parametrize("k", range(8))
def test_control_region_goldens(k):
    from srsran_amd import pdcch as D
    from srsran_amd.ue_dl import UeDl
    Z = load("pdcch.npz")
    cell, nrx, job, chest, _keep, y, h = _region_jobs(k, Z)
    nprb, ports, cid, sf = cell.nof_prb, cell.nof_ports, cell.id, job.tti
    ue = UeDl(cell, nrx)
    cfis, ctrl, dcis = D.find_dl_dci(ue, [job], [D.SIRNTI], [D.UeDlCfg()], chest)
    assert cfis[0] == int(Z[f"sf{k}_cfi"]) and ctrl[0].cfi == cfis[0]
    rg = P.regs(nprb, ports, cid, 0)
    noise = float(Z[f"sf{k}_noise"])
    o_cfi, o_corr, _ = P.pcfich_decode(y, h, rg, cid, sf, noise)
    assert o_cfi == cfis[0] and ctrl[0].cfi_corr == max(0.0, float(o_corr.max()))
    llr = D.last_llr(ue, 0)
    o_llr = P.pdcch_llr(y, h, rg, o_cfi, cid, sf, noise)
    assert np.array_equal(llr, o_llr)  # bit-exact with the oracle
    ref = Z[f"sf{k}_llr"]
    assert np.abs(llr - ref).max() <= 1e-5 * np.abs(ref).max()
    # candidates: every slot's status / location / CRC remainder / payload equals the oracle's decode of the same LLRs
    # (UE-specific slots unused for the SI-RNTI, common slots past the list empty, gated-out slots status 1)
    cand = D.last_candidates(ue, 0)
    nb = [P.dci_sizeof(f, nprb, ports, P.DciCfg(is_not_ue_ss=True)) for f in (P.FORMAT1A, P.FORMAT1C)]
    count = _check_slots(cand, o_llr, rg.nof_cce(o_cfi), sf, P.SIRNTI, None, nb)
    assert count[1] + count[2] == 2 * len(P.common_locations(rg.nof_cce(o_cfi)))
    found = P.find_dl_dci(o_llr, rg.nof_cce(o_cfi), sf, P.SIRNTI, nprb, ports)
    assert ctrl[0].nof_dci == len(found) == len(dcis[0])
    for d, f in zip(dcis[0], found):
        assert (d.format, d.location.L, d.location.ncce) == (f["format"], f["L"], f["ncce"])
        assert (d.type2_alloc.riv, d.tb[0].mcs_idx, d.tb[0].rv) == (f["dci"]["riv"], f["dci"]["tb"][0]["mcs_idx"],
                                                                    f["dci"]["tb"][0]["rv"])
    ue.close()


# ------------------------------------------------------------------ UE-specific search space at few CCEs

# a fixed flat channel: one complex gain per transmit port
FLAT_H = np.array([0.9 + 0.3j, -0.5 + 0.7j, 0.6 - 0.6j, -0.8 - 0.2j], np.complex64)
# (nof_prb, ports, cfi, nof_cce): control regions of 1..6 CCEs, where levels drop out of the UE-specific search space
# (N / L = 0) and a level's 6 / 6 / 2 / 2 candidates wrap onto fewer distinct ones
SMALL_REGIONS = [(6, 1, 1, 2), (6, 1, 2, 4), (6, 1, 3, 6), (6, 4, 1, 1), (6, 4, 2, 3), (6, 4, 3, 5), (15, 2, 1, 2)]


@pytest.mark.parametrize("nprb,ports,cfi,ncce", SMALL_REGIONS, ids=[f"{r[0]}prb_{r[1]}p_{r[3]}cce" for r in SMALL_REGIONS])
def test_ue_space_slots_at_few_cces(nprb, ports, cfi, ncce):
    """The device's own enumeration of the search spaces (slot_location, a closed form of pdcch.c:230-330 without the
    candidate list) slot by slot against the oracle's lists, UE-specific slots 0-15 included, in control regions of
    1..6 CCEs.  One format 1A DCI at a UE-specific location (the highest level in one subframe, the first candidate
    in the other) over a flat channel; the search covers the UE-specific space and the common space."""
    from srsran_amd import pdcch as D
    from srsran_amd import pdsch as S
    from srsran_amd.ue_dl import ChestRes, UeDl
    cid, rnti, tm, sigma = 5, 0x3C1A, 0 if ports == 1 else 1, 0.02
    cell = S.make_cell(nprb, ports, cid)
    assert D.nof_cce(cell, cfi) == ncce
    rg = P.regs(nprb, ports, cid, 0)
    G = 14 * 12 * nprb
    rng = np.random.default_rng(100 * nprb + 10 * ports + cfi)
    jobs, keep, grids, noise = [], [], [], 2 * sigma * sigma
    h = np.ascontiguousarray(np.broadcast_to(FLAT_H[:ports, None, None], (ports, 1, G)))
    for sf, pick in ((1, -1), (6, 0)):
        L, n = D.ue_locations(ncce, sf, rnti)[pick]
        m = D.pack(cell, _make_dci(D, cell, P.FORMAT1A, 7, rnti), sf)
        m.location, m.rnti = D.DciLocation(L, n), rnti
        tx = np.zeros((ports, G), np.complex64)
        D.encode_ctrl_host(cell, sf, cfi, [m], tx)
        y = (FLAT_H[:ports, None] * tx).sum(axis=0) + sigma * (rng.standard_normal(G) + 1j * rng.standard_normal(G))
        y = y.astype(np.complex64)[None, :]
        j, _chest, k = _host_job(y, h, sf, noise)
        jobs.append(j), keep.append(k), grids.append((sf, y, D.msg_bits(m)))
    chest = (ChestRes * 2)()
    chest[0].noise_estimate = chest[1].noise_estimate = noise
    ucfg = D.UeDlCfg()
    ucfg.tm, ucfg.dci_common_ss = tm, 1
    ue = UeDl(cell, 1)
    cfis, ctrl, dcis = D.find_dl_dci(ue, jobs, [rnti] * 2, [ucfg] * 2, chest)
    nb_ue = [P.dci_sizeof(f, nprb, ports) for f in P.UE_FORMATS[tm]]
    nb_com = [P.dci_sizeof(P.FORMAT1A, nprb, ports, P.DciCfg(is_not_ue_ss=True)), 0]
    for i, (sf, y, sent) in enumerate(grids):
        assert cfis[i] == cfi and ctrl[i].nof_cce == ncce
        o_llr = P.pdcch_llr(y, h, rg, cfi, cid, sf, noise)
        assert np.array_equal(D.last_llr(ue, i), o_llr)
        count = _check_slots(D.last_candidates(ue, i), o_llr, ncce, sf, rnti, nb_ue, nb_com)
        nloc = len(P.ue_locations(ncce, sf, rnti))
        assert count[0] == 44 - 2 * nloc - len(P.common_locations(ncce)) and count[2] >= 1
        found = P.find_dl_dci(o_llr, ncce, sf, rnti, nprb, ports, tm=tm, dci_common_ss=True)
        assert len(found) >= 1 and np.array_equal(found[0]["bits"], sent)  # (the oracle itself finds what was sent)
        assert ctrl[i].nof_dci == len(found) == len(dcis[i])
        for d, f in zip(dcis[i], found):
            assert (d.format, d.location.L, d.location.ncce) == (f["format"], f["L"], f["ncce"])
            assert (d.type2_alloc.riv, d.tb[0].mcs_idx, d.tb[0].rv) == (f["dci"]["riv"], f["dci"]["tb"][0]["mcs_idx"],
                                                                        f["dci"]["tb"][0]["rv"])
    ue.close()


# ------------------------------------------------------------------ end to end: I/Q -> DCI -> grant -> PDSCH

# (name, nof_prb, ports, rx, tm, dci format, mcs, tbs_alt, cell_id)
CASES = [("tm1_siso_qpsk", 25, 1, 1, 0, P.FORMAT1, 9, False, 3),
         ("tm2_sfbc_16qam", 50, 2, 2, 1, P.FORMAT1, 14, False, 11),
         ("tm3_cdd_64qam", 25, 2, 2, 2, P.FORMAT2A, 20, False, 7),
         ("tm4_sm_256qam", 100, 2, 2, 3, P.FORMAT2, 27, True, 1),
         ("tm2_1a_sfbc", 15, 2, 2, 1, P.FORMAT1A, 12, False, 5)]  # 4-port control regions: the golden cases


def _make_dci(D, cell, fmt, mcs, rnti):
    d = D.DciDl()
    d.rnti, d.format = rnti, fmt
    if fmt == P.FORMAT1A:
        d.alloc_type = D.ALLOC_TYPE2
        d.type2_alloc.riv = D._declare().mi355_ra_type2_to_riv(cell.nof_prb - 2, 1, cell.nof_prb)
        d.tb[0].mcs_idx, d.tb[0].rv, d.tb[0].ndi = mcs, 0, 1
        d.tb[1].mcs_idx, d.tb[1].rv = 0, 1
        return d
    Pg = P.ra_type0_P(cell.nof_prb)
    nb = -(-cell.nof_prb // Pg)
    d.alloc_type = 0
    d.type0_alloc.rbg_bitmask = (1 << nb) - 1
    d.tb[0].mcs_idx, d.tb[0].rv, d.tb[0].ndi = mcs, 0, 1
    if fmt in (P.FORMAT2, P.FORMAT2A):
        d.tb[1].mcs_idx, d.tb[1].rv, d.tb[1].ndi = mcs, 0, 1
        d.tb[1].cw_idx = 1
    else:
        d.tb[1].mcs_idx, d.tb[1].rv = 0, 1
    d.pid = 3
    return d


def _ctrl_subframes(case, sf_idxs=(0, 2, 3, 6, 9)):
    """The control-channel cases' subframes: (cell, rnti, subs, expect), see test_find_and_decode_end_to_end"""
    from srsran_amd import pdcch as D
    from srsran_amd import pdsch as S
    from pdsch_jobs import DevIqSubframe
    name, nprb, ports, nrx, tm, fmt, mcs, alt, cid = case
    rng = np.random.default_rng(len(name) * 7 + nprb)
    cell = S.make_cell(nprb, ports, cid)
    rnti = 0x3C1A
    subs, expect = [], []
    for sf_idx in sf_idxs:
        cfi = 1 if mcs == 27 else 1 + sf_idx % 3  # MCS 27 (256QAM, TBS 97896) only fits a CFI-1 control region
        d = _make_dci(D, cell, fmt, mcs, rnti)
        m = D.pack(cell, d, sf_idx)
        g = D.dci_to_grant(cell, D.unpack(cell, _with_rnti(m, rnti), sf_idx), sf_idx, cfi, tm, alt)
        assert g is not None
        ncce = D.nof_cce(cell, cfi)
        locs = D.ue_locations(ncce, sf_idx, rnti)
        L, n = next((lv for lv in locs if lv[0] == 2), locs[-1])
        m.location = D.DciLocation(L, n)
        m.rnti = rnti
        prb = np.array([[g.prb_idx[s][k] for k in range(nprb)] for s in range(2)], np.uint8)
        ntb = g.nof_tb
        cfg = pc.Cfg(nof_prb=nprb, nof_ports=ports, cell_id=cid, nof_rx=nrx, cfi=cfi, sf_idx=sf_idx, rnti=rnti,
                     scheme=g.tx_scheme, nof_layers=g.nof_layers, pmi=g.pmi,
                     qm=[[1, 2, 4, 6, 8][g.tb[t].mod] for t in range(ntb)], tbs=[g.tb[t].tbs for t in range(ntb)],
                     rv=[0, 0], prb=prb, csi_enable=True)

        def ctrl(tx, m=m, sf_idx=sf_idx, cfi=cfi):
            D.encode_ctrl_host(cell, sf_idx, cfi, [m], tx)

        # 256QAM spatial multiplexing over phy_dl_test's crossed 2x2 channel at 40 dB (as the bench); the other
        # cases over random frequency-selective taps at 32 dB
        chan, snr = ("cross", 40) if mcs == 27 else ("taps", 32)
        iq, payload, _h, _s2 = uc.synth_iq(cfg, rng, snr_db=snr, ctrl=ctrl, channel=chan)
        subs.append(DevIqSubframe(cfg, iq, softbuffers=(2 * len(subs), 2 * len(subs) + 1)))
        expect.append((cfg, payload, g, m))
    return cell, rnti, subs, expect


@pytest.mark.parametrize("full", [False, True], ids=["hits", "full_readback"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_find_and_decode_end_to_end(case, full, monkeypatch):
    """Subframes synthesised with the product's eNodeB-side encoders (DCI pack, PCFICH / PDCCH, PDSCH) through a
    frequency-selective channel; mi355_ue_dl_find_and_decode_batch must find exactly the transmitted DCI at its
    UE-specific candidate, derive the transmitted grant and decode every TB with CRC ok.  The control-channel
    LLRs and blind-search result are checked bit-exactly against the oracle on the GPU's own grids.
    full: the replay reads every subframe's whole candidate array (the overflow path of the compact per-subframe
    hit records, pdcch_runtime.cpp) instead of the records."""
    if full:
        monkeypatch.setenv("MI355_PDCCH_HMAX", "0")
    from srsran_amd import pdcch as D
    from srsran_amd import pdsch as S
    from srsran_amd.dlsch import SoftbufferPool
    from srsran_amd.ue_dl import UeDl, default_chest_cfg
    name, nprb, ports, nrx, tm, fmt, mcs, alt, cid = case
    cell, rnti, subs, expect = _ctrl_subframes(case)
    ue = UeDl(cell, nrx)
    pool = SoftbufferPool(2 * len(subs), max_cb=32)
    ucfg = D.UeDlCfg()
    ucfg.tm, ucfg.use_tbs_index_alt = tm, int(alt)
    cfgs = []
    for s in subs:
        c = S.PdschCfg()
        c.rnti, c.decoder_type, c.csi_enable = rnti, S.MIMO_DECODER_MMSE, 1
        c.softbuffer[0], c.softbuffer[1] = s.job.cfg.softbuffer[0], s.job.cfg.softbuffer[1]
        cfgs.append(c)
    pays = [p for s in subs for p in (s.job.payload[0] or s.payload[0].ptr, s.job.payload[1] or s.payload[0].ptr)]
    sfs, chest, ctrl, dcis, res, got_cfgs = D.find_and_decode(ue, pool, [s.sfjob for s in subs], [ucfg] * len(subs),
                                                             cfgs, default_chest_cfg(), pays)
    for i, (s, (cfg, payload, g, m)) in enumerate(zip(subs, expect)):
        assert sfs[i].cfi == cfg.cfi, (name, i)
        assert ctrl[i].nof_dci == 1, (name, i, ctrl[i].nof_dci)
        d = dcis[i][0]
        # a high-SNR candidate also decodes from the first CCE(s) of its own circular buffer at a lower aggregation
        # level, which the UE searches first (as the reference does): the location is checked against the oracle
        assert d.format == m.format and d.location.ncce == m.location.ncce
        gg = got_cfgs[i].grant
        assert (gg.nof_prb, gg.nof_re, gg.tx_scheme, gg.nof_layers) == (g.nof_prb, g.nof_re, g.tx_scheme, g.nof_layers)
        for t in range(cfg.nof_tb):
            assert res[2 * i + t].crc, (name, i, t)
            assert np.array_equal(s.payload_bytes(t)[: cfg.tbs[t] // 8], payload[t][: cfg.tbs[t] // 8])
        # control stage vs the oracle on the GPU's own grid / estimates / noise
        grids, ces = s.grids(), s.ces()
        rg = P.regs(nprb, ports, cid, 0)
        o_cfi, _c, _l = P.pcfich_decode(grids, ces, rg, cid, cfg.sf_idx, chest[i].noise_estimate)
        assert o_cfi == cfg.cfi
        o_llr = P.pdcch_llr(grids, ces, rg, o_cfi, cid, cfg.sf_idx, chest[i].noise_estimate)
        assert np.array_equal(D.last_llr(ue, i), o_llr)
        found = P.find_dl_dci(o_llr, rg.nof_cce(o_cfi), cfg.sf_idx, rnti, nprb, ports, tm=tm)
        assert [(f["L"], f["ncce"], f["format"]) for f in found] == [(d.location.L, d.location.ncce, d.format)]
        assert np.array_equal(found[0]["bits"], D.msg_bits(m))
    ue.close()


def _with_rnti(m, rnti):
    m.rnti = rnti
    return m


@pytest.mark.parametrize("common_ss", [False, True], ids=["ue_ss", "ue_and_common_ss"])
def test_blind_search_two_dcis(common_ss):
    """Two DL DCIs for the same RNTI in every subframe, at non-overlapping UE-specific locations (the TM's format 2 at
    level 2, a format 1A at level 3): the blind search finds both, in dci_blind_search's order, as the oracle's
    find_dl_dci does on the same LLRs (ue_dl.c:450-550, the reference's overlap test for allocated locations)."""
    from srsran_amd import pdcch as D
    from srsran_amd import pdsch as S
    from srsran_amd.dlsch import SoftbufferPool
    from srsran_amd.ue_dl import UeDl, default_chest_cfg
    from pdsch_jobs import DevIqSubframe
    nprb, ports, nrx, tm, cid, rnti = 50, 2, 2, 3, 11, 0x4602
    cell = S.make_cell(nprb, ports, cid)
    rng = np.random.default_rng(77)
    subs, placed = [], []
    for sf_idx in (1, 4, 7, 8):
        cfi = 3
        ncce = D.nof_cce(cell, cfi)
        locs = D.ue_locations(ncce, sf_idx, rnti)
        la = next(lv for lv in locs if lv[0] == 2)
        lb = next((lv for lv in locs if lv[0] == 3 and (lv[1] + 8 <= la[1] or la[1] + 4 <= lv[1])), None)
        if lb is None:
            continue
        mA = D.pack(cell, _make_dci(D, cell, P.FORMAT2, 14, rnti), sf_idx)
        mB = D.pack(cell, _make_dci(D, cell, P.FORMAT1A, 9, rnti), sf_idx)
        mA.location, mB.location = D.DciLocation(*la), D.DciLocation(*lb)
        mA.rnti = mB.rnti = rnti
        g = D.dci_to_grant(cell, D.unpack(cell, _with_rnti(mA, rnti), sf_idx), sf_idx, cfi, tm, False)
        prb = np.array([[g.prb_idx[s][k] for k in range(nprb)] for s in range(2)], np.uint8)
        cfg = pc.Cfg(nof_prb=nprb, nof_ports=ports, cell_id=cid, nof_rx=nrx, cfi=cfi, sf_idx=sf_idx, rnti=rnti,
                     scheme=g.tx_scheme, nof_layers=g.nof_layers, pmi=g.pmi,
                     qm=[[1, 2, 4, 6, 8][g.tb[t].mod] for t in range(g.nof_tb)],
                     tbs=[g.tb[t].tbs for t in range(g.nof_tb)], rv=[0, 0], prb=prb, csi_enable=True)

        def ctrl(tx, ms=(mA, mB), sf_idx=sf_idx, cfi=cfi):
            D.encode_ctrl_host(cell, sf_idx, cfi, list(ms), tx)

        iq, _payload, _h, _s2 = uc.synth_iq(cfg, rng, snr_db=32, ctrl=ctrl, channel="taps")
        subs.append(DevIqSubframe(cfg, iq, softbuffers=(2 * len(subs), 2 * len(subs) + 1)))
        placed.append((sf_idx, cfi))
    assert len(subs) >= 2
    ucfg = D.UeDlCfg()
    ucfg.tm, ucfg.dci_common_ss = tm, int(common_ss)
    ue = UeDl(cell, nrx)
    pool = SoftbufferPool(2 * len(subs), max_cb=32)
    cfgs = []
    for s in subs:
        c = S.PdschCfg()
        c.rnti, c.decoder_type, c.csi_enable = rnti, S.MIMO_DECODER_MMSE, 1
        c.softbuffer[0], c.softbuffer[1] = s.job.cfg.softbuffer[0], s.job.cfg.softbuffer[1]
        cfgs.append(c)
    pays = [p for s in subs for p in (s.job.payload[0] or s.payload[0].ptr, s.job.payload[1] or s.payload[0].ptr)]
    _sfs, chest, ctrl, dcis, _res, _g = D.find_and_decode(ue, pool, [s.sfjob for s in subs], [ucfg] * len(subs),
                                                          cfgs, default_chest_cfg(), pays)
    rg = P.regs(nprb, ports, cid, 0)
    for i, (s, (sf_idx, cfi)) in enumerate(zip(subs, placed)):
        assert ctrl[i].nof_dci == 2, (i, ctrl[i].nof_dci)
        o_llr = P.pdcch_llr(s.grids(), s.ces(), rg, cfi, cid, sf_idx, chest[i].noise_estimate)
        assert np.array_equal(D.last_llr(ue, i), o_llr)
        found = P.find_dl_dci(o_llr, rg.nof_cce(cfi), sf_idx, rnti, nprb, ports, tm=tm, dci_common_ss=common_ss)
        assert [(f["format"], f["L"], f["ncce"]) for f in found] == [(d.format, d.location.L, d.location.ncce)
                                                                     for d in dcis[i]]
    ue.close()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fft_estimate_find_dci_matches_two_calls(case):
    """mi355_ue_dl_fft_estimate_find_dci_batch (the drop-in's srslte_ue_dl_decode_fft_estimate: estimation and the
    PCFICH / PDCCH stage in one call, noise kept on the device) gives exactly what decode_fft_estimate_batch followed
    by find_dl_dci_batch gives on the same subframes: estimator results, CFIs, control results and DCIs; the hook
    runs once, between the two stages."""
    import ctypes as C

    from srsran_amd import pdcch as D
    from srsran_amd.ue_dl import ChestRes, DlSfJob, UeDl, default_chest_cfg
    name, nprb, ports, nrx, tm, fmt, mcs, alt, cid = case
    cell, rnti, subs, expect = _ctrl_subframes(case)
    jobs = [s.sfjob for s in subs]
    n = len(jobs)
    ucfg = D.UeDlCfg()
    ucfg.tm, ucfg.use_tbs_index_alt = tm, int(alt)
    ue = UeDl(cell, nrx)
    chest_a = ue.fft_estimate(jobs, default_chest_cfg())
    cfis_a, ctrl_a, dcis_a = D.find_dl_dci(ue, jobs, [rnti] * n, [ucfg] * n, chest_a)
    L = D._declare()
    hook_t = C.CFUNCTYPE(None, C.c_void_p)
    calls = []
    hook = hook_t(lambda arg: calls.append(arg))
    L.mi355_ue_dl_fft_estimate_find_dci_batch.argtypes = [
        C.c_void_p, C.POINTER(DlSfJob), C.POINTER(D.DlSfCfg), C.POINTER(D.UeDlCfg), C.POINTER(C.c_uint16),
        C.c_void_p, C.POINTER(ChestRes), C.c_uint32, C.POINTER(D.CtrlRes), C.POINTER(D.DciDl), hook_t, C.c_void_p,
        C.c_void_p]
    sfs = (D.DlSfCfg * n)(*[D.DlSfCfg(j.tti, 0) for j in jobs])
    chest_b, ctrl_b = (ChestRes * n)(), (D.CtrlRes * n)()
    dci_b = (D.DciDl * (n * D.MAX_DCI_MSG))()
    cc = default_chest_cfg()
    assert L.mi355_ue_dl_fft_estimate_find_dci_batch(ue.h, (DlSfJob * n)(*jobs), sfs, (D.UeDlCfg * n)(*([ucfg] * n)),
                                                     (C.c_uint16 * n)(*([rnti] * n)), C.addressof(cc), chest_b, n,
                                                     ctrl_b, dci_b, hook, 1234, None) == 0
    assert calls == [1234]
    assert bytes(chest_b) == bytes(chest_a)
    assert [sfs[i].cfi for i in range(n)] == list(cfis_a) == [e[0].cfi for e in expect]
    assert bytes(ctrl_b) == bytes(ctrl_a)
    for i in range(n):
        got = [bytes(dci_b[i * D.MAX_DCI_MSG + k]) for k in range(max(0, ctrl_b[i].nof_dci))]
        assert got == [bytes(d) for d in dcis_a[i]] and len(got) == 1, (name, i)
    ue.close()
