"""CPU: the host side of the neighbour-cell measurement (include/srsran_amd/cell_meas.h).

mi355_cell_meas_decide through the library: every decision the compiled reference recorded in
tests/golden/cell_meas.npz from the per-subframe values it recorded, with float outputs exactly the reference's; each
stage-3 rule swept over its mild and severe thresholds, one rule at a time; the float64 restatement
(tests/cell_meas_ref.py) against every call of the golden file on regenerated captures; out-of-contract jobs refused by
mi355_cell_meas_check_jobs, the rule the batch calls apply before they launch (srsran_amd/csrc/cell_meas_plan.h, which
tests/test_cell_meas_plan_host.py also checks under sanitizers); refusal of bad arguments."""
import json
import math
import os

import numpy as np
import pytest

import cell_meas_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(HERE, "golden", "cell_meas.npz"))
    assert tuple(z["iv_fields"]) == R.RES_INT and tuple(z["fv_fields"]) == R.RES_FLOAT
    assert tuple(z["sf_fields"]) == ("sf_idx",) + R.SF_FLOAT
    return dict(meta=json.loads(str(z["meta"])), iv=z["iv"], fv=z["fv"], sf=z["sf"])


def _recs(sf_rows):
    from srsran_amd import cell_meas as M
    return [M.CellMeasSf(int(r[0]), *[float(v) for v in r[1:]]) for r in sf_rows]


def test_decide_reproduces_every_recorded_decision(golden):
    from srsran_amd import cell_meas as M
    n = 0
    for meta, iv, fv, sf in zip(golden["meta"], golden["iv"], golden["fv"], golden["sf"]):
        g = dict(zip(R.RES_INT, iv.tolist()))
        if not g["stage1_found"]:
            continue
        n += 1
        peak = g["peak_index"] if g["found"] else 12345
        r = M.decide(_recs(sf[:g["sf_count"]]), meta["cap"]["nof_prb"], peak)
        for f in ("found", "peak_index", "sf_count", "false_count", "false_alarm"):
            assert getattr(r, f) == g[f], (meta, f, getattr(r, f), g[f])
        for i, f in enumerate(R.RES_FLOAT[:4]):
            a, b = np.float32(getattr(r, f)), np.float32(fv[i])
            assert a.tobytes() == b.tobytes() or (np.isnan(a) and np.isnan(b)), (meta, f, a, b)
    assert n >= 30
    kinds = [dict(zip(R.RES_INT, iv.tolist())) for iv in golden["iv"]]
    assert any(k["stage1_found"] and k["false_alarm"] for k in kinds)   # rejected in stage 3
    assert any(k["found"] and k["false_count"] == 1 for k in kinds)     # one mild fault, still found
    assert any(not k["stage1_found"] for k in kinds) and any(k["peak_shifted"] for k in kinds)


def _base():
    """ten subframes 0..9 that raise no rule: SSS ratio 100, false-RSRP ratio 10 dB, no CFO or RSRP spread"""
    sf = []
    for i in range(10):
        full = i % 5 == 0
        sf.append(dict(sf_idx=i, rsrp=1.0, rssi=20.0, cfo=0.0, sss_strength=100.0 if full else 0.0,
                       sss_strength_false=1.0 if full else 0.0, rsrp_false=0.1 if full else 0.0))
    return sf


def _run(sf):
    from srsran_amd import cell_meas as M
    r = M.decide(sf, 6, 4242)
    return r.false_count, r.false_alarm, r.found


def test_decide_base_case_values():
    from srsran_amd import cell_meas as M
    r = M.decide(_base(), 6, 4242)
    assert (r.found, r.peak_index, r.sf_count, r.false_count, r.false_alarm) == (1, 4242, 10, 0, 0)
    assert r.rsrp_dBfs == np.float32(30.0) and r.cfo_Hz == 0.0
    assert abs(r.rssi_dBfs - (10 * math.log10(20.0) + 30)) < 1e-5
    assert abs(r.rsrq_dB - (10 * math.log10(6) + r.rsrp_dBfs - r.rssi_dBfs)) < 1e-5
    # a single subframe that is neither 0 nor 5: the SSS and false-RSRP sums stay empty and raise nothing
    r = M.decide([dict(_base()[3])], 6, 7)
    assert (r.found, r.sf_count, r.false_count) == (1, 1, 0)


@pytest.mark.parametrize("ratio,want", [(15.1, (0, 0, 1)), (14.9, (1, 0, 1)), (1.51, (1, 0, 1)), (1.49, (0, 1, 0))])
def test_decide_sss_rule(ratio, want):
    sf = _base()
    for s in sf:
        if s["sf_idx"] % 5 == 0:
            s["sss_strength"] = ratio * s["sss_strength_false"]
    assert _run(sf) == want


@pytest.mark.parametrize("spread,want", [(999.0, (0, 0, 1)), (1001.0, (1, 0, 1)), (1999.0, (1, 0, 1)),
                                         (2001.0, (0, 1, 0))])
def test_decide_cfo_rule(spread, want):
    sf = _base()
    sf[4]["cfo"] = spread
    assert _run(sf) == want


@pytest.mark.parametrize("db,want", [(5.9, (0, 0, 1)), (6.1, (1, 0, 1)), (9.9, (1, 0, 1)), (10.1, (0, 1, 0))])
def test_decide_rsrp_spread_rule(db, want):
    sf = _base()
    sf[7]["rsrp"] = 10 ** (-db / 10)
    # (the mean falls by at most 0.46 dB, so the false-RSRP ratio stays above 9.5 dB)
    assert _run(sf) == want


@pytest.mark.parametrize("db,want", [(4.1, (0, 0, 1)), (3.9, (1, 0, 1)), (3.1, (1, 0, 1)), (2.9, (0, 1, 0))])
def test_decide_false_rsrp_rule(db, want):
    sf = _base()
    for s in sf:
        if s["sf_idx"] % 5 == 0:
            s["rsrp_false"] = 10 ** (-db / 10)
    assert _run(sf) == want


def test_decide_two_mild_faults_reject():
    from srsran_amd import cell_meas as M
    sf = _base()
    sf[4]["cfo"] = 1001.0
    for s in sf:
        if s["sf_idx"] % 5 == 0:
            s["sss_strength"] = 14.9
    r = M.decide(sf, 6, 4242)
    assert (r.false_count, r.false_alarm, r.found, r.peak_index) == (2, 1, 0, M.NOT_FOUND)
    assert all(math.isnan(v) for v in (r.rsrp_dBfs, r.rssi_dBfs, r.rsrq_dB, r.cfo_Hz))


def test_decide_refuses_bad_arguments():
    import ctypes as C
    from srsran_amd import cell_meas as M
    L = M._declare()
    res, one = M.CellMeasRes(), (M.CellMeasSf * 1)()
    assert L.mi355_cell_meas_decide(one, 1, 6, 0, None) == -2
    assert L.mi355_cell_meas_decide(None, 1, 6, 0, C.byref(res)) == -2
    assert L.mi355_cell_meas_decide(one, 1, 0, 0, C.byref(res)) == -2
    assert L.mi355_cell_meas_decide(one, 0, 6, 0, C.byref(res)) == -2  # no subframe measured: nothing to decide


def test_check_jobs_refuses_out_of_contract_jobs():
    """nsamples = m sf_len with 2 <= m <= max_nof_sf, a cell of the list, an input; one bad job fails the list"""
    from srsran_amd import cell_meas as M
    L, ptr = 1920, 0x1000
    good = (ptr, 6 * L, 3)
    assert M.check_jobs([good] * 5, 6, 12, 8) == 0 and M.check_jobs([], 6, 12, 8) == 0
    for m in range(2, 13):
        assert M.check_jobs([(ptr, m * L, 7)], 6, 12, 8) == 0
    for bad in ((ptr, 0, 3), (ptr, L, 3), (ptr, 6 * L + 1, 3), (ptr, 6 * L - 1, 3), (ptr, 6 * L + 960, 3),
                (ptr, 13 * L, 3), (ptr, 6 * L, 8), (None, 6 * L, 3)):
        for jobs in ([bad], [good, bad], [bad, good], [good] * 7 + [bad]):
            assert M.check_jobs(jobs, 6, 12, 8) == -2, bad
    assert M.check_jobs([(ptr, 6 * L, 0)], 6, 12, 0) == -2       # no cells set
    assert M.check_jobs([(ptr, 3 * 23040, 0)], 100, 3, 1) == 0   # 100 PRB: sf_len 23040
    assert M.check_jobs([(ptr, 3 * 1920, 0)], 100, 3, 1) == -2
    assert M.check_jobs([good], 0, 12, 8) == -2 and M.check_jobs([good], 111, 12, 8) == -2
    assert M.check_jobs([good], 6, 1, 8) == -2
    assert M._declare().mi355_cell_meas_check_jobs(None, 1, 6, 12, 8) == -2


def test_restatement_agrees_with_golden(golden):
    """the float64 restatement on the regenerated captures against every call the compiled reference recorded:
    decisions equal, floats within the recorded deviation itself, a quarter of TOL (0.1 % on top: TOL holds four
    printed digits)"""
    for meta, iv, fv, sf in zip(golden["meta"], golden["iv"], golden["fv"], golden["sf"]):
        cap = dict(meta["cap"], cells=[tuple(c) for c in meta["cap"]["cells"]])
        x = R.synth_capture(**cap)
        cid, ports = meta["cell"]
        w = R.run(R.set_cell(cid, ports, cap["nof_prb"]), x, x.size, cap["nof_prb"])
        got = dict(zip(R.RES_INT, iv.tolist()))
        got.update(zip(R.RES_FLOAT, [float(v) for v in fv]))
        recs = [dict(zip(("sf_idx",) + R.SF_FLOAT, [int(r[0])] + [float(v) for v in r[1:]])) for r in sf[:got["sf_count"]]]
        R.compare(got, w, f"{meta['tag']} cell {cid}", recs, share=0.25 * 1.001)
    assert len(golden["meta"]) == 56
