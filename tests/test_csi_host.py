"""CPU: the host half of include/srsran_amd/csi.h against the recorded reference answers of
tests/golden/csi_feedback.npz -- the numpy restatement (tests/csi_ref.py) within the tolerances the GPU tests use, and
mi355_csi_decide / mi355_cqi_from_snr / mi355_cqi_hl_get_no_subbands through the library: every recorded decision from
the reference's own sums, every CQI threshold at its value and one float below, the 0.1 dB and 20 dB rank rules and
the 17 dB condition-number rule on each side, lists without a positive entry and with NaNs."""
import math

import numpy as np
import pytest

import csi_ref as R

CASES = R.load_cases()
DECISIONS = ("pmi_1l", "pmi_2l", "ri", "pmi", "ri_cn", "cqi")
F = np.float32


def _below(x):
    return np.nextafter(F(x), F(-np.inf))


def _above(x):
    return np.nextafter(F(x), F(np.inf))


def test_fixture_cases():
    """The case list the issue asks for is all there, and the sample counts are the AVX2 build's."""
    names = [c["name"] for c in CASES]
    assert sum(n.startswith("gold") for n in names) == 20
    for prb in (6, 15, 100):
        assert any(n.startswith(f"rand_prb{prb}_") for n in names)
    for n in ("rank1_w0", "rank1_w1", "rank1_w2", "rank1_w3", "unitary", "all_zero", "nan_sample", "outliers_m40_41"):
        assert n in names
    assert [(R.n_groups(p), 8 * R.n_groups(p), R.n_cn(p)) for p in (6, 15, 25, 50, 75, 100)] == [
        (5, 40, 42), (13, 104, 105), (21, 168, 175), (43, 344, 350), (65, 520, 525), (87, 696, 700)]
    for c in CASES:
        assert c["samples"].shape == (2, 2, R.n_cn(c["nof_prb"]))
        assert c["cn_count"] == (R.n_cn(6) - 1 if c["name"] == "nan_sample" else R.n_cn(c["nof_prb"]))


def test_restatement_against_reference():
    """tests/csi_ref.sums (exact divisions, the reference's summation order) against the recorded AVX2 outputs within
    sinr_1l 1e-5 mean ||H||_F^2 / noise, sinr_2l 1.5e-3 (ref + 2), cn 1e-3 dB, NaN for NaN and infinity for infinity.
    Measured here: sinr_1l equal bit for bit, sinr_2l up to 0.24 of its bound (the reference's two chained
    _mm256_rcp_ps), cn up to 0.004 of its bound -- none of the bounds is too tight for the reference itself."""
    worst = dict(sinr_1l=0.0, sinr_2l=0.0, cn=0.0)
    for c in CASES:
        s, tol = R.sums(c["samples"], c["nof_prb"], c["noise"]), R.tolerances(c)
        assert s["cn_count"] == c["cn_count"], c["name"]
        for k in worst:
            assert R.same_class(s[k], c[k], tol[k]), (c["name"], k, s[k], c[k], tol[k])
            with np.errstate(all="ignore"):
                rel = np.abs(np.asarray(s[k], np.float64) - np.asarray(c[k], np.float64)) / np.asarray(tol[k], np.float64)
            if np.all(np.isfinite(rel)):
                worst[k] = max(worst[k], float(np.max(rel)))
    print("restatement vs reference, largest |delta| / tolerance:", worst)


def test_restatement_decisions_and_exclusion_cap():
    """The restated decisions from the restated sums equal the recorded ones outside the exclusion band (recorded
    values within twice the tolerance of a tie or a threshold), and at most 5 % of the cases have an excluded decision."""
    nexcl = 0
    for c in CASES:
        s = R.sums(c["samples"], c["nof_prb"], c["noise"])
        d = R.decide(s["sinr_1l"], s["sinr_2l"], s["cn"], c["offset"])
        ex = R.excluded(c)
        nexcl += bool(ex)
        for k in DECISIONS:
            if k not in ex:
                assert d[k] == c[k], (c["name"], k, d[k], c[k])
    assert nexcl <= 0.05 * len(CASES), (nexcl, len(CASES))


def test_outliers_enter_the_condition_number_only():
    """6 PRB: the samples m = 40, 41 lie past the last whole group of eight; the recorded SINRs are those of the case
    without them, the recorded condition number is not."""
    c = next(c for c in CASES if c["name"] == "outliers_m40_41")
    assert np.abs(c["samples"][:, :, 40:]).min() > 200 and np.abs(c["samples"][:, :, :40]).max() < 10
    calm = dict(c, samples=c["samples"].copy())
    calm["samples"][:, :, 40:] = c["samples"][:, :, 38:40]
    s = R.sums(calm["samples"], 6, c["noise"])
    tol = R.tolerances(c)
    assert R.same_class(s["sinr_1l"], c["sinr_1l"], tol["sinr_1l"]) and R.same_class(s["sinr_2l"], c["sinr_2l"], tol["sinr_2l"])
    assert abs(float(s["cn"]) - float(c["cn"])) > 0.1


# ------------------------------------------------------------------ the library's host functions

def test_decide_reproduces_every_recorded_decision():
    """mi355_csi_decide fed the reference's own recorded lists and condition number: every decision of every case,
    no exclusions; sinr_db bit for bit (log10f is the same libm's).  What this pins against the reference itself:
    pmi_1l and pmi_2l (srslte_precoding_pmi_select's own argmaxes) and the SNR -> CQI table (srslte_cqi_from_snr).
    The recorded ri, pmi, sinr_db and ri_cn come from the rule of select_ri_pmi / srslte_ue_dl_select_ri as
    tests/golden/csi_ref_wrap.c states it (the reference's functions are static or need a whole ue_dl object): for
    those this is one statement of the rule against another, compiled beside the reference with its flags."""
    from srsran_amd import csi
    for c in CASES:
        r = csi.decide(c["sinr_1l"], c["sinr_2l"], float(c["cn"]), float(c["noise"]), float(c["offset"]), c["cn_count"])
        for k in DECISIONS:
            assert getattr(r, k) == c[k], (c["name"], k, getattr(r, k), c[k])
        assert F(r.sinr_db).tobytes() == F(c["sinr_db"]).tobytes() or (math.isnan(r.sinr_db) and math.isnan(c["sinr_db"]))
        # the inputs stay as they were
        assert np.array_equal(np.array(r.sinr_1l[:], F), c["sinr_1l"], equal_nan=True) and r.cn_count == c["cn_count"]


def test_decide_ignores_the_noise_argument():
    from srsran_amd import csi
    c = CASES[3]
    a = csi.decide(c["sinr_1l"], c["sinr_2l"], float(c["cn"]), 0.0, 1.0)
    b = csi.decide(c["sinr_1l"], c["sinr_2l"], float(c["cn"]), float("nan"), 1.0)
    assert bytes(a) == bytes(b)


def test_cqi_thresholds():
    """Every threshold of cqi.c:589 as a float: at the value the CQI is reached, one float below it is not; NaN and
    -inf give 0, +inf 15.  The library equals the restatement over a sweep."""
    from srsran_amd import csi
    for i, t in enumerate(R.CQI_TABLE):
        assert csi.cqi_from_snr(float(t)) == i + 1
        assert csi.cqi_from_snr(float(_below(t))) == i
    assert csi.cqi_from_snr(float("nan")) == 0 and csi.cqi_from_snr(float("-inf")) == 0
    assert csi.cqi_from_snr(float("inf")) == 15 and csi.cqi_from_snr(-3.0) == 0
    for x in np.linspace(-10, 40, 1001).astype(F):
        assert csi.cqi_from_snr(float(x)) == R.cqi_from_snr(x)
    # through mi355_csi_decide: sinr_db + offset is one float addition
    for i, t in enumerate(R.CQI_TABLE):
        lin = F(10.0)  # 10 dB exactly
        r = csi.decide([lin, 0, 0, 0], [0, 0], 30.0, 0.1, float(F(t) - F(10)))
        assert r.sinr_db == 10.0 and r.cqi == R.cqi_from_snr(F(10) + (F(t) - F(10)))


@pytest.mark.parametrize("nof_prb", range(1, 112))
def test_no_subbands(nof_prb):
    """36.213 Table 7.2.1-3: k = 4 for 7..26 PRB (the reference's bounds), 6 up to 63, 8 up to 110; N = ceil(nof_prb / k),
    0 below 7 PRB and above 110."""
    from srsran_amd import csi
    k = 0 if nof_prb < 7 else 4 if nof_prb <= 26 else 6 if nof_prb <= 63 else 8 if nof_prb <= 110 else 0
    assert csi.cqi_hl_get_no_subbands(nof_prb) == (-(-nof_prb // k) if k else 0)


def _lin(db):
    return F(10.0 ** (float(db) / 10.0))


def _lib_db(csi, x):
    """10 log10f(x) as the library computes it"""
    return csi.decide([x, 0, 0, 0], [0, 0], 30.0).sinr_db


def _first_float(pred, lo, hi):
    """the smallest float32 in (lo, hi] for which pred holds (pred monotonic, false at lo, true at hi)"""
    a, b = int(F(lo).view(np.uint32)), int(F(hi).view(np.uint32))
    assert not pred(F(lo)) and pred(F(hi))
    while b - a > 1:
        m = (a + b) // 2
        if pred(np.uint32(m).view(F)):
            b = m
        else:
            a = m
    return np.uint32(b).view(F)


def test_rank_rule_point_one_db():
    """Below 20 dB ri = 1 replaces ri = 0 only when its SINR is more than 0.1 dB better, compared in double as the
    reference's `best + 0.1`: the first float whose dB value exceeds the bound is accepted, the float below it is not."""
    from srsran_amd import csi
    s1 = _lin(12.0)
    base = csi.decide([0, s1, 0, 0], [0, 0], 30.0)
    assert (base.ri, base.pmi, base.pmi_1l) == (0, 1, 1)
    x = _first_float(lambda v: float(_lib_db(csi, v)) > float(base.sinr_db) + 0.1, _lin(12.0), _lin(12.2))
    r = csi.decide([0, s1, 0, 0], [0, x], 30.0)
    assert (r.ri, r.pmi, r.pmi_2l) == (1, 1, 1) and r.sinr_db == _lib_db(csi, x)
    r = csi.decide([0, s1, 0, 0], [0, _below(x)], 30.0)
    assert (r.ri, r.pmi) == (0, 1) and r.sinr_db == base.sinr_db


def test_rank_rule_twenty_db():
    """Above 20 dB the 2-layer choice wins even when the 1-layer SINR is far better; at 20 dB and below it does not."""
    from srsran_amd import csi
    hi = _lin(33.0)
    x = _first_float(lambda v: float(_lib_db(csi, v)) > 20.0, _lin(19.9), _lin(20.1))
    r = csi.decide([hi, 0, 0, 0], [x, 0], 30.0)
    assert (r.ri, r.pmi) == (1, 0) and r.sinr_db > 20.0
    r = csi.decide([hi, 0, 0, 0], [_below(x), 0], 30.0)
    assert (r.ri, r.pmi) == (0, 0) and r.sinr_db == _lib_db(csi, hi)


def test_condition_number_rule():
    from srsran_amd import csi
    assert csi.decide([1, 0, 0, 0], [1, 0], float(_below(17.0))).ri_cn == 1
    assert csi.decide([1, 0, 0, 0], [1, 0], 17.0).ri_cn == 0
    assert csi.decide([1, 0, 0, 0], [1, 0], float("-inf")).ri_cn == 1
    assert csi.decide([1, 0, 0, 0], [1, 0], float("nan")).ri_cn == 0


def test_no_positive_entry_and_nan():
    """The argmax starts from max = 0.0 with a strict >: lists without a positive entry or with a NaN in front leave the
    PMI at 0; no rank is accepted when both candidates are -inf or NaN, so sinr_db = -inf and the CQI is 0."""
    from srsran_amd import csi
    nan = float("nan")
    r = csi.decide([0, 0, 0, 0], [0, 0], 5.0)
    assert (r.pmi_1l, r.pmi_2l, r.ri, r.pmi, r.cqi) == (0, 0, 0, 0, 0) and r.sinr_db == float("-inf")
    r = csi.decide([-1, -2, -3, -4], [nan, nan], 5.0, offset=100.0)
    assert (r.pmi_1l, r.pmi_2l, r.ri, r.pmi, r.cqi) == (0, 0, 0, 0, 0) and r.sinr_db == float("-inf")
    r = csi.decide([nan, nan, nan, nan], [nan, nan], nan)
    assert (r.pmi_1l, r.pmi_2l, r.ri, r.pmi, r.cqi, r.ri_cn) == (0, 0, 0, 0, 0, 0) and r.sinr_db == float("-inf")
    # a NaN that is not the running maximum does not stop later entries
    r = csi.decide([nan, 2.0, nan, 3.0], [nan, 1.0], 5.0)
    assert (r.pmi_1l, r.pmi_2l) == (3, 1)
    # the 1-layer list dead, the 2-layer alive: ri = 1 is the first accepted candidate
    r = csi.decide([0, 0, 0, 0], [0.5, 2.0], 5.0)
    assert (r.ri, r.pmi) == (1, 1) and abs(r.sinr_db - 10 * math.log10(2.0)) < 1e-5


def test_struct_layout():
    """CsiRes mirrors mi355_csi_res_t: 15 four-byte members, no padding."""
    import ctypes as C
    from srsran_amd import csi
    assert C.sizeof(csi.CsiRes) == 60
    assert csi.CsiRes.cn.offset == 24 and csi.CsiRes.pmi_1l.offset == 32 and csi.CsiRes.cqi.offset == 56
