"""numpy float32 restatement of the UE's channel-state feedback as the reference's AVX2 build computes it
(srslte_precoding_pmi_select, mimo/precoding.c:2363-2478 and :2609-2810; srslte_precoding_cn, :2813-2854 over
srslte_mat_2x2_cn, utils/mat.c:127-159; select_ri_pmi / srslte_ue_dl_select_ri, ue/ue_dl.c:791-884;
srslte_cqi_from_snr, phch/cqi.c:589-602), the loader of tests/golden/csi_feedback.npz, and the tolerances and
exclusion rule the CPU and GPU tests share.

Every product, sum and division is one float32 operation in the reference's order (numpy does not contract), including
the per-group pairwise sums of _mm256_hadd_ps; the one difference is 1 / x: exact here, _mm256_rcp_ps there."""
from __future__ import annotations

import math
import os

import numpy as np

F = np.float32
STEP, SIMD = 24, 8
CQI_TABLE = np.array([1.95, 4, 6, 8, 10, 11.95, 14.05, 16, 17.9, 20.9, 22.5, 24.75, 25.5, 27.30, 29], np.float32)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "csi_feedback.npz")
POISON = np.complex64(3e4 - 7e4j)  # what the estimates between two samples hold: never read


def n_cn(nof_prb: int) -> int:
    return 14 * 12 * nof_prb // STEP


def n_groups(nof_prb: int) -> int:
    return (14 * 12 * nof_prb - STEP * SIMD) // (STEP * SIMD) + 1


def bound_noise(noise) -> np.float32:
    """precoding.c:2796: not normal, or below 1e-9 -> 1e-9"""
    n = F(noise)
    normal = np.isfinite(n) and abs(n) >= np.finfo(np.float32).tiny
    return F(1e-9) if (not normal or n < F(1e-9)) else n


# ------------------------------------------------------------------ complex helpers on (re, im) float32 pairs

def _c(z):
    z = np.asarray(z, np.complex64)
    return z.real.astype(F), z.imag.astype(F)


def _add(a, b):
    return a[0] + b[0], a[1] + b[1]


def _sub(a, b):
    return a[0] - b[0], a[1] - b[1]


def _conj(a):
    return a[0], -a[1]


def _mulj(a):
    return -a[1], a[0]


def _prod(a, b):
    return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


def _tree8(v):
    """three rounds of _mm256_hadd_ps: adjacent pairs"""
    v = v[..., 0::2] + v[..., 1::2]
    v = v[..., 0::2] + v[..., 1::2]
    return (v[..., 0::2] + v[..., 1::2])[..., 0]


def _seq_sum(v):
    acc = F(0)
    for x in v:
        acc = F(acc + x)
    return acc


def _rows(h):
    """h (2 ports, 2 rx, n) samples -> B = W' H' H rows per 1-layer codebook index: (b0[4], b1[4]), and the h parts"""
    h00, h01, h10, h11 = _c(h[0, 0]), _c(h[1, 0]), _c(h[0, 1]), _c(h[1, 1])
    q00, q01, q10, q11 = _conj(h00), _conj(h01), _conj(h10), _conj(h11)
    a0 = [_add(q00, q01), _sub(q00, q01), _sub(q00, _mulj(q01)), _add(q00, _mulj(q01))]
    a1 = [_add(q10, q11), _sub(q10, q11), _sub(q10, _mulj(q11)), _add(q10, _mulj(q11))]
    b0 = [_add(_prod(a0[i], h00), _prod(a1[i], h10)) for i in range(4)]
    b1 = [_add(_prod(a0[i], h01), _prod(a1[i], h11)) for i in range(4)]
    return b0, b1


def _gamma_2l(c00, c01, c10, c11, noise):
    q = F(0.25)
    c00, c01, c10, c11 = [(c[0] * q, c[1] * q) for c in (c00, c01, c10, c11)]
    c00 = (c00[0] + noise, c00[1] + F(0))
    c11 = (c11[0] + noise, c11[1] + F(0))
    det = _prod(c00, c11)[0] - _prod(c01, c10)[0]
    det = np.where(det < F(1e-10), F(1e-10), det)
    inv = noise * (F(1) / det)
    g0 = F(1) / (c00[0] * inv) - F(1)
    g1 = F(1) / (c11[0] * inv) - F(1)
    g0 = np.where(g0 < F(1e-9), F(1e-9), g0)
    g1 = np.where(g1 < F(1e-9), F(1e-9), g1)
    return g0.astype(F), g1.astype(F)


def sums(samples: np.ndarray, nof_prb: int, noise) -> dict:
    """samples (2 ports, 2 rx, 7 nof_prb) complex64 = the estimates at j = 24 m -> sinr_1l, sinr_2l, cn, cn_count"""
    with np.errstate(all="ignore"):
        noise = bound_noise(noise)
        G = n_groups(nof_prb)
        h = np.asarray(samples, np.complex64)[:, :, : SIMD * G]
        b0, b1 = _rows(h)
        re_c = [_add(b0[0], b1[0])[0], _sub(b0[1], b1[1])[0], _add(b0[2], _mulj(b1[2]))[0], _sub(b0[3], _mulj(b1[3]))[0]]
        s1 = np.zeros(4, F)
        for i in range(4):
            g = (re_c[i] * F(0.5)).reshape(G, SIMD)
            s1[i] = _seq_sum(_tree8(g) / F(SIMD)) / F(noise * F(G))
        s2 = np.zeros(2, F)
        for i, (u, v) in enumerate(((0, 1), (2, 3))):
            rot = (lambda z: z) if i == 0 else _mulj
            g0, g1 = _gamma_2l(_add(b0[u], rot(b1[u])), _sub(b0[u], rot(b1[u])), _add(b0[v], rot(b1[v])),
                               _sub(b0[v], rot(b1[v])), noise)
            g0, g1 = g0.reshape(G, SIMD), g1.reshape(G, SIMD)
            # hadd(gamma0, gamma1): the pairs of gamma0, then the pairs of gamma1
            first = np.concatenate([g0[:, 0::2] + g0[:, 1::2], g1[:, 0::2] + g1[:, 1::2]], axis=1)
            s2[i] = _seq_sum(_tree8(first) / F(SIMD)) / F(G)
        cn, count = cond_number(samples)
    return dict(sinr_1l=s1, sinr_2l=s2, cn=cn, cn_count=count)


def cond_number(samples: np.ndarray):
    """srslte_precoding_2x2_cn_gen over every sample: (mean cn in dB or 0, counted samples)"""
    with np.errstate(all="ignore"):
        h = np.asarray(samples, np.complex64)
        h00, h01, h10, h11 = _c(h[0, 0]), _c(h[1, 0]), _c(h[0, 1]), _c(h[1, 1])
        a00 = h00[0] * h00[0] + h01[0] * h01[0] + h00[1] * h00[1] + h01[1] * h01[1]
        a01 = _add(_prod(h00, _conj(h10)), _prod(h01, _conj(h11)))
        a11 = h10[0] * h10[0] + h11[0] * h11[0] + h10[1] * h10[1] + h11[1] * h11[1]
        b = a00 + a11
        c = a00 * a11 - (a01[0] * a01[0] + a01[1] * a01[1])
        sqr = np.sqrt(b * b - F(4) * c)
        xmax, xmin = b + sqr, b - sqr
        ok = np.isfinite(xmin) & np.isfinite(xmax)
        xmin = np.where(xmin > F(1e-9), xmin, F(1e-9)).astype(F)
        xmax = np.where(xmax < F(1e+9), xmax, F(1e+9)).astype(F)
        cn = (F(10) * np.log10((xmax / xmin).astype(F)).astype(F)).astype(F)
        count = int(ok.sum())
        return (F(_seq_sum(cn[ok]) / F(count)) if count else F(0)), count


# ------------------------------------------------------------------ decisions

def argmax_from_zero(lst) -> int:
    best, at = F(0), 0
    for i, x in enumerate(lst):
        if x > best:
            best, at = x, i
    return at


def to_db(x) -> np.float32:
    x = float(x)
    if math.isnan(x) or x < 0:
        return F(np.nan)
    return F(10) * F(math.log10(x)) if x > 0 else F(-np.inf)


def cqi_from_snr(snr) -> int:
    for cqi in range(14, -1, -1):
        if F(snr) >= CQI_TABLE[cqi]:
            return cqi + 1
    return 0


def decide(sinr_1l, sinr_2l, cn, offset=0.0) -> dict:
    p1, p2 = argmax_from_zero(sinr_1l), argmax_from_zero(sinr_2l)
    best, pmi, ri = F(-np.inf), 0, 0
    for this_ri, (p, lst) in enumerate(((p1, sinr_1l), (p2, sinr_2l))):
        db = to_db(lst[p])
        if float(db) > float(best) + 0.1 or float(db) > 20.0:
            best, pmi, ri = db, p, this_ri
    return dict(pmi_1l=p1, pmi_2l=p2, ri=ri, pmi=pmi, sinr_db=best, ri_cn=1 if F(cn) < F(17) else 0,
                cqi=cqi_from_snr(F(best + F(offset))))


# ------------------------------------------------------------------ fixture

def load_cases() -> list[dict]:
    """The recorded cases: name, nof_prb, noise, offset, samples (2, 2, 7 nof_prb) and the reference's outputs."""
    z = np.load(FIXTURE, allow_pickle=False)
    names = [str(s) for s in z["names"]]
    out = []
    for i, name in enumerate(names):
        c = dict(name=name, nof_prb=int(z["nof_prb"][i]), noise=F(z["noise"][i]), offset=F(z["offset"][i]),
                 samples=z[f"h_{i}"], sinr_1l=z["sinr_1l"][i], sinr_2l=z["sinr_2l"][i], cn=F(z["cn"][i]),
                 cn_count=int(z["cn_count"][i]), sinr_db=F(z["sinr_db"][i]))
        for k in ("pmi_1l", "pmi_2l", "ri", "pmi", "ri_cn", "cqi"):
            c[k] = int(z[k][i])
        out.append(c)
    return out


def grid_of(case: dict, rows: int = 14) -> np.ndarray:
    """(2 ports, 2 rx, rows * 12 nof_prb) estimates: the recorded samples at j = 24 m, POISON between them"""
    nre = 12 * case["nof_prb"]
    g = np.full((2, 2, 14 * nre), POISON, np.complex64)
    g[:, :, ::STEP] = case["samples"]
    return g[:, :, : rows * nre]


# ------------------------------------------------------------------ tolerances and exclusions

def tolerances(case: dict) -> dict:
    """sinr_1l: 1e-5 mean ||H||_F^2 / noise (over the PMI samples); sinr_2l: 1.5e-3 (ref + 2) per entry; cn: 1e-3 dB"""
    with np.errstate(all="ignore"):
        G = n_groups(case["nof_prb"])
        h = case["samples"][:, :, : SIMD * G].astype(np.complex128)
        fro = float(np.mean(np.sum(np.abs(h) ** 2, axis=(0, 1))))
        return dict(sinr_1l=np.full(4, 1e-5 * fro / float(bound_noise(case["noise"]))),
                    sinr_2l=1.5e-3 * (case["sinr_2l"].astype(np.float64) + 2.0), cn=1e-3)


def same_class(got, ref, tol) -> bool:
    """|got - ref| <= tol, a NaN for a NaN, an infinity for the infinity of the same sign"""
    got, ref = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(ref, np.float64))
    tol = np.broadcast_to(np.asarray(tol, np.float64), ref.shape)
    for g, r, t in zip(got, ref, tol):
        if math.isnan(r):
            ok = math.isnan(g)
        elif math.isinf(r):
            ok = g == r
        else:
            ok = math.isfinite(g) and abs(g - r) <= t
        if not ok:
            return False
    return True


def _db_slack(x, tol, k=2) -> float:
    """how far 10 log10 moves when x moves by k tol"""
    x, tol = float(x), float(tol)
    if not math.isfinite(x) or not math.isfinite(tol) or x <= 0:
        return 0.0
    lo = x - k * tol
    return max(10 * math.log10((x + k * tol) / x), 10 * math.log10(x / lo) if lo > 0 else math.inf)


def sinr_db_tol(case: dict) -> float:
    """the tolerance of the selected SINR entry carried through 10 log10, plus one float rounding of the dB value"""
    tol = tolerances(case)
    if case["ri"] == 1:
        x, t = case["sinr_2l"][case["pmi_2l"]], tol["sinr_2l"][case["pmi_2l"]]
    else:
        x, t = case["sinr_1l"][case["pmi_1l"]], tol["sinr_1l"][0]
    return _db_slack(x, t, 1) + 1e-5


def excluded(case: dict) -> set:
    """The decisions of a case that a value within its tolerance of the recorded one could take differently: the
    recorded values lie within twice the tolerance of a tie (argmax) or of a threshold (0.1 dB, 20 dB, 17 dB, a CQI
    step).  Comparisons with a NaN are false on both sides and exclude nothing."""
    tol = tolerances(case)
    out = set()

    def tie(lst, t):
        v = np.asarray(lst, np.float64)
        if np.isnan(v).any():
            return False
        o = np.argsort(-v, kind="stable")
        top, second = v[o[0]], max(v[o[1]], 0.0)  # the start value 0.0 competes too
        if math.isinf(top):
            return False
        return top - second <= 2 * float(np.max(t))

    if tie(case["sinr_1l"], tol["sinr_1l"]):
        out.add("pmi_1l")
    if tie(case["sinr_2l"], tol["sinr_2l"]):
        out.add("pmi_2l")
    s1, s2 = case["sinr_1l"][case["pmi_1l"]], case["sinr_2l"][case["pmi_2l"]]
    d1, d2 = float(to_db(s1)), float(to_db(s2))
    e1, e2 = _db_slack(s1, tol["sinr_1l"][0]), _db_slack(s2, tol["sinr_2l"][case["pmi_2l"]])
    if math.isfinite(d1) and math.isfinite(d2):
        if abs(d2 - (d1 + 0.1)) <= e1 + e2 or abs(d2 - 20.0) <= e2:
            out.add("ri")
    if "ri" in out or ("pmi_1l" in out and case["ri"] == 0) or ("pmi_2l" in out and case["ri"] == 1):
        out.add("pmi")
    e = e2 if case["ri"] == 1 else e1
    snr = float(case["sinr_db"]) + float(case["offset"])
    if "ri" in out or (math.isfinite(snr) and np.any(np.abs(CQI_TABLE.astype(np.float64) - snr) <= e)):
        out.add("cqi")
    if math.isfinite(float(case["cn"])) and abs(float(case["cn"]) - 17.0) <= 2 * tol["cn"]:
        out.add("ri_cn")
    return out
