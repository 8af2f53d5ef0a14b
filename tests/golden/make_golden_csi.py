#!/usr/bin/env python3
"""Record tests/golden/csi_feedback.npz: the reference's channel-state feedback (srslte_precoding_pmi_select,
srslte_precoding_cn, srslte_cqi_from_snr, and select_ri_pmi's decisions around them) for the cases the CSI tests run.

    python tests/golden/make_golden_csi.py

Needs the reference tree: tests/golden/csi_ref_wrap.c is compiled together with the reference's precoding.c, mat.c,
cqi.c and what they call, read where they lie, with the flags oracle/Makefile gives the reference (REF_OPT, ARCH,
REF_DEFS: the AVX2 build), into a temporary directory that is removed afterwards.

Per case the fixture holds the inputs -- nof_prb, the noise estimate, the SNR -> CQI offset and the estimates at the
sampled positions j = 24 m, (2 ports, 2 rx, 7 nof_prb) complex64 (the estimates in between are never read; the grids
the reference ran on held tests/csi_ref.py's POISON there) -- and the outputs: sinr_1l[4], sinr_2l[2], pmi_1l, pmi_2l,
cn, ri, pmi, sinr_db, ri_cn, cqi.  Of these, sinr_1l, sinr_2l, pmi_1l, pmi_2l and cn are the reference's own output
(srslte_precoding_pmi_select, srslte_precoding_cn).  ri, pmi, sinr_db and ri_cn are NOT: select_ri_pmi is a static
function of ue_dl.c, and csi_ref_wrap.c states its rule in this project's words around the reference's pmi_select,
compiled with the reference's flags; cqi is the reference's srslte_cqi_from_snr applied to that sinr_db.  cn_count,
which srslte_precoding_cn does not return, is the number of samples the restatement counts (all of them except in the
NaN case).

Cases: the 20 constant channels and noise values of the reference's pmi_select_test (6 PRB); seeded random 2x2
channels at 6, 15 and 100 PRB at SNRs between -5 and 35 dB (a draw whose reference values fall within the exclusion
band of a tie or threshold is replaced by the next seed); rank-1 channels matched to each codebook vector; a scaled
unitary channel; an all-zero channel with zero noise; a NaN in a sampled estimate; 6 PRB with large outliers at the
samples m = 40, 41, which enter the condition number only.

The script asserts that the reference passes its own pmi_select_test bounds, that the restatement agrees with the
reference within the tolerances of tests/csi_ref.py, and that at most 5 % of the cases have a decision excluded from
the exact comparison."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import csi_ref as R  # noqa: E402

REF = "/root/reference/lib"
GOLD_H = os.path.join(REF, "src/phy/mimo/test/pmi_select_test.h")
REF_SRC = ["src/phy/mimo/precoding.c", "src/phy/utils/mat.c", "src/phy/phch/cqi.c", "src/phy/utils/vector.c",
           "src/phy/utils/vector_simd.c", "src/phy/utils/bit.c", "src/phy/utils/debug.c"]


def _make_var(name: str) -> list[str]:
    text = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    m = re.search(r"^" + name + r"\s*\??=\s*(.*)$", text, flags=re.M)
    assert m, name
    return m.group(1).split()


def build_ref(tmp: str) -> C.CDLL:
    so = os.path.join(tmp, "libcsi_ref.so")
    vs = os.path.join(tmp, "exports.map")
    with open(vs, "w") as f:
        f.write("{ global: csiwrap_*; local: *; };\n")
    # cqi.c includes the umbrella srslte/srslte.h, which wants the CMake-generated srslte/version.h (and FFTW); it
    # also includes every header it uses by name, so an empty srslte/srslte.h earlier on the include path serves
    os.makedirs(os.path.join(tmp, "inc", "srslte"))
    open(os.path.join(tmp, "inc", "srslte", "srslte.h"), "w").close()
    cmd = (["gcc"] + _make_var("REF_OPT") + ["-fPIC", "-w"] + _make_var("ARCH") + _make_var("REF_DEFS") +
           [f"-I{tmp}/inc", f"-I{REF}/include", "-ffunction-sections", "-shared", "-Wl,--gc-sections",
            f"-Wl,--version-script={vs}", "-o", so, os.path.join(HERE, "csi_ref_wrap.c")] + [os.path.join(REF, s) for s in REF_SRC] + ["-lm"])
    subprocess.run(cmd, check=True)
    und = subprocess.run(["nm", "-D", "--undefined-only", so], check=True, capture_output=True, text=True).stdout
    assert "srslte_" not in und, und
    L = C.CDLL(so)
    fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    L.csiwrap_pmi_select.argtypes = [fp] * 4 + [C.c_uint32, C.c_float, C.c_int, u32p, fp]
    L.csiwrap_cn.argtypes = [fp] * 4 + [C.c_uint32, fp]
    L.csiwrap_decide.argtypes = [fp] * 4 + [C.c_uint32] + [C.c_float] * 3 + [u32p, u32p, fp, u32p, u32p]
    return L


def run_ref(L, case: dict) -> dict:
    g = R.grid_of(case)
    ptr = [g[p, r].ctypes.data_as(C.POINTER(C.c_float)) for p in range(2) for r in range(2)]
    n = g.shape[2]
    out = {}
    for layers, key, k in ((1, "sinr_1l", 4), (2, "sinr_2l", 2)):
        pmi, lst = C.c_uint32(), (C.c_float * 4)()
        assert L.csiwrap_pmi_select(*ptr, n, float(case["noise"]), layers, C.byref(pmi), lst) == k
        out[key], out["pmi_%dl" % layers] = np.array(lst[:k], np.float32), pmi.value
    cn = C.c_float()
    assert L.csiwrap_cn(*ptr, n, C.byref(cn)) == 0
    out["cn"] = np.float32(cn.value)
    ri, pmi, ri_cn, cqi, db = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_float()
    assert L.csiwrap_decide(*ptr, n, float(case["noise"]), cn.value, float(case["offset"]), C.byref(ri), C.byref(pmi),
                            C.byref(db), C.byref(ri_cn), C.byref(cqi)) == 0
    out.update(ri=ri.value, pmi=pmi.value, sinr_db=np.float32(db.value), ri_cn=ri_cn.value, cqi=cqi.value)
    return out


def gold_cases() -> list[dict]:
    """h[2][2] and n of the reference's pmi_select_test, with its expected values"""
    text = open(GOLD_H).read()
    num = r"([+-]?[0-9.]+(?:e[+-]?[0-9]+)?)f?"
    out = []
    for blk in re.findall(r"\{\s*/\* Test case \d+ \*/(.*?)\.k\s*=\s*" + num, text, flags=re.S):
        body, k = blk
        hm = re.search(r"\.h\s*=\s*\{(.*?)\}\s*,\s*\.n", body, flags=re.S).group(1)
        cplx = re.findall(num + r"\s*([+-])\s*" + num + r"\s*\*\s*_Complex_I", hm)
        if cplx:
            vals = [float(a) + (1 if s == "+" else -1) * float(b) * 1j for a, s, b in cplx]
        else:
            vals = [float(x) for x in re.findall(num, hm)]
        assert len(vals) == 4, hm
        n = float(re.search(r"\.n\s*=\s*" + num, body).group(1))
        s1 = [float(x) for x in re.findall(num, re.search(r"\.snri_1l\s*=\s*\{(.*?)\}", body).group(1))]
        s2 = [float(x) for x in re.findall(num, re.search(r"\.snri_2l\s*=\s*\{(.*?)\}", body).group(1))]
        pm = [int(x) for x in re.findall(r"\d+", re.search(r"\.pmi\s*=\s*\{(.*?)\}", body).group(1))]
        # gold->h[i][j] is the reference's h[i][j]: [port][rx]
        out.append(dict(h=np.array(vals, np.complex64).reshape(2, 2), n=n, s1=s1, s2=s2, pmi=pm, k=float(k)))
    assert len(out) == 20
    return out


W2 = [1, -1, 1j, -1j]


def _cn(rng, shape, scale=1.0):
    return (scale * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)).astype(np.complex64)


def make_cases() -> list[dict]:
    cases = []

    def add(name, nof_prb, noise, samples, offset=0.0):
        assert samples.shape == (2, 2, R.n_cn(nof_prb))
        cases.append(dict(name=name, nof_prb=nof_prb, noise=np.float32(noise), offset=np.float32(offset),
                          samples=np.ascontiguousarray(samples, np.complex64)))

    for i, g in enumerate(gold_cases()):
        add(f"gold{i + 1}", 6, g["n"], np.repeat(g["h"][:, :, None], R.n_cn(6), axis=2))
        cases[-1]["gold"] = g
    # seeded random channels: a random 2x2 matrix plus a per-sample perturbation of 0.3 of its scale
    for nof_prb, count in ((6, 60), (15, 24), (100, 6)):
        for k in range(count):
            snr = -5 + 40 * k / (count - 1)

            def draw(attempt, nof_prb=nof_prb, k=k):
                rng = np.random.default_rng(1000 * nof_prb + k + 100000 * attempt)
                return _cn(rng, (2, 2, 1)) + _cn(rng, (2, 2, R.n_cn(nof_prb)), 0.3)

            add(f"rand_prb{nof_prb}_{k}", nof_prb, 10 ** (-snr / 10), draw(0), offset=[0.0, -2.0, 3.5][k % 3])
            cases[-1]["draw"] = draw
    # rank 1, matched to codebook vector i: H = u w_i^H  (h[port][rx] = u[rx] conj(w_i[port]))
    for i in range(4):
        rng = np.random.default_rng(50 + i)
        u = _cn(rng, (2,))
        w = np.array([1, W2[i]], np.complex64) / np.sqrt(2)
        h = (np.conj(w)[:, None] * u[None, :])[:, :, None] + _cn(rng, (2, 2, R.n_cn(6)), 0.02)
        add(f"rank1_w{i}", 6, 0.01, h)
    rng = np.random.default_rng(60)
    uni = 1.5 * np.exp(0.7j) * np.array([[1, 1], [1, -1]], np.complex64) / np.sqrt(2)
    add("unitary", 6, 1e-3, uni[:, :, None] + _cn(rng, (2, 2, R.n_cn(6)), 0.01))
    add("all_zero", 6, 0.0, np.zeros((2, 2, R.n_cn(6)), np.complex64))
    rng = np.random.default_rng(61)
    h = _cn(rng, (2, 2, 1)) + _cn(rng, (2, 2, R.n_cn(6)), 0.3)
    h[1, 0, 3] = np.nan
    add("nan_sample", 6, 0.05, h)
    rng = np.random.default_rng(62)
    h = _cn(rng, (2, 2, 1)) + _cn(rng, (2, 2, R.n_cn(6)), 0.3)
    h[:, :, 40] = np.array([[900, -400j], [250j, 700]], np.complex64)
    h[:, :, 41] = np.array([[-800j, 300], [600, 500j]], np.complex64)
    add("outliers_m40_41", 6, 0.05, h)
    return cases


def main():
    tmp = tempfile.mkdtemp(prefix="csi_ref_")
    try:
        L = build_ref(tmp)
        cases = make_cases()
        for c in cases:
            c.update(run_ref(L, c))
            # the seeds of the random cases are chosen so that the reference's values keep clear of ties and
            # thresholds: a draw with an excluded decision is replaced by the next one
            attempt = 0
            while "draw" in c and R.excluded(c):
                attempt += 1
                assert attempt < 8, c["name"]
                c["samples"] = np.ascontiguousarray(c["draw"](attempt), np.complex64)
                c.update(run_ref(L, c))
            c["cn_count"] = R.cond_number(c["samples"])[1]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    worst = dict(sinr_1l=0.0, sinr_2l=0.0, cn=0.0)
    nexcl = 0
    for c in cases:
        if "gold" in c:  # the reference's own test bounds (pmi_select_test.c:84-150)
            g = c["gold"]
            for ref, got in ((g["s1"], c["sinr_1l"]), (g["s2"], c["sinr_2l"])):
                for a, b in zip(ref, got):
                    err = abs(a - b) / (a if a > 1000 else 1.0)
                    assert err <= 0.1, (c["name"], ref, got)
            assert [c["pmi_1l"], c["pmi_2l"]] == g["pmi"] and abs(c["cn"] - g["k"]) <= 0.1, c["name"]
        if c["name"].startswith("rank1_w"):
            assert c["pmi_1l"] == int(c["name"][-1]) and c["ri"] == 0, c
        if c["name"] == "unitary":
            assert c["ri"] == 1 and c["ri_cn"] == 1, c
        # the restatement against the reference
        s, tol = R.sums(c["samples"], c["nof_prb"], c["noise"]), R.tolerances(c)
        for k in ("sinr_1l", "sinr_2l", "cn"):
            assert R.same_class(s[k], c[k], tol[k]), (c["name"], k, s[k], c[k], tol[k])
            with np.errstate(all="ignore"):
                rel = np.abs(np.asarray(s[k], np.float64) - np.asarray(c[k], np.float64)) / np.asarray(tol[k], np.float64)
            if np.all(np.isfinite(rel)):
                worst[k] = max(worst[k], float(np.max(rel)))
        ex = R.excluded(c)
        nexcl += bool(ex)
        d = R.decide(c["sinr_1l"], c["sinr_2l"], c["cn"], c["offset"])
        for k in ("pmi_1l", "pmi_2l", "ri", "pmi", "ri_cn", "cqi"):
            assert d[k] == c[k], (c["name"], k, d[k], c[k])
        print(f"{c['name']:18s} prb {c['nof_prb']:3d} s1 {c['sinr_1l']} s2 {c['sinr_2l']} cn {c['cn']:.3f} "
              f"ri {c['ri']} pmi {c['pmi']} db {c['sinr_db']:.2f} cqi {c['cqi']} excluded {sorted(ex)}")
    print("restatement vs reference, largest |delta| / tolerance:", worst)
    print(f"cases with an excluded decision: {nexcl} of {len(cases)}")
    assert nexcl <= 0.05 * len(cases), (nexcl, len(cases))
    arrs = dict(names=np.array([c["name"] for c in cases]))
    for k, dt in (("nof_prb", np.uint32), ("noise", np.float32), ("offset", np.float32), ("cn", np.float32),
                  ("cn_count", np.uint32), ("sinr_db", np.float32), ("pmi_1l", np.uint32), ("pmi_2l", np.uint32),
                  ("ri", np.uint32), ("pmi", np.uint32), ("ri_cn", np.uint32), ("cqi", np.uint32)):
        arrs[k] = np.array([c[k] for c in cases], dt)
    arrs["sinr_1l"] = np.stack([c["sinr_1l"] for c in cases]).astype(np.float32)
    arrs["sinr_2l"] = np.stack([c["sinr_2l"] for c in cases]).astype(np.float32)
    for i, c in enumerate(cases):
        arrs[f"h_{i}"] = c["samples"]
    out = os.path.join(HERE, "csi_feedback.npz")
    np.savez_compressed(out, **arrs)
    print(out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < (1 << 20)


if __name__ == "__main__":
    main()
