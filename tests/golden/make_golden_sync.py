#!/usr/bin/env python3
"""Record tests/golden/sync_find.npz: the reference's srslte_sync_find for the cases the cell-search tests run.

    python tests/golden/make_golden_sync.py

Needs the reference tree: tests/golden/sync_ref_wrap.c is compiled together with the reference's sync.c, pss.c, sss.c,
gen_sss.c, find_sss.c, cp.c, cfo.c, convolution.c and what they call, read where they lie, with the flags
oracle/Makefile gives the reference (REF_OPT, ARCH, REF_DEFS: the AVX2 build) and an empty srslte/srslte.h stand-in
for the generated header, into a temporary directory that is removed afterwards.

The reference's FFT is a stand-in: FFTW is not available where this runs, so sync_ref_wrap.c supplies srslte_dft_* as
a plain double-precision DFT that honours the plans' mirror / dc / norm flags.  The recorded values carry that
transform's rounding (one rounding to float per output), not an fp32 FFT's; everything outside the transform -- the
vector kernels, the averages, the SSS correlations, the decisions -- is the reference's AVX2 code.

The fixture holds, per call, the case's parameters (a JSON list: object settings, where the input comes from -- a slice
of tests/golden/signal_1.92M_amar.c64 or the arguments of tests/sync_ref.py's synth_frame, which regenerates the
samples bit for bit -- and find_offset), and every result field: iv (ret, peak_pos, sss_available, sss_detected, m0,
m1, n_id_1, sf_idx, cell_id, cp, frame_type) and fv (peak_value, peak_abs, cfo_pss, cfo_pss_mean, m0_value, m1_value,
sss_corr, M_norm_avg, M_ext_avg).

It also holds the reference's PSS for the three N_id_2 and its SSS (subframes 0 and 5) for ten cell ids.

The script prints, per float field, the largest deviation of the compiled reference from the float64 restatement
(tests/sync_ref.py) relative to the field's scale, and four times that: the tolerance the tests apply.  A synthetic
draw with a decision inside the tolerance band (sync_ref.safe) is replaced by the next seed (+1000); what cannot be
replaced (the recording) is kept and counted, and at most 5 % of the calls may be of that kind.  On every other call
the reference's decisions must be the restatement's: the script asserts it.  It also prints the reference's own time
per srslte_sync_find call on one host core -- with the O(n^2) stand-in transform, so an orientation for nothing but
this build of it."""
from __future__ import annotations

import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import sync_ref as R  # noqa: E402

REF = "/root/reference/lib"
REF_SRC = ["src/phy/sync/sync.c", "src/phy/sync/pss.c", "src/phy/sync/sss.c", "src/phy/sync/gen_sss.c",
           "src/phy/sync/find_sss.c", "src/phy/sync/cp.c", "src/phy/sync/cfo.c", "src/phy/utils/convolution.c",
           "src/phy/utils/cexptab.c", "src/phy/utils/filter.c", "src/phy/utils/vector.c", "src/phy/utils/vector_simd.c",
           "src/phy/utils/bit.c", "src/phy/utils/debug.c", "src/phy/utils/phy_logger.c", "src/phy/common/phy_common.c"]
IV = ("ret", "peak_pos", "sss_available", "sss_detected", "m0", "m1", "n_id_1", "sf_idx", "cell_id", "cp", "frame_type")
FV = ("peak_value", "peak_abs", "cfo_pss", "cfo_pss_mean", "m0_value", "m1_value", "sss_corr", "M_norm_avg", "M_ext_avg")
# the scale a field's deviation is taken relative to, where the value itself may be near zero
SCALE = {"cfo_pss": 1.0, "cfo_pss_mean": 1.0, "M_norm_avg": 1.0, "M_ext_avg": 1.0, "m0_value": 961.0,
         "m1_value": 961.0, "sss_corr": 961.0}
RECORDING = os.path.join(HERE, "signal_1.92M_amar.c64")


def _make_var(name: str) -> list[str]:
    text = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    m = re.search(r"^" + name + r"\s*\??=\s*(.*)$", text, flags=re.M)
    assert m, name
    return m.group(1).split()


def build_ref(tmp: str) -> C.CDLL:
    so, vs = os.path.join(tmp, "libsync_ref.so"), os.path.join(tmp, "exports.map")
    with open(vs, "w") as f:
        f.write("{ global: syncwrap_*; local: *; };\n")
    os.makedirs(os.path.join(tmp, "inc", "srslte"))
    open(os.path.join(tmp, "inc", "srslte", "srslte.h"), "w").close()
    cmd = (["gcc"] + _make_var("REF_OPT") + ["-fPIC", "-w"] + _make_var("ARCH") + _make_var("REF_DEFS") +
           ["-include", "stdint.h", "-include", "stdbool.h", "-include", "srslte/phy/utils/debug.h", f"-I{tmp}/inc",
            f"-I{REF}/include", "-ffunction-sections", "-shared", "-Wl,--gc-sections",
            f"-Wl,--version-script={vs}", "-o", so, os.path.join(HERE, "sync_ref_wrap.c")] +
           [os.path.join(REF, s) for s in REF_SRC] + ["-lm"])
    subprocess.run(cmd, check=True)
    und = subprocess.run(["nm", "-D", "--undefined-only", so], check=True, capture_output=True, text=True).stdout
    bad = [l for l in und.splitlines() if "srslte_" in l or "fftw" in l or l.split()[-1] == "ERROR"]
    assert not bad, bad
    L = C.CDLL(so)
    L.syncwrap_create.restype = C.c_void_p
    L.syncwrap_create.argtypes = [C.c_uint32] * 3 + [C.c_float] * 3 + [C.c_int] * 8 + [C.c_float]
    L.syncwrap_reset.argtypes = [C.c_void_p]
    L.syncwrap_free.argtypes = [C.c_void_p]
    L.syncwrap_find.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.syncwrap_pss_generate.argtypes = [C.c_uint32, C.c_void_p]
    L.syncwrap_sss_generate.restype = None
    L.syncwrap_sss_generate.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p]
    return L


def frame_of(src: dict) -> np.ndarray:
    if src["kind"] == "recording":
        iq = np.fromfile(RECORDING, np.complex64)
        return iq[src["start"]:src["start"] + src["len"]].copy()
    return R.synth_frame(**src["args"])


def cases() -> list[dict]:
    """each case: cfg (SyncRef keywords with n_id_2), a list of (source, find_offset) calls on one object"""
    out = []
    rec = [dict(kind="recording", start=9600 * h, len=9600 + 128) for h in range(2)]
    for id2 in range(3):
        out.append(dict(cfg=dict(fft_size=128, max_offset=9600, n_id_2=id2, threshold=2.0, cfo_pss_enable=True),
                        calls=[(rec[0], 0), (rec[1], 0)]))
    cells = [(0, 0), (4, 5), (89, 0), (90, 5), (502, 0), (503, 5)]
    k = 0
    for cp in (R.CP_NORM, R.CP_EXT):
        for alg in (R.FULL, R.PARTIAL_3, R.DIFF):
            for cid, sf in cells:
                for snr in (20.0, 3.0):
                    k += 1
                    src = dict(kind="synth", args=dict(cell_id=cid, sf_idx=sf, cp=cp, lead=300 + 13 * k, snr_db=snr,
                                                       seed=k))
                    out.append(dict(cfg=dict(fft_size=128, max_offset=9600, n_id_2=cid % 3, threshold=2.0, sss_alg=alg,
                                             cp=cp), calls=[(src, 0), (src, 0)]))
    for cp in (R.CP_NORM, R.CP_EXT):
        for ft in (R.FDD, R.TDD):
            for filt in (False, True):
                for j, (cid, sf) in enumerate(cells[:4]):
                    k += 1
                    src = dict(kind="synth", args=dict(cell_id=cid, sf_idx=sf, cp=cp, frame_type=ft, lead=500 + 7 * k,
                                                       cfo=0.3 if j % 2 else -0.3, snr_db=15.0, seed=k))
                    out.append(dict(cfg=dict(fft_size=128, max_offset=9600, n_id_2=cid % 3, threshold=2.0,
                                             cfo_pss_enable=True, pss_filt_enable=filt, detect_cp=False, cp=cp,
                                             cfo_ema_alpha=0.1), calls=[(src, 0), (src, 77)]))
    for off in (832, 832 - 17, 832 - 30):  # max_offset < fft_size
        k += 1
        src = dict(kind="synth", args=dict(cell_id=151, sf_idx=5, lead=0, seed=k))
        out.append(dict(cfg=dict(fft_size=128, max_offset=32, n_id_2=1, threshold=0.0, cfo_pss_enable=True),
                        calls=[(src, off)]))
    for off in (1664, 1520, 1409):  # fft 256
        k += 1
        src = dict(kind="synth", args=dict(cell_id=77, sf_idx=0, nof_prb=15, lead=0, seed=k, nsf=1))
        out.append(dict(cfg=dict(fft_size=256, max_offset=512, n_id_2=2, threshold=2.0, cfo_pss_enable=True,
                                 pss_filt_enable=True), calls=[(src, off)]))
    # a sequence with the correlation average on
    seq = [(dict(kind="synth", args=dict(cell_id=200, sf_idx=5 * (i % 2), cp=R.CP_EXT, lead=400, cfo=c,
                                         snr_db=12.0, seed=40 + i)), 0)
           for i, c in enumerate([0.1, 0.12, 0.08, 0.1, 0.5, 0.1, 0.11, 0.09])]
    for alpha in (0.2, 1.0):
        out.append(dict(cfg=dict(fft_size=128, max_offset=9600, n_id_2=2, threshold=1.25, ema_alpha=alpha,
                                 cfo_pss_enable=True), calls=seq))
    return out


SEQ_IDS = (0, 1, 2, 89, 90, 151, 200, 301, 502, 503)  # cell ids whose SSS the fixture records


def run_case(L, case: dict, bump: int):
    """the case's calls on one reference object and one restatement; synthetic sources use seed + bump"""
    c = dict(fft_size=128, max_offset=9600, n_id_2=0, threshold=2.0, ema_alpha=1.0, cfo_ema_alpha=0.1,
             cfo_pss_enable=False, pss_filt_enable=False, sss_en=True, sss_alg=R.FULL, detect_cp=True,
             cp=R.CP_NORM, detect_frame_type=True, frame_type=R.FDD, sss_corr_threshold=0.0)
    c.update(case["cfg"])
    h = L.syncwrap_create(c["fft_size"], c["max_offset"], c["n_id_2"], c["threshold"], c["ema_alpha"],
                          c["cfo_ema_alpha"], int(c["cfo_pss_enable"]), int(c["pss_filt_enable"]), int(c["sss_en"]),
                          c["sss_alg"], int(c["detect_cp"]), c["cp"], int(c["detect_frame_type"]), c["frame_type"],
                          c["sss_corr_threshold"])
    assert h
    q = R.SyncRef(**c)
    recs = []
    for src, off in case["calls"]:
        if src["kind"] == "synth" and bump:
            src = dict(kind="synth", args=dict(src["args"], seed=src["args"]["seed"] + bump))
        x = np.concatenate([frame_of(src), np.zeros(1024, np.complex64)])
        iv, fv = np.zeros(len(IV), np.int32), np.zeros(len(FV), np.float32)
        t0 = time.perf_counter()
        L.syncwrap_find(h, x.ctypes.data, off, iv.ctypes.data, fv.ctypes.data)
        dt = time.perf_counter() - t0
        recs.append(dict(iv=iv, fv=fv, want=q.find(x, off), dt=dt,
                         meta=dict(cfg=c, src=src, find_offset=off)))
    L.syncwrap_free(h)
    return recs


def main():
    tmp = tempfile.mkdtemp(prefix="sync_ref_")
    try:
        L = build_ref(tmp)
        iv_all, fv_all, meta, times = [], [], [], []
        dev = {f: 0.0 for f in FV}
        unsafe = total = replaced = 0
        for ci, case in enumerate(cases()):
            synth = all(src["kind"] == "synth" for src, _ in case["calls"])
            for attempt in range(8):
                recs = run_case(L, case, 1000 * attempt)
                if all(R.safe(r["want"]) for r in recs) or not synth:
                    break
                replaced += 1  # a draw with a decision inside the tolerance band: the next seed
            for r in recs:
                iv, fv, w = r["iv"], r["fv"], r["want"]
                total += 1
                ok = R.safe(w)
                unsafe += not ok
                if ok:
                    got = dict(zip(IV, iv.tolist()))
                    for f in IV:  # (m0 / m1 / N_id_1 are the reference's only where the SSS was detected)
                        if f in ("n_id_1", "m0", "m1", "cell_id") and not w["sss_detected"]:
                            continue
                        assert got[f] == w[f], (ci, f, got, {g: w[g] for g in IV})
                    for i, f in enumerate(FV):
                        if f in ("m0_value", "m1_value", "sss_corr") and not w["sss_available"]:
                            continue
                        d = abs(float(fv[i]) - w[f]) / max(abs(w[f]), SCALE.get(f, 1e-30))
                        dev[f] = max(dev[f], d)
                if r["meta"]["cfg"]["fft_size"] == 128 and r["meta"]["cfg"]["max_offset"] == 9600:
                    times.append(r["dt"])
                iv_all.append(iv), fv_all.append(fv)
                meta.append(dict(case=ci, safe=bool(ok), **r["meta"]))
        print(f"calls {total}, draws replaced by the next seed {replaced}, kept with a decision inside the tolerance "
              f"band {unsafe} ({100.0 * unsafe / total:.1f} %)")
        assert unsafe <= 0.05 * total
        for f in FV:
            print(f"{f:14s} max deviation {dev[f]:.3e}   tolerance (4 x) {4 * dev[f]:.3e}")
        times.sort()
        ref_ms = 1e3 * times[len(times) // 2]
        print(f"reference srslte_sync_find, fft 128, 9,600 samples, one N_id_2, one host core, WITH THE DFT STAND-IN "
              f"(an O(n^2) transform of 9,728 points, not FFTW): median {ref_ms:.1f} ms per call over {len(times)} calls")
        pss = np.zeros((3, 62), np.complex64)
        for i in range(3):
            assert L.syncwrap_pss_generate(i, pss[i].ctypes.data) == 0
        sss = np.zeros((len(SEQ_IDS), 2, 62), np.float32)
        for k, cid in enumerate(SEQ_IDS):
            L.syncwrap_sss_generate(cid, sss[k, 0].ctypes.data, sss[k, 1].ctypes.data)
        out = os.path.join(HERE, "sync_find.npz")
        np.savez_compressed(out, meta=json.dumps(meta), iv=np.array(iv_all), fv=np.array(fv_all),
                            iv_fields=np.array(IV), fv_fields=np.array(FV), pss=pss, sss_ids=np.array(SEQ_IDS), sss=sss,
                            ref_ms_per_call_standin=np.float64(ref_ms))
        print(out, os.path.getsize(out), "bytes")
    finally:
        import shutil
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
