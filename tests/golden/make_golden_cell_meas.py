#!/usr/bin/env python3
"""Record tests/golden/cell_meas.npz: the reference's srslte_refsignal_dl_sync_run for the cases the neighbour-cell
measurement tests run.

    python tests/golden/make_golden_cell_meas.py

Needs the reference tree: tests/golden/cell_meas_ref_wrap.c is compiled together with the reference's
refsignal_dl_sync.c, refsignal_dl.c, ofdm.c, convolution.c, the PSS / SSS generators and what they call, read where they
lie, with the flags oracle/Makefile gives the reference (REF_OPT, ARCH, REF_DEFS: the AVX2 build) and an empty
srslte/srslte.h stand-in for the generated header, into a temporary directory that is removed afterwards.

The reference's FFT is a stand-in: FFTW is not available where this runs, so cell_meas_ref_wrap.c supplies srslte_dft_*
as a plain double-precision DFT.  The recorded values carry that transform's rounding (one rounding to float per
output), not an fp32 FFT's; everything outside the transform -- the vector kernels, the dot products, the averages, the
decisions -- is the reference's AVX2 code.

The fixture holds the cases (a JSON list: bandwidth, the arguments of tests/cell_meas_ref.py's synth_capture, which
regenerates the samples bit for bit, and the cells measured on it), per call the result fields iv / fv and the
per-subframe records, and checksums of the reference's sequences for a few cells.  It holds no samples.

The script prints, per float field, the largest deviation of the compiled reference from the float64 restatement
(tests/cell_meas_ref.py) relative to the field's scale (dB fields and CFO absolute, linear powers relative), and four
times that: the tolerance the tests apply, copied into cell_meas_ref.TOL.  A draw with a decision margin inside one
tolerance (cell_meas_ref.safe) is replaced by the next seed (+1000); every case is synthetic, so none is kept: the
script asserts that 0 % of the calls are excluded, and that the reference's decisions are the restatement's on every
call.  It also prints the reference's own time per call with the O(n^2) stand-in transform, for orientation only."""
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
import cell_meas_ref as R  # noqa: E402

REF = "/root/reference/lib"
REF_SRC = ["src/phy/ch_estimation/refsignal_dl.c", "src/phy/dft/ofdm.c", "src/phy/utils/convolution.c",
           "src/phy/sync/pss.c", "src/phy/sync/sss.c", "src/phy/sync/gen_sss.c", "src/phy/sync/find_sss.c",
           "src/phy/common/sequence.c", "src/phy/common/phy_common.c", "src/phy/utils/cexptab.c",
           "src/phy/utils/vector.c", "src/phy/utils/vector_simd.c", "src/phy/utils/bit.c", "src/phy/utils/debug.c",
           "src/phy/utils/phy_logger.c"]
L6 = 1920
MAX_SF = 12


def _make_var(name: str) -> list[str]:
    text = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    m = re.search(r"^" + name + r"\s*\??=\s*(.*)$", text, flags=re.M)
    assert m, name
    return m.group(1).split()


def build_ref(tmp: str) -> C.CDLL:
    so, vs = os.path.join(tmp, "libcell_meas_ref.so"), os.path.join(tmp, "exports.map")
    with open(vs, "w") as f:
        f.write("{ global: cmwrap_*; local: *; };\n")
    os.makedirs(os.path.join(tmp, "inc", "srslte"))
    open(os.path.join(tmp, "inc", "srslte", "srslte.h"), "w").close()
    cmd = (["gcc"] + _make_var("REF_OPT") + ["-fPIC", "-w"] + _make_var("ARCH") + _make_var("REF_DEFS") +
           ["-include", "stdint.h", "-include", "stdbool.h", "-include", "srslte/phy/utils/debug.h", f"-I{tmp}/inc",
            f"-I{REF}/include", f"-I{REF}", "-ffunction-sections", "-shared", "-Wl,--gc-sections",
            f"-Wl,--version-script={vs}", "-o", so, os.path.join(HERE, "cell_meas_ref_wrap.c")] +
           [os.path.join(REF, s) for s in REF_SRC] + ["-lm"])
    subprocess.run(cmd, check=True)
    und = subprocess.run(["nm", "-D", "--undefined-only", so], check=True, capture_output=True, text=True).stdout
    bad = [l for l in und.splitlines() if "srslte_" in l or "fftw" in l or l.split()[-1] == "ERROR"]
    assert not bad, bad
    L = C.CDLL(so)
    vp, u32 = C.c_void_p, C.c_uint32
    L.cmwrap_create.restype = vp
    L.cmwrap_set_cell.argtypes = [vp, u32, u32, u32]
    L.cmwrap_sf_len.restype = u32
    L.cmwrap_sf_len.argtypes = [vp]
    L.cmwrap_sequence.restype = None
    L.cmwrap_sequence.argtypes = [vp, u32, vp]
    L.cmwrap_free.restype = None
    L.cmwrap_free.argtypes = [vp]
    L.cmwrap_run.restype = None
    L.cmwrap_run.argtypes = [vp, vp, u32, u32, vp, vp, vp]
    return L


def cases() -> list[dict]:
    """each case: the arguments of synth_capture and the (cell id, ports) pairs measured on the capture"""
    out = []

    def add(nof_prb, nsf, cells, meas=None, cfo_hz=0.0, snr_db=20.0, tag=""):
        out.append(dict(tag=tag, cap=dict(nof_prb=nof_prb, nsf=nsf, cells=[list(c) for c in cells], cfo_hz=cfo_hz,
                                          snr_db=snr_db, seed=len(out) + 1),
                        meas=[list(m) for m in (meas or [c[:2] for c in cells])]))
    # capture lengths: 2 is the single-block case, 12 hits the 10-block cap; an absent PCI each
    for m, cid in zip((2, 3, 6, 11, 12), (1, 8, 21, 100, 333)):
        add(6, m, [(cid, 1 + (m % 2), 300 + 7 * m, 1.0)], [(cid, 1 + (m % 2)), (cid + 40, 1)], cfo_hz=150.0 * (m - 6),
            tag=f"len{m}")
    # peak positions: lag 0 of block 0, lag 1, lag sf_len - 1, both sides of the tile boundary, in blocks 0 and 1
    for d in (0, 1, L6 - 1, 1023, 1024, L6 + 1023, L6 + 1024):
        add(6, 6, [(13 + d % 5, 2, d, 1.0)], tag=f"lag{d}")
    # captures starting in every subframe: subframe 0 of the cell (10 - s) subframes into the capture
    ids = (0, 1, 2, 3, 4, 5, 150, 301, 412, 503)
    for s in range(10):
        add(6, 6, [(ids[s], (1, 2, 4)[s % 3], ((10 - s) % 10) * L6 + 137 + s, 1.0)], cfo_hz=-400.0 + 90 * s,
            snr_db=15.0, tag=f"start{s}")
    # the shift by 5 sf_len landing in the last block of an 11-subframe capture
    add(6, 11, [(77, 2, 9 * L6 + 500, 1.0)], tag="shift_last")
    # several cells per capture, strong and weak, low SNR: stage-3 rejections and mild faults live here
    for k, snr in enumerate((5.0, 5.0, 8.0, 5.0, 6.0, 5.0)):
        add(6, 6 + k, [(30 + 3 * k, 1, 211 + 300 * k, 1.0), (31 + 3 * k + 6, 2, 4000 + 1000 * k, 0.6),
                       (32 + 3 * k + 12, 1, 9000 + 500 * k, 0.3 + 0.02 * k)],
            [(30 + 3 * k, 1), (31 + 3 * k + 6, 2), (32 + 3 * k + 12, 1), (400 + k, 1)], cfo_hz=200.0 * k, snr_db=snr,
            tag=f"multi{k}")
    # other bandwidths (25 PRB: symbol size 384, the CP lengths are rounded up)
    add(15, 3, [(44, 2, 777, 1.0), (45, 1, 5000, 0.7)], tag="prb15")
    add(25, 3, [(99, 4, 1234, 1.0), (202, 1, 7000, 0.7)], tag="prb25")
    return out


SEQ_CELLS = [(0, 1, 6), (1, 2, 6), (2, 4, 6), (3, 1, 6), (4, 2, 6), (5, 4, 6), (503, 2, 6), (150, 1, 15), (301, 2, 15),
             (412, 4, 15), (99, 4, 25), (202, 1, 25), (7, 2, 25)]


def checksums(seq: np.ndarray) -> np.ndarray:
    """per subframe: sum, index-weighted sum (re, im each), sum |.|^2, of a (10, sf_len) array; float64"""
    s = np.asarray(seq, np.complex128)
    w = np.cos(0.37 * np.arange(s.shape[1])) + 1j * np.sin(0.11 * np.arange(s.shape[1]))
    a, b = s.sum(axis=1), (s * w).sum(axis=1)
    return np.stack([a.real, a.imag, b.real, b.imag, (np.abs(s) ** 2).sum(axis=1)], axis=1)


def run_case(L, objs, case: dict, bump: int):
    cap = dict(case["cap"], seed=case["cap"]["seed"] + bump)
    x = R.synth_capture(**{**cap, "cells": [tuple(c) for c in cap["cells"]]})
    recs = []
    for cid, ports in case["meas"]:
        key = (cid, ports, cap["nof_prb"])
        h = objs["h"]
        assert L.cmwrap_set_cell(h, cid, cap["nof_prb"], ports) == 0
        iv, fv = np.zeros(8, np.uint32), np.zeros(6, np.float32)
        sf = np.zeros((MAX_SF, 7), np.float32)
        xx = x.copy()
        t0 = time.perf_counter()
        L.cmwrap_run(h, xx.ctypes.data, x.size, MAX_SF, iv.ctypes.data, fv.ctypes.data, sf.ctypes.data)
        dt = time.perf_counter() - t0
        want = R.run(R.set_cell(*key), x, x.size, cap["nof_prb"])
        recs.append(dict(iv=iv, fv=fv, sf=sf, want=want, dt=dt, meta=dict(tag=case["tag"], cap=cap, cell=[cid, ports])))
    return recs


def main():
    tmp = tempfile.mkdtemp(prefix="cell_meas_ref_")
    try:
        L = build_ref(tmp)
        objs = dict(h=L.cmwrap_create())
        assert objs["h"]
        iv_all, fv_all, sf_all, meta, times = [], [], [], [], []
        dev = {f: 0.0 for f in R.RES_FLOAT + R.SF_FLOAT + ("sequence",)}
        total = replaced = unsafe = 0
        for ci, case in enumerate(cases()):
            for attempt in range(8):
                recs = run_case(L, objs, case, 1000 * attempt)
                if all(R.safe(r["want"]) for r in recs):
                    break
                replaced += 1  # a decision margin inside one tolerance: the next seed
            for r in recs:
                iv, fv, sf, w = r["iv"], r["fv"], r["sf"], r["want"]
                total += 1
                unsafe += not R.safe(w)
                got = dict(zip(R.RES_INT, iv.tolist()))
                for f in R.RES_INT:
                    assert got[f] == w[f], (ci, r["meta"], f, got, {g: w[g] for g in R.RES_INT}, w["margin"])
                for i, f in enumerate(R.RES_FLOAT):
                    if np.isnan(w[f]):
                        assert np.isnan(fv[i]), (ci, f)
                        continue
                    d = abs(float(fv[i]) - w[f]) / (1.0 if f in R.ABSOLUTE else abs(w[f]))
                    dev[f] = max(dev[f], d)
                assert got["sf_count"] == len(w["sf"])
                for k, ws in enumerate(w["sf"]):
                    assert int(sf[k, 0]) == ws["sf_idx"]
                    for i, f in enumerate(R.SF_FLOAT):
                        scale = 1.0 if f in R.ABSOLUTE else max(abs(ws[f]), abs(ws["rsrp"]) if f != "rssi" else 0.0)
                        dev[f] = max(dev[f], abs(float(sf[k, 1 + i]) - ws[f]) / scale)
                if r["meta"]["cap"]["nof_prb"] == 6 and r["meta"]["cap"]["nsf"] == 6:
                    times.append(r["dt"])
                iv_all.append(iv), fv_all.append(fv), sf_all.append(sf)
                meta.append(dict(case=ci, **r["meta"]))
        # the sequences
        seq_sums = []
        for cid, ports, prb in SEQ_CELLS:
            assert L.cmwrap_set_cell(objs["h"], cid, prb, ports) == 0
            n = L.cmwrap_sf_len(objs["h"])
            got = np.zeros((10, n), np.complex64)
            for sf in range(10):
                L.cmwrap_sequence(objs["h"], sf, got[sf].ctypes.data)
            want = R.set_cell(cid, ports, prb)
            assert want.shape == got.shape
            dev["sequence"] = max(dev["sequence"], float(np.max(np.abs(got - want)) / np.max(np.abs(want))))
            seq_sums.append(checksums(got))
        L.cmwrap_free(objs["h"])
        print(f"calls {total}, draws replaced by the next seed {replaced}, excluded {unsafe} "
              f"({100.0 * unsafe / total:.1f} %)")
        assert unsafe == 0
        n_s3 = sum(1 for iv in iv_all if iv[3] and iv[7])
        n_mild = sum(1 for iv in iv_all if iv[0] and iv[6] == 1)
        print(f"stage-1 found and stage-3 rejected: {n_s3} calls; found with exactly one mild fault: {n_mild} calls; "
              f"not found in stage 1: {sum(1 for iv in iv_all if not iv[3])}; "
              f"half-frame shift: {sum(1 for iv in iv_all if iv[4])}")
        assert n_s3 >= 1 and n_mild >= 1
        for f in dev:
            print(f"{f:20s} max deviation {dev[f]:.3e}   tolerance (4 x) {4 * dev[f]:.3e}")
        times.sort()
        ref_ms = 1e3 * times[len(times) // 2]
        print(f"reference srslte_refsignal_dl_sync_run, 6 PRB, 6 subframes, one cell, one host core, WITH THE DFT "
              f"STAND-IN (an O(n^2) transform of 3,840 points, not FFTW): median {ref_ms:.1f} ms per call over "
              f"{len(times)} calls")
        out = os.path.join(HERE, "cell_meas.npz")
        np.savez_compressed(out, meta=json.dumps(meta), iv=np.array(iv_all), fv=np.array(fv_all),
                            sf=np.array(sf_all), iv_fields=np.array(R.RES_INT), fv_fields=np.array(R.RES_FLOAT),
                            sf_fields=np.array(("sf_idx",) + R.SF_FLOAT), seq_cells=np.array(SEQ_CELLS),
                            seq_sums=np.array(seq_sums), ref_ms_per_call_standin=np.float64(ref_ms))
        print(out, os.path.getsize(out), "bytes")
    finally:
        import shutil
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
