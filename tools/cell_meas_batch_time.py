#!/usr/bin/env python
"""Time neighbour-cell measurement batches on the GPU: `python tools/cell_meas_batch_time.py [--workload all]`.

Workloads (captures synthetic, already in HBM; one mi355_cell_meas_run_batch call each, synchronous -- two launches and
one read-back -- so the host clock around it is the call's time):
  many    256 captures x 8 PCIs at 6 PRB, 5 subframes (16 distinct captures, tiled)
  brute   one 6 PRB capture of 6 subframes x all 504 PCIs
  wide    one 100 PRB capture of 5 subframes x 8 PCIs
Prints one JSON line per workload: ms per call (median of --calls after --warmup, min, max), the complex MACs of the
correlation kernel (jobs x blocks x sf_len^2) and the rate they amount to over the whole call."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def workload(name):
    import cell_meas_ref as R
    if name == "many":
        prb, nsf, pcis = 6, 5, [3 * i + 1 for i in range(8)]
        caps = [R.synth_capture(prb, nsf, [(pcis[i % 8], 1, 100 + 517 * i, 1.0), (pcis[(i + 3) % 8], 2, 4000 + 300 * i, 0.7)],
                                snr_db=15.0, seed=i) for i in range(16)]
        jobs = [(c % 16, k) for c in range(256) for k in range(8)]
    elif name == "brute":
        prb, nsf, pcis = 6, 6, list(range(504))
        caps = [R.synth_capture(prb, nsf, [(10, 1, 500, 1.0), (83, 2, 3000, 1.0), (302, 1, 5000, 1.0)], cfo_hz=120.0, seed=1)]
        jobs = [(0, k) for k in range(504)]
    else:
        prb, nsf, pcis = 100, 5, [17, 250, 400, 401, 402, 403, 404, 405]
        caps = [R.synth_capture(prb, nsf, [(17, 2, 3001, 1.0), (250, 1, 30000, 0.8)], snr_db=15.0, seed=3)]
        jobs = [(0, k) for k in range(8)]
    return prb, nsf, pcis, caps, jobs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all", choices=["all", "many", "brute", "wide"])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    from srsran_amd import cell_meas as M
    from srsran_amd.tdec import DeviceBuffer

    for name in (["many", "brute", "wide"] if args.workload == "all" else [args.workload]):
        prb, nsf, pcis, caps, jobs = workload(name)
        host = np.stack(caps)
        buf = DeviceBuffer(host.nbytes).upload(host)
        q = M.CellMeas(prb, nsf)
        t0 = time.perf_counter()
        q.set_cells([(p, 1) for p in pcis])
        set_ms = (time.perf_counter() - t0) * 1e3
        n = len(jobs)
        arr = (M.CellMeasJob * n)(*[M.CellMeasJob(buf.ptr + c * host.shape[1] * 8, host.shape[1], k) for c, k in jobs])
        res = (M.CellMeasRes * n)()
        times = []
        for it in range(args.warmup + args.calls):
            t0 = time.perf_counter()
            rc = q.L.mi355_cell_meas_run_batch(q.h, arr, n, res, None, None)
            dt = time.perf_counter() - t0
            assert rc == 0
            if it >= args.warmup:
                times.append(dt * 1e3)
        times.sort()
        med = times[len(times) // 2]
        blocks = min(nsf - 1, 10)
        macs = n * blocks * q.sf_len ** 2
        print(json.dumps({"cell_meas_batch": {
            "workload": name, "nof_prb": prb, "subframes": nsf, "jobs": n, "cells": len(pcis),
            "found": sum(1 for i in range(n) if res[i].found), "set_cells_ms": round(set_ms, 3), "calls": args.calls,
            "ms_per_call_median": round(med, 3), "ms_per_call_min": round(times[0], 3),
            "ms_per_call_max": round(times[-1], 3), "corr_complex_macs": macs,
            "corr_tflops_fp64_over_call": round(8 * macs / (med * 1e-3) / 1e12, 3)}}))
        q.close()


if __name__ == "__main__":
    main()
