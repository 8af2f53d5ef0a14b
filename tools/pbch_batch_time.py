#!/usr/bin/env python
"""Time one PBCH batch on the GPU: `python tools/pbch_batch_time.py [--jobs 2048] [--prb 100] [--ports 2] [--mode 0]`.

The jobs are subframe-0 grids and 4-port channel estimates already in HBM (16 distinct synthetic frames, tiled), decoded
by one mi355_pbch_decode_batch call with all port hypotheses searched; the call is synchronous (kernels, one read-back,
host replay), so the host clock around it is the call's time.  Prints one JSON line (ms per call: median, min, max)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=2048)
    ap.add_argument("--prb", type=int, default=100)
    ap.add_argument("--ports", type=int, default=2, help="transmit ports of the synthetic cell")
    ap.add_argument("--mode", type=int, default=0, help="0 INDEPENDENT, 1 SEQUENCE")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import pbch_ref as R
    from srsran_amd import pbch as B
    from srsran_amd import pdsch as P
    from srsran_amd.tdec import DeviceBuffer
    from srsran_amd.ue_dl import ChestRes, DlSfJob

    cell_id, distinct = 3, 16
    rng = np.random.default_rng(0)
    payload = B.mib_pack(P.make_cell(args.prb, args.ports, cell_id, phich_resources=2), 656)
    frames = [R.synth_frame(args.prb, cell_id, args.ports, 4, payload, i % 4, 0.3, rng) for i in range(distinct)]
    G = 14 * 12 * args.prb
    host = np.zeros((distinct, 5, G), np.complex64)
    for i, (g, ce, _nz) in enumerate(frames):
        host[i, 0], host[i, 1:] = g, ce
    buf = DeviceBuffer(host.nbytes).upload(host)
    jobs, chest = (DlSfJob * args.jobs)(), (ChestRes * args.jobs)()
    for i in range(args.jobs):
        k = i % distinct
        jobs[i].sf_symbols[0] = buf.ptr + k * 5 * G * 8
        for p in range(4):
            jobs[i].ce[p][0] = buf.ptr + (k * 5 + 1 + p) * G * 8
        chest[i].noise_estimate = frames[k][2]
    q = B.Pbch(P.make_cell(args.prb, 0, cell_id))
    res = (B.PbchRes * args.jobs)()
    times = []
    for it in range(args.warmup + args.calls):
        if args.mode:
            q.reset()
        t0 = time.perf_counter()
        rc = q.L.mi355_pbch_decode_batch(q.h, jobs, chest, args.jobs, args.mode, res, None)
        dt = time.perf_counter() - t0
        assert rc == 0
        if it >= args.warmup:
            times.append(dt * 1e3)
    ok = sum(1 for i in range(args.jobs) if res[i].ret == 1 and res[i].nof_tx_ports == args.ports)
    times.sort()
    print(json.dumps({"pbch_batch": {"jobs": args.jobs, "nof_prb": args.prb, "tx_ports": args.ports,
                                     "mode": "SEQUENCE" if args.mode else "INDEPENDENT", "search_all_ports": True,
                                     "decoded": ok, "calls": args.calls,
                                     "ms_per_call_median": round(times[len(times) // 2], 3),
                                     "ms_per_call_min": round(times[0], 3), "ms_per_call_max": round(times[-1], 3)}}))
    q.close()


if __name__ == "__main__":
    main()
