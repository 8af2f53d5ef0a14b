#!/usr/bin/env python
"""Time one PHICH batch on the GPU: `python tools/phich_batch_time.py [--sf 2048] [--per-sf 1] [--prb 100] [--ports 2]`.

The subframes are grids and channel estimates already in HBM (16 distinct synthetic subframes with every PHICH of the
cell loaded, tiled), decoded by one mi355_ue_dl_decode_phich_batch call with --per-sf jobs per subframe; the call is
synchronous (descriptor upload, one kernel, one read-back), so the host clock around it is the call's time.  Prints one
JSON line (ms per call: median, min, max)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=int, default=2048, help="subframes in the batch")
    ap.add_argument("--per-sf", type=int, default=1, help="PHICH jobs per subframe")
    ap.add_argument("--prb", type=int, default=100)
    ap.add_argument("--ports", type=int, default=2)
    ap.add_argument("--rx", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    from srsran_amd import pdsch as P
    from srsran_amd import phich as H
    from srsran_amd.tdec import DeviceBuffer
    from srsran_amd.ue_dl import ChestRes, DlSfJob, UeDl

    cell_id, distinct = 3, 16
    cell = P.make_cell(args.prb, args.ports, cell_id, phich_resources=3)  # Ng = 2: 25 groups at 100 PRB
    ngroups = H.ngroups(cell)
    G = 14 * 12 * args.prb
    rng = np.random.default_rng(0)
    gains = (rng.standard_normal((args.ports, args.rx)) + 1j * rng.standard_normal((args.ports, args.rx))) / np.sqrt(2)
    host = np.zeros((distinct, args.rx * (1 + args.ports), G), np.complex64)
    acks = rng.integers(0, 2, (distinct, ngroups, H.NSEQUENCES))
    for k in range(distinct):
        tx = np.zeros((args.ports, G), np.complex64)
        for g in range(ngroups):
            for s in range(H.NSEQUENCES):
                assert H.phich_encode_host(cell, k % 10, g, s, int(acks[k, g, s]), tx) == 0
        for r in range(args.rx):
            host[k, r] = (gains[:, r, None] * tx).sum(axis=0)
            host[k, r] += 0.05 * (rng.standard_normal(G) + 1j * rng.standard_normal(G))
            for p in range(args.ports):
                host[k, args.rx + p * args.rx + r] = gains[p, r]
    buf = DeviceBuffer(host.nbytes).upload(host)
    sfjobs, chest, sfs = (DlSfJob * args.sf)(), (ChestRes * args.sf)(), (P.DlSfCfg * args.sf)()
    for i in range(args.sf):
        k = i % distinct
        base = buf.ptr + k * host.shape[1] * G * 8
        sfjobs[i].tti = sfs[i].tti = k % 10
        for r in range(args.rx):
            sfjobs[i].sf_symbols[r] = base + r * G * 8
            for p in range(args.ports):
                sfjobs[i].ce[p][r] = base + (args.rx + p * args.rx + r) * G * 8
        chest[i].noise_estimate = 0.005
    # job j of subframe i: PRB / cyclic shift chosen to spread over the groups and sequences
    n = args.sf * args.per_sf
    jobs, sent = (H.PhichJob * n)(), np.zeros(n, np.uint32)
    for i in range(args.sf):
        for j in range(args.per_sf):
            lo, dm = (7 * i + 13 * j) % args.prb, (i + j) % 8
            jobs[i * args.per_sf + j] = H.PhichJob(i, H.PhichGrant(lo, dm, 0))
            g, s = H.calc(cell, lo, dm)
            sent[i * args.per_sf + j] = acks[i % distinct, g, s]
    ue = UeDl(cell, args.rx)
    res = (H.PhichRes * n)()
    L = H._declare()
    times = []
    for it in range(args.warmup + args.calls):
        t0 = time.perf_counter()
        rc = L.mi355_ue_dl_decode_phich_batch(ue.h, sfjobs, sfs, chest, args.sf, jobs, n, res, None)
        dt = time.perf_counter() - t0
        assert rc == 0
        if it >= args.warmup:
            times.append(dt * 1e3)
    ok = sum(1 for i in range(n) if res[i].ret == 0 and res[i].ack_value == sent[i])
    times.sort()
    print(json.dumps({"phich_batch": {"subframes": args.sf, "jobs_per_subframe": args.per_sf, "jobs": n,
                                      "nof_prb": args.prb, "tx_ports": args.ports, "rx": args.rx, "groups": ngroups,
                                      "acks_correct": ok, "calls": args.calls,
                                      "ms_per_call_median": round(times[len(times) // 2], 3),
                                      "ms_per_call_min": round(times[0], 3), "ms_per_call_max": round(times[-1], 3)}}))
    ue.close()


if __name__ == "__main__":
    main()
