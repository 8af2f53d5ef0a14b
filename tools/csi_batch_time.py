#!/usr/bin/env python
"""Time one CSI feedback batch on the GPU: `python tools/csi_batch_time.py [--sf 2048] [--prb 100] [--ce-rows 0|1]`.

The subframes are 2x2 channel estimates already in HBM (--distinct synthetic channels, 16 by default -- a random matrix
plus a per-subcarrier perturbation, the same in every OFDM symbol -- tiled over the batch; 16 channels of 100 PRB are
8.6 MB and stay in the caches, --distinct 512 is 275 MB, more than the 256 MiB Infinity Cache), evaluated by one
mi355_ue_dl_csi_batch call; the call is synchronous (descriptor upload, one kernel, one read-back, the decisions on the
host), so the host clock around it is the call's time.  --ce-rows 1 times the row-0-only layout of
mi355_ue_dl_set_ce_rows(1) on the same channels (14x fewer estimate bytes behind the same number of loads); both
layouts give the same results.  Prints one JSON line (ms per call: median, min, max)."""
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
    ap.add_argument("--prb", type=int, default=100)
    ap.add_argument("--ce-rows", type=int, default=0, choices=(0, 1), help="1: estimates hold row 0 only")
    ap.add_argument("--distinct", type=int, default=16, help="distinct channels tiled over the batch")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    from srsran_amd import csi
    from srsran_amd import pdsch as P
    from srsran_amd.tdec import DeviceBuffer
    from srsran_amd.ue_dl import ChestRes, DlSfJob, UeDl

    distinct, nre = min(args.distinct, args.sf), 12 * args.prb
    rows = 1 if args.ce_rows else 14
    G = rows * nre
    rng = np.random.default_rng(0)
    def cn(shape):
        return rng.standard_normal(shape, np.float32) + 1j * rng.standard_normal(shape, np.float32)

    row = cn((distinct, 2, 2, 1)) + np.float32(0.3) * cn((distinct, 2, 2, nre))
    host = np.ascontiguousarray(np.tile(row.astype(np.complex64), (1, 1, 1, rows)))
    buf = DeviceBuffer(host.nbytes).upload(host)
    sfjobs, chest = (DlSfJob * args.sf)(), (ChestRes * args.sf)()
    for i in range(args.sf):
        k = i % distinct
        for p in range(2):
            for r in range(2):
                sfjobs[i].ce[p][r] = buf.ptr + ((k * 2 + p) * 2 + r) * G * 8
        chest[i].noise_estimate = 10 ** (-(5 + 2 * (k % 16)) / 10)
    ue = UeDl(P.make_cell(args.prb, 2, 3), 2)
    ue.set_ce_rows(args.ce_rows)
    res = (csi.CsiRes * args.sf)()
    L = csi._declare()
    times = []
    for it in range(args.warmup + args.calls):
        t0 = time.perf_counter()
        rc = L.mi355_ue_dl_csi_batch(ue.h, sfjobs, chest, args.sf, 0.0, res, None)
        dt = time.perf_counter() - t0
        assert rc == 0
        if it >= args.warmup:
            times.append(dt * 1e3)
    # the tiled subframes repeat every `distinct`: so must the results
    same = sum(1 for i in range(distinct, args.sf) if bytes(res[i]) == bytes(res[i % distinct]))
    times.sort()
    print(json.dumps({"csi_batch": {"subframes": args.sf, "nof_prb": args.prb, "ce_rows": args.ce_rows,
                                    "distinct": distinct, "samples_per_subframe": 7 * args.prb, "estimate_bytes": int(host.nbytes),
                                    "repeats_consistent": same == max(args.sf - distinct, 0),
                                    "ri": [int(res[k].ri) for k in range(min(distinct, 16))],
                                    "cqi": [int(res[k].cqi) for k in range(min(distinct, 16))],
                                    "calls": args.calls, "ms_per_call_median": round(times[len(times) // 2], 3),
                                    "ms_per_call_min": round(times[0], 3), "ms_per_call_max": round(times[-1], 3)}}))
    ue.close()


if __name__ == "__main__":
    main()
