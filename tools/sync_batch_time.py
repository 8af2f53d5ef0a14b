#!/usr/bin/env python
"""Time one cell-search batch on the GPU: `python tools/sync_batch_time.py [--jobs 2048] [--fft 128] [--mode 0]`.

The jobs are 5 ms frames (75 fft_size samples, 9,600 at fft 128) already in HBM (16 distinct synthetic frames, tiled),
searched by one mi355_sync_find_batch call with all three N_id_2 hypotheses, the PSS-based CFO estimate, SSS_FULL, CP
and frame-type detection; the call is synchronous (five launches, one read-back), so the host clock around it is the
call's time.  Prints one JSON line (ms per call: median, min, max)."""
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
    ap.add_argument("--fft", type=int, default=128, choices=[128, 256])
    ap.add_argument("--mode", type=int, default=0, help="0 INDEPENDENT, 1 SEQUENCE")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import sync_ref as R
    from srsran_amd import sync as S
    from srsran_amd.tdec import DeviceBuffer

    distinct, nprb = 16, {128: 6, 256: 15}[args.fft]
    flen = 75 * args.fft
    cells = [(3 * (11 * i % 168) + i % 3, 5 * (i % 2)) for i in range(distinct)]
    frames = [R.synth_frame(cid, sf, nof_prb=nprb, lead=100 + 97 * i, seed=i, tail=2 * args.fft)[:flen + args.fft]
              for i, (cid, sf) in enumerate(cells)]
    host = np.stack(frames)
    buf = DeviceBuffer(host.nbytes).upload(host)
    jobs = (S.SyncJob * args.jobs)(*[S.SyncJob(buf.ptr + (i % distinct) * host.shape[1] * 8, 0)
                                     for i in range(args.jobs)])
    q = S.Sync(S.sync_cfg(fft_size=args.fft, max_offset=flen, cfo_pss_enable=True))
    res = (S.SyncRes * (3 * args.jobs))()
    times = []
    for it in range(args.warmup + args.calls):
        if args.mode:
            q.reset()
        t0 = time.perf_counter()
        rc = q.L.mi355_sync_find_batch(q.h, jobs, args.jobs, args.mode, res, None)
        dt = time.perf_counter() - t0
        assert rc == 0
        if it >= args.warmup:
            times.append(dt * 1e3)
    ok = sum(1 for i in range(args.jobs) if res[3 * i + cells[i % distinct][0] % 3].cell_id == cells[i % distinct][0])
    times.sort()
    print(json.dumps({"sync_batch": {"jobs": args.jobs, "fft_size": args.fft, "samples": flen, "hypotheses": 3,
                                     "mode": "SEQUENCE" if args.mode else "INDEPENDENT", "acquired": ok,
                                     "calls": args.calls, "ms_per_call_median": round(times[len(times) // 2], 3),
                                     "ms_per_call_min": round(times[0], 3), "ms_per_call_max": round(times[-1], 3)}}))
    q.close()


if __name__ == "__main__":
    main()
