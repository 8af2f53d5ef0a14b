"""The workspaces that are freed and reallocated when a call outgrows them (DevScratch::SyncFree,
srsran_amd/csrc/device_mem.h): a small call, one that outgrows the workspace, then the small one again, all on one
object; every call's outputs equal, byte for byte, those of the same call on a freshly created object.  The tables
cached by the first call (interleavers, RE maps, scrambling sequences, search plans) are reused by the later ones."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import pdsch_chain as pc
from srsran_amd import enb_dl
from srsran_amd import pdcch as D
from srsran_amd import pdsch as P
from srsran_amd.tdec import DeviceBuffer, Tdec8Batch, TdecBatch, tdec_buf_len
from srsran_amd.ue_dl import ChestRes, DlSfJob, UeDl
from tests.pdsch_jobs import cell_of
from tests.test_enb_dl_gpu import dev_zeros, enb_job

pytestmark = pytest.mark.gpu

SIZES = (2, 70, 2)  # code blocks: small, outgrowing the workspace, small again
SUBFRAMES = (1, 8, 1)


def _on_one_and_on_fresh(make, call, sizes):
    """call(obj, size index) on one object for every size, and each on an object of its own"""
    one = make()
    got = [call(one, i) for i in range(len(sizes))]
    one.close()
    for i in range(len(sizes)):
        fresh = make()
        want = call(fresh, i)
        fresh.close()
        assert len(got[i]) == len(want)
        for k, (g, w) in enumerate(zip(got[i], want)):
            assert g.tobytes() == w.tobytes(), (i, sizes[i], k)


@pytest.mark.parametrize("K", [40, 512, 1008])  # generic, 8-window and 16-window decoders
def test_tdec_batch_regrow(K):
    rng = np.random.default_rng(K)
    bufs = [rng.integers(-96, 97, (n, tdec_buf_len(K)), dtype=np.int16) for n in SIZES]
    _on_one_and_on_fresh(TdecBatch, lambda dec, i: [dec.run(bufs[i], K, 4)], SIZES)


@pytest.mark.parametrize("K", [1008, 2112])  # 16-window and 32-window 8-bit decoders
def test_tdec8_batch_regrow(K):
    rng = np.random.default_rng(8 * K)
    stride = (tdec_buf_len(K) + 255) // 256 * 256
    bufs = [rng.integers(-40, 41, (n, stride), dtype=np.int8) for n in SIZES]

    def call(dec, i):
        n = SIZES[i]
        d_in = DeviceBuffer(bufs[i].nbytes).upload(bufs[i])
        d_out = DeviceBuffer(n * (K // 8))
        assert dec.run_dev(d_in.ptr, stride, n, K, 4, d_out.ptr, K // 8) == 0
        return [d_out.download(np.zeros((n, K // 8), np.uint8))]

    _on_one_and_on_fresh(Tdec8Batch, call, SIZES)


def test_enb_dl_regrow():
    base = pc.Cfg(nof_prb=6, cfi=2, qm=[4], tbs=[pc.valid_tbs(1500)])
    sf_of = (1, 2, 3, 4, 6, 7, 8, 9)
    rng = np.random.default_rng(6)
    payloads = [[rng.integers(0, 256, base.tbs[0] // 8, dtype=np.uint8) for _ in range(n)] for n in SUBFRAMES]

    def call(enb, i):
        jobs, keep = [], []
        for s, pl in enumerate(payloads[i]):
            cfg = pc.Cfg(**{**base.__dict__, "sf_idx": sf_of[s], "rnti": 0x100 + s})
            d_pl = [DeviceBuffer(pl.nbytes).upload(pl)]
            d_g = [dev_zeros(cfg.grid_len * 8) for _ in range(cfg.nof_ports)]
            keep.append((d_pl, d_g))
            jobs.append(enb_job(cfg, d_pl, d_g))
        enb.put_pdsch(jobs)
        return [g.download(np.zeros(base.grid_len, np.complex64)) for _, d_g in keep for g in d_g]

    _on_one_and_on_fresh(lambda: enb_dl.EnbDl(cell_of(base)), call, SUBFRAMES)


def test_pdcch_search_regrow():
    nprb, ports, nrx, cid = 6, 2, 2, 5
    cell = P.make_cell(nprb, ports, cid)
    G = 14 * 12 * nprb
    rng = np.random.default_rng(66)

    def cplx(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)

    sets = []  # per call: jobs, noise estimates and the device buffers the jobs point into
    for n in SUBFRAMES:
        jobs, keep = [], []
        chest = (ChestRes * n)()
        for s in range(n):
            y, h = cplx(nrx, G), cplx(ports, nrx, G)
            bufs = [DeviceBuffer(G * 8).upload(y[r]) for r in range(nrx)]
            bufs += [DeviceBuffer(G * 8).upload(h[p, r]) for p in range(ports) for r in range(nrx)]
            j = DlSfJob()
            j.tti = s
            for r in range(nrx):
                j.sf_symbols[r] = bufs[r].ptr
                for p in range(ports):
                    j.ce[p][r] = bufs[nrx + p * nrx + r].ptr
            chest[s].noise_estimate = 0.5
            jobs.append(j)
            keep.append(bufs)
        sets.append((jobs, chest, keep))

    def call(ue, i):
        jobs, chest, _keep = sets[i]
        n = len(jobs)
        cfis, ctrl, _dcis = D.find_dl_dci(ue, jobs, [0x3C1A] * n, [D.UeDlCfg()] * n, chest)
        out = [np.array(cfis, np.uint32), np.frombuffer(bytes(ctrl), np.uint8)]
        for s in range(n):
            cand = D.last_candidates(ue, s).copy()
            # the kernel writes what a slot's status defines (pdcch_internal.h DciCand): 0 nothing more,
            # 1 the location, 2 everything
            cand["crc_rem"][cand["status"] < 2] = 0
            cand["bits"][cand["status"] < 2] = 0
            cand["L"][cand["status"] < 1] = 0
            cand["ncce"][cand["status"] < 1] = 0
            out += [D.last_llr(ue, s), cand]
        return out

    _on_one_and_on_fresh(lambda: UeDl(cell, nrx), call, SUBFRAMES)
