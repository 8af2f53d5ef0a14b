"""GPU: mi355_pdsch_decode_launch / mi355_pdsch_decode_collect -- the batch decode in two halves, with two
iteration-count groups in flight on one stream.

Three jobs (the shapes of tests/test_pdsch_caches_gpu.py: 15 PRB, 1 port, 1 rx antenna, QPSK, six-PRB allocations,
28 dB) with max_nof_iterations 2, 0, 10: the setting persists, so the DL-SCH decodes {2: jobs 0 and 1} and then
{10: job 2}, each group's results left in flight until collect."""
import numpy as np
import pytest

from srsran_amd import pdsch as P
from srsran_amd.dlsch import SoftbufferPool
from tests.pdsch_jobs import DevSubframe, cell_of
from tests.test_pdsch_caches_gpu import TBS, case

ITS = (2, 0, 10)
MI355_ERROR = -1


def subframes(cases, first_sb):
    subs = [DevSubframe(cfg, sf, softbuffers=(first_sb + j,)) for j, (cfg, sf, _) in enumerate(cases)]
    for s, its in zip(subs, ITS):
        s.job.cfg.max_nof_iterations = its
    return subs


@pytest.mark.gpu
def test_launch_then_collect_equals_decode_batch():
    cases = [case(a) for a in "ABC"]
    pd = P.Pdsch(cell_of(cases[0][0]), 1)
    pool = SoftbufferPool(8, max_cb=2)
    subs = subframes(cases, 0)
    r, res = pd.decode_launch(pool, [s.job for s in subs])
    assert r == 0
    # (a) one launch may be outstanding per receiver
    assert pd.decode_launch(pool, [s.job for s in subs])[0] == MI355_ERROR
    # (b) collect fills the results of both groups
    assert pd.decode_collect() == 0
    for j, (cfg, sf, _) in enumerate(cases):
        assert res[2 * j].ret == 0 and res[2 * j].crc, j
        np.testing.assert_array_equal(subs[j].payload_bytes(0)[:TBS // 8], sf.payload[0], err_msg=f"job {j}")
    got = [(res[2 * j].crc, res[2 * j].ret, res[2 * j].avg_iterations_block) for j in range(3)]
    # (d) nothing left to collect: success, results untouched
    assert pd.decode_collect() == 0
    assert got == [(res[2 * j].crc, res[2 * j].ret, res[2 * j].avg_iterations_block) for j in range(3)]
    # (c) the same jobs through mi355_pdsch_decode_batch, fresh softbuffers
    again = subframes(cases, 3)
    ref = pd.decode(pool, [s.job for s in again])
    assert got == [(ref[2 * j].crc, ref[2 * j].ret, ref[2 * j].avg_iterations_block) for j in range(3)]
    for j, (cfg, sf, _) in enumerate(cases):
        np.testing.assert_array_equal(again[j].payload_bytes(0)[:TBS // 8], sf.payload[0], err_msg=f"batch job {j}")
    pd.close()
    pool.close()
