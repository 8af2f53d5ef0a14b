"""GPU: eviction of the PDSCH receiver's two device caches -- the RE extraction maps (one per allocation, cfi and
subframe) and the packed descrambling sequences (one per c_init) -- with their bounds lowered through
mi355_pdsch_debug_set_cache_limits so that a handful of jobs reaches them.

A map handed to a job of a batch must stay intact until the next call on the receiver begins: the bound is applied
once per call, before planning.  (Evicting while a batch was being planned handed the buffers of its earlier jobs to
its later ones, which overwrote them before any kernel ran.)  All allocations of the map tests have the same RE count,
so a job reading another allocation's map shows as a mismatch here, never as an access outside a buffer.

15 PRB, 1 port, 1 rx antenna, QPSK, 28 dB; equalised symbols, CSI and LLRs bit-exact against oracle.pdsch_chain."""
import functools

import numpy as np
import pytest

from oracle import pdsch_chain as pc
from srsran_amd import pdsch as P
from srsran_amd.dlsch import SoftbufferPool
from tests.pdsch_jobs import DevSubframe, cell_of, grant_of

NPRB = 15
TBS = pc.valid_tbs(600)


def alloc(first: int, n: int = 6) -> tuple:
    return tuple(int(first <= p < first + n) for p in range(NPRB))


ALLOCS = {name: alloc(i) for i, name in enumerate("ABCDEF")}  # six PRBs each: the same RE count
ALLOCS["s"] = alloc(9, 4)  # a smaller one: its map fits a recycled buffer of the others


@functools.lru_cache(maxsize=None)
def case(name: str, rnti: int = 0x1234, csi: bool = False):
    """(cfg, subframe, oracle (d, csi, e)) of one allocation and RNTI: computed once, shared, read-only."""
    prb = np.array([ALLOCS[name]] * 2, np.uint8)
    cfg = pc.Cfg(nof_prb=NPRB, nof_ports=1, nof_rx=1, scheme=0, nof_layers=1, qm=[2], tbs=[TBS], prb=prb, rnti=rnti,
                 csi_enable=csi)
    seed = 5000 + 97 * sorted(ALLOCS).index(name) + rnti
    sf = pc.synth_subframe(cfg, np.random.default_rng(seed), snr_db=28, channel="static")
    return cfg, sf, pc.rx_front(cfg, sf.y, sf.ce, sf.noise)


def run_batch(pd, pool, cases, tag, fused=False):
    """Decode the cases as one batch; per job: the device map it was planned with is its allocation's, jobs of
    different allocations have different maps, d / csi / e equal the oracle's, CRC ok, payload equal.  fused: through
    pdsch_eq_rm, whose LLRs the debug stage regenerates from the same maps (no d or csi to read)."""
    pool.reset_all()
    pd.set_ce_invariant(fused)
    subs = [DevSubframe(cfg, sf, softbuffers=(j,)) for j, (cfg, sf, _) in enumerate(cases)]
    res = pd.decode(pool, [s.job for s in subs])
    ptrs = []
    for j, (cfg, sf, (d_o, csi_o, e_o)) in enumerate(cases):
        what = f"{tag} job {j}"
        ptr, dev_map = pd.debug_job_map(j)
        host_map = P.re_map(cell_of(cfg), grant_of(cfg), cfg.cfi, cfg.sf_idx)
        assert host_map.size == sf.nof_re
        np.testing.assert_array_equal(dev_map, host_map, err_msg=what)
        ptrs.append(ptr)
        d, csi, e = pd.stage(j, 0, sf.nof_re, sf.nof_re * 2)
        if not fused:
            np.testing.assert_array_equal(d.view(np.uint32), d_o[0].view(np.uint32), err_msg=what)
            np.testing.assert_array_equal(csi.view(np.uint32), csi_o[0][:sf.nof_re].view(np.uint32), err_msg=what)
        np.testing.assert_array_equal(e, e_o[0], err_msg=what)
        assert res[2 * j].ret == 0 and res[2 * j].crc, what
        np.testing.assert_array_equal(subs[j].payload_bytes(0)[:TBS // 8], sf.payload[0], err_msg=what)
    for i in range(len(cases)):
        for j in range(i):
            if cases[i][0].prb_mask().tobytes() != cases[j][0].prb_mask().tobytes():
                assert ptrs[i] != ptrs[j], (tag, i, j)


def test_allocations_share_the_re_count():
    n = {name: case(name)[1].nof_re for name in "ABCDEF"}
    assert len(set(n.values())) == 1 and case("s")[1].nof_re < n["A"]
    assert len({ALLOCS[a] for a in ALLOCS}) == len(ALLOCS)


@pytest.mark.gpu
def test_map_cache_bound_reached_within_a_batch():
    """max_maps = 3, eight jobs over six allocations: the bound is passed while the batch is planned."""
    pd = P.Pdsch(cell_of(case("A")[0]), 1)
    pd.debug_set_cache_limits(max_maps=3)
    pool = SoftbufferPool(8, max_cb=2)
    run_batch(pd, pool, [case(a) for a in "ABCDEFAD"], "batch 0")
    pd.close()
    pool.close()


@pytest.mark.gpu
def test_map_cache_eviction_across_batches_reuses_buffers():
    """Every call after the first starts over the bound: its maps are rebuilt in recycled buffers, a smaller map in
    a larger buffer, while the previous call's buffers are no longer read -- two-kernel path and pdsch_eq_rm."""
    pd = P.Pdsch(cell_of(case("A")[0]), 1)
    pd.debug_set_cache_limits(max_maps=3)
    pool = SoftbufferPool(8, max_cb=2)
    for b, (order, fused) in enumerate((("ABCDEFAD", False), ("FsEDCBAs", False), ("sABsCD", True), ("DCsA", True),
                                        ("EFsBAC", False))):
        run_batch(pd, pool, [case(a, csi=fused) for a in order], f"batch {b}", fused=fused)
    pd.close()
    pool.close()


@pytest.mark.gpu
def test_sequence_cache_eviction():
    """max_scr = 2, three batches of three jobs with new RNTIs, the last with one RNTI of the first: after eviction
    the sequences are generated again into fresh buffers."""
    pd = P.Pdsch(cell_of(case("A")[0]), 1)
    pd.debug_set_cache_limits(max_scr=2)
    pool = SoftbufferPool(8, max_cb=2)
    for b, rntis in enumerate(((101, 102, 103), (104, 105, 106), (107, 101, 108))):
        run_batch(pd, pool, [case("ABC"[j], rnti=r) for j, r in enumerate(rntis)], f"batch {b}")
    pd.close()
    pool.close()
