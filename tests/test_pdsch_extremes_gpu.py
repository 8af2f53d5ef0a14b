"""GPU: every LLR path of the PDSCH front end on inputs that saturate int16 / int8, wrap in the scalar tails and leave
the int32 range of the x86 conversions the kernels restate (x86_cvt_i32, sat16 against f2s_trunc, wrap16 / abs16, the
wrapping add_pairs16 of HARQ combining) -- bit-exact against oracle.pdsch_chain.rx_front / rx_decode and
oracle.Softbuffer, no tolerances.  The demappers of both checkers are pinned to the compiled reference at these
amplitudes by tests/golden/demod_extremes.npz (test_pdsch_oracle.py::test_demod_extremes_golden).

Inputs: pc.synth_subframe(cfg, default_rng(1200 + k), 25 dB, static channel), then every grid RE of y times a gain from
{1, 1, 1, 40, 300, 3e5, 1e9, 0} and the estimates times a gain from {1, 1, 0.03, 30, 0} per (port, rx antenna, PRB),
the same in all 14 symbols so they stay row-invariant (no 0 for the ZF job: 0 / 0).  Only finite inputs: the order
of NaN and Inf through the reference's equaliser is not pinned to the reference, so nothing is claimed about it.
The transport blocks are garbage and fail their CRCs -- the decoder must fail the same way as the oracle's.

Paths: (1) pdsch_equalize + pdsch_llr, every scheme; (2) the fused pdsch_eq_llr; (3) pdsch_eq_rm, two transmissions
(fresh buffers, then the read-modify-write path with wrapping int16 sums); (4) the same decode through pdsch_eq_llr +
dlsch_rm_rx (MI355_NO_EQRM); (5) the 8-bit LLRs against tests/llr8_ref.py."""
import functools

import numpy as np
import pytest

import oracle
from oracle import pdsch_chain as pc
from srsran_amd import pdsch as P
from srsran_amd.dlsch import SoftbufferPool
from tests import llr8_ref
from tests.pdsch_jobs import DevSubframe, cell_of, pool_softbuffer_check

Y_GAINS = (1.0, 1.0, 1.0, 40.0, 300.0, 3e5, 1e9, 0.0)
H_GAINS = (1.0, 1.0, 0.03, 30.0, 0.0)


def eqrm_tbs(nof_re: int, qm: int) -> int:
    """The smallest TBS the tables could give (pc.valid_tbs: no filler bits, one code-block size) whose code blocks
    take their share of nof_re * qm LLRs without wrap-around, E <= 3 K + 12: what pdsch_eq_rm asks of a job."""
    for t in range(16, 75376, 8):
        if pc.valid_tbs(t) != t:
            continue
        s = oracle.cbsegm(t)
        if qm * (nof_re // s["C"]) + qm <= 3 * s["K1"] + 12:
            return t
    raise ValueError((nof_re, qm))


def _nre(**kw) -> int:
    c = pc.Cfg(**kw)
    return int(oracle.pdsch_re_map(c.nof_prb, c.nof_ports, c.cell_id, c.prb_mask(), c.lstart, c.sf_idx).size)


_SISO = dict(nof_prb=25, nof_ports=1, nof_rx=1)  # cfi 2, sf 3: 3450 REs, a scalar tail at every modulation
_SM25 = dict(nof_prb=25, nof_ports=2, nof_rx=2)
_SM27 = dict(nof_prb=27, nof_ports=2, nof_rx=2, sf_idx=0)
_SM6 = dict(nof_prb=6, nof_ports=2, nof_rx=2, cfi=3)
CFGS = [
    pc.Cfg(**_SISO, scheme=0, nof_layers=1, qm=[2], tbs=[eqrm_tbs(_nre(**_SISO), 2)]),
    pc.Cfg(**_SISO, scheme=0, nof_layers=1, qm=[4], tbs=[eqrm_tbs(_nre(**_SISO), 4)], csi_enable=True),
    pc.Cfg(**{**_SISO, "nof_rx": 2}, scheme=0, nof_layers=1, qm=[6], tbs=[eqrm_tbs(_nre(**_SISO), 6)]),
    pc.Cfg(nof_prb=15, nof_ports=2, nof_rx=1, scheme=1, nof_layers=2, qm=[2], tbs=[1480], sf_idx=5, csi_enable=True),
    pc.Cfg(nof_prb=25, nof_ports=2, nof_rx=2, scheme=1, nof_layers=2, qm=[6], tbs=[6968], power_scale=True,
           p_a=-3.0, p_b=1),
    pc.Cfg(**_SM25, scheme=2, nof_layers=2, qm=[8, 8], tbs=[9912, 9912], csi_enable=True),
    pc.Cfg(**_SM25, scheme=2, nof_layers=2, qm=[2, 6], tbs=[1480, 5992], pmi=0),
    pc.Cfg(**_SM27, scheme=2, nof_layers=2, qm=[4, 4], tbs=[eqrm_tbs(_nre(**_SM27), 4)] * 2, pmi=1, csi_enable=True,
           mmse=False),
    pc.Cfg(nof_prb=15, nof_ports=2, nof_rx=2, scheme=3, nof_layers=2, qm=[2, 2], tbs=[1480, 1480], sf_idx=5),
    pc.Cfg(**_SM6, scheme=2, nof_layers=1, qm=[4], tbs=[eqrm_tbs(_nre(**_SM6), 4)], pmi=3, csi_enable=True),
    pc.Cfg(**_SM6, scheme=2, nof_layers=2, qm=[8, 8], tbs=[eqrm_tbs(_nre(**_SM6), 8)] * 2, pmi=1),
]
ALL = list(range(len(CFGS)))
FUSED = [k for k in ALL if CFGS[k].scheme in (0, 2)]
# pdsch_eq_rm: fused, one TBS and one modulation per job, no filler bits, E <= 3 K + 12 (the TBS chosen above)
EQRM = [k for k in FUSED if len(set(CFGS[k].qm)) == 1 and len(set(CFGS[k].tbs)) == 1]
LLR8 = [0, 1, 2, 3, 5]  # QPSK, 16QAM, 64QAM, QPSK through SFBC, 256QAM
QPSK_SCALE_8BIT = 20 * np.sqrt(2.0)  # the smallest factor any demapper applies before converting to an integer


@functools.lru_cache(maxsize=None)
def subframe(k: int) -> pc.Subframe:
    cfg = CFGS[k]
    rng = np.random.default_rng(1200 + k)
    sf = pc.synth_subframe(cfg, rng, snr_db=25, channel="static")
    y = (sf.y * rng.choice(np.array(Y_GAINS, np.float32), sf.y.shape)).astype(np.complex64)
    hg = np.array(H_GAINS if cfg.mmse else H_GAINS[:-1], np.float32)
    g = rng.choice(hg, (cfg.nof_ports, cfg.nof_rx, cfg.nof_prb))
    ce = (sf.ce * np.tile(np.repeat(g, 12, axis=2), (1, 1, 14))).astype(np.complex64)
    for a in (y, ce):
        a.setflags(write=False)
    return pc.Subframe(y, ce, sf.noise, sf.payload, sf.idx, sf.nof_re)


@functools.lru_cache(maxsize=None)
def front(k: int):
    """The oracle's (d[cw], csi[cw], e[tb]) of configuration k, computed once and shared."""
    sf = subframe(k)
    d, csi, e = pc.rx_front(CFGS[k], sf.y, sf.ce, sf.noise)
    for a in list(d) + list(csi) + list(e):
        a.setflags(write=False)
    return d, csi, e


def test_inputs_reach_the_saturating_and_out_of_range_code():
    """What the GPU tests below rely on, from the oracle alone: every d and csi finite, LLRs at +-32767 / -32768 in
    every job without CSI weighting, symbols beyond int32 even at the smallest demapper scale in every job, and QPSK,
    16QAM and 64QAM each in a job whose RE count leaves a scalar tail."""
    tails = set()
    for k, cfg in enumerate(CFGS):
        sf = subframe(k)
        assert np.array_equal(sf.ce[:, :, :12 * cfg.nof_prb], sf.ce[:, :, -12 * cfg.nof_prb:])  # row-invariant
        d, csi, e = front(k)
        ncw = cfg.nof_layers if cfg.scheme in (2, 3) else 1
        for cw in range(ncw):
            assert np.isfinite(d[cw].view(np.float32)).all() and np.isfinite(csi[cw]).all(), (k, cw)
        for t in range(cfg.nof_tb):
            comp = np.abs(d[t].view(np.float32)).astype(np.float64)
            assert (comp * QPSK_SCALE_8BIT >= 2.0 ** 31).mean() > 0, (k, t)
            if not cfg.csi_enable:
                assert ((e[t] == 32767) | (e[t] <= -32767)).mean() > 0, (k, t)
            if sf.nof_re % (8 if cfg.qm[t] == 2 else 4):
                tails.add(cfg.qm[t])
    assert {2, 4, 6} <= tails
    # pdsch_eq_rm: one-layer (circular image) and two-layer (compact image) jobs, each kind with and without CSI
    # weighting -- without it the LLRs reach +-32767 and the second transmission's int16 sums wrap
    assert {(CFGS[k].nof_tb, CFGS[k].csi_enable) for k in EQRM} == {(1, False), (1, True), (2, False), (2, True)}
    assert {q for k in LLR8 for q in CFGS[k].qm} == {2, 4, 6, 8}
    assert all(subframe(k).nof_re % 8 and subframe(k).nof_re > 8 for k in LLR8)  # an 8-symbol body and a tail


def _stage_equal(pd, k, what="dce"):
    cfg, sf = CFGS[k], subframe(k)
    d_o, csi_o, e_o = front(k)
    nre = sf.nof_re
    ncw = cfg.nof_layers if cfg.scheme in (2, 3) else 1
    for cw in range(ncw):
        d, csi, e = pd.stage(0, cw, nre, nre * cfg.qm[cw] if cw < cfg.nof_tb else None)
        if "d" in what:
            np.testing.assert_array_equal(d.view(np.uint32), d_o[cw].view(np.uint32), err_msg=f"d {k} {cw}")
        if "c" in what:
            np.testing.assert_array_equal(csi.view(np.uint32), csi_o[cw][:nre].view(np.uint32), err_msg=f"csi {k} {cw}")
        if cw < cfg.nof_tb:
            np.testing.assert_array_equal(e, e_o[cw], err_msg=f"e {k} {cw}")


@pytest.mark.gpu
@pytest.mark.parametrize("k", ALL)
def test_two_kernel_path(k):
    """pdsch_equalize + pdsch_llr: equalised symbols, CSI and LLRs of every scheme."""
    cfg = CFGS[k]
    ds = DevSubframe(cfg, subframe(k))
    pd = P.Pdsch(cell_of(cfg), cfg.nof_rx)
    pd.frontend([ds.job])
    _stage_equal(pd, k)
    pd.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", FUSED)
def test_fused_eq_llr(k):
    """pdsch_eq_llr (row-invariant estimates, port 0 / spatial multiplexing): its LLRs -- the kernel keeps the
    equalised symbols and the CSI in registers, so there is no d or csi to read back."""
    cfg = CFGS[k]
    ds = DevSubframe(cfg, subframe(k))
    pd = P.Pdsch(cell_of(cfg), cfg.nof_rx)
    pd.set_ce_invariant(True)
    pd.frontend([ds.job])
    _stage_equal(pd, k, what="e")
    pd.close()


def _wrapped(before: np.ndarray, e: np.ndarray, cfg: pc.Cfg, t: int, rv: int) -> bool:
    """Did combining e (as rv) into the oracle buffers `before` overflow an int16 sum somewhere?"""
    C = oracle.cbsegm(cfg.tbs[t])["C"]
    add = np.zeros(C * oracle.SOFTBUFFER_SIZE, np.int16)
    ee = np.ascontiguousarray(e, np.int16)
    assert oracle.lib().orc_dlsch_rm_tb(ee, ee.size, cfg.tbs[t], cfg.qm[t], rv, add, oracle.SOFTBUFFER_SIZE) == C
    s = before[:C].reshape(-1).astype(np.int32) + add.astype(np.int32)
    return bool(((s > 32767) | (s < -32768)).any())


def _two_transmissions(k: int, eqrm: bool):
    cfg, sf = CFGS[k], subframe(k)
    _d, _csi, e_o = front(k)
    pool = SoftbufferPool(2, max_cb=4)
    pd = P.Pdsch(cell_of(cfg), cfg.nof_rx)
    pd.set_ce_invariant(True)
    sbs = [oracle.Softbuffer(4) for _ in cfg.tbs]
    wrapped = False
    P.eqrm_profile(True)
    try:
        for rv in (0, 2):  # the same I/Q again as rv 2, no reset: read-modify-write of the buffers of rv 0
            c = pc.Cfg(**{**cfg.__dict__, "rv": [rv, rv]})
            ds = DevSubframe(c, sf, softbuffers=(0, 1))
            res = pd.decode(pool, [ds.job])
            if rv:
                wrapped = any(_wrapped(sbs[t].buf, e_o[t], c, t, rv) for t in range(cfg.nof_tb))
            want = pc.rx_decode(c, e_o, sbs)
            for t in range(cfg.nof_tb):
                ret, _data, its = want[t]
                assert res[t].ret == 0, (k, rv, t)
                assert bool(res[t].crc) == (ret == 0), (k, rv, t)
                assert res[t].avg_iterations_block == np.float32(its), (k, rv, t)
                C = oracle.cbsegm(cfg.tbs[t])["C"]
                pool_softbuffer_check(pool, t, sbs[t].buf[:C], cfg.tbs[t], (k, rv, t))
    finally:
        groups = int(P.eqrm_profile(False)[0])
    # 32767 + 32767 = -2 somewhere (CSI weighting multiplies by at most 32767 / 65536: such sums cannot overflow)
    assert wrapped or cfg.csi_enable, k
    assert (groups > 0) == eqrm, (k, groups)
    pd.close()
    pool.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", EQRM)
def test_eq_rm_two_transmissions(k, monkeypatch):
    """pdsch_eq_rm (proved to have run by its workgroup counter): decoder buffers of every code block, return codes,
    CRCs and iteration counts after rv 0 into fresh buffers and after rv 2 combined into them.  Two-layer jobs take
    the compact image, one-layer jobs the circular one."""
    monkeypatch.delenv("MI355_NO_EQRM", raising=False)
    _two_transmissions(k, True)


@pytest.mark.gpu
@pytest.mark.parametrize("k", EQRM)
def test_eq_llr_rm_rx_two_transmissions(k, monkeypatch):
    """The same decode with MI355_NO_EQRM: pdsch_eq_llr + dlsch_rm_rx."""
    monkeypatch.setenv("MI355_NO_EQRM", "1")
    _two_transmissions(k, False)


@pytest.mark.gpu
@pytest.mark.parametrize("k", LLR8)
def test_8bit_llrs(k):
    """mi355_pdsch_set_llr_8bit: the int8 LLRs against tests/llr8_ref.py on the GPU's own equalised symbols and CSI
    (themselves equal to the oracle's: checked here too), SIMD bodies and scalar tails."""
    cfg, sf = CFGS[k], subframe(k)
    ds = DevSubframe(cfg, sf)
    pd = P.Pdsch(cell_of(cfg), cfg.nof_rx)
    pd.set_llr_8bit(True)
    pd.frontend([ds.job])
    d_o, csi_o, _e = front(k)
    for t in range(cfg.nof_tb):
        qm = cfg.qm[t]
        d, csi, e8 = pd.stage(0, t, sf.nof_re, sf.nof_re * qm)
        np.testing.assert_array_equal(d.view(np.uint32), d_o[t].view(np.uint32), err_msg=f"d {k} {t}")
        np.testing.assert_array_equal(csi.view(np.uint32), csi_o[t][:sf.nof_re].view(np.uint32), err_msg=f"csi {k} {t}")
        want = llr8_ref.demod_b(d, qm)
        c = oracle.sequence_lte(oracle.pdsch_c_init(cfg.rnti, t, cfg.sf_idx, cfg.cell_id), sf.nof_re * qm)
        want = llr8_ref.scramble_sb(want, c)
        if cfg.csi_enable:
            want = llr8_ref.csi_b(want, csi, qm)
        np.testing.assert_array_equal(e8, want, err_msg=f"cfg {k} tb {t}")
    pd.close()
