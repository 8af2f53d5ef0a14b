"""GPU: pdsch_eq_rm (equaliser, LLRs and rate dematching in one kernel) at every code-block size an allocation exists
for, bit-exact against the oracle chain (oracle.pdsch_chain.rx_front / rx_decode into oracle.Softbuffer), with the
machinery of tests/test_pdsch_extremes_gpu.py.  Its compact decoder-order tables (dlsch_rm_compact, keyed by (K, rv, E))
met the oracle at a handful of (K, rv, E) only.

Per size K one job of single-block TBs (tbs = K - 24) in a 6-PRB (cfi 3: 108 REs per PRB) or a 15-PRB cell (132 REs per
PRB), two ports, two receive antennas, the first n PRBs allocated: the modulation cycles over QPSK / 16QAM / 64QAM /
256QAM with the size and falls back to a lower one, n is the largest with E + Qm = (REs + 1) Qm <= 3 K + 12 (what
plan_eq_rm asks), the cell alternates where both fit.  Two-layer spatial multiplexing with two equal TBs takes the
compact image, one-layer jobs the circular one.  Sizes without an allocation: LEFT_OUT, those whose 3 K + 12 is below
one PRB's QPSK LLRs (218).  One subframe per job (static channel, 25 dB) serves every rv: the rate dematching is what
is under test, so at rv != 0 the blocks fail, as the oracle's do."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import rm_inputs as RI
import tdec_inputs as TI
from oracle import pdsch_chain as pc
from srsran_amd import pdsch as P
from srsran_amd.dlsch import SoftbufferPool
from tests.pdsch_jobs import DevSubframe, cell_of, dirty_pool, pool_softbuffer_check

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CELLS = {6: dict(nof_prb=6, nof_ports=2, nof_rx=2, cfi=3), 15: dict(nof_prb=15, nof_ports=2, nof_rx=2)}
LEFT_OUT = (40, 48, 56, 64)
KINDS = ("two_layer", "one_layer")


def _prb(nof_prb: int, n: int) -> np.ndarray:
    m = np.zeros((2, nof_prb), np.uint8)
    m[:, :n] = 1
    return m


@functools.lru_cache(maxsize=None)
def _nre(cell: int, n: int) -> int:
    c = pc.Cfg(**CELLS[cell], prb=_prb(cell, n))
    return int(oracle.pdsch_re_map(c.nof_prb, c.nof_ports, c.cell_id, c.prb_mask(), c.lstart, c.sf_idx).size)


@functools.lru_cache(maxsize=None)
def allocation(i: int):
    """(cell, PRBs, qm) of size number i, or None"""
    N = RI.N_of(TI.CB_SIZES[i])
    pref = (2, 4, 6, 8)[i % 4]
    for qm in [pref] + [q for q in (6, 4, 2) if q < pref]:
        for cell in ((6, 15) if i % 2 == 0 else (15, 6)):
            fit = [n for n in range(1, cell + 1) if (_nre(cell, n) + 1) * qm <= N]
            if fit:
                return cell, fit[-1], qm
    return None


def _cfg(kind: str, cell: int, n: int, qm: int, tbs: int, rv: int = 0) -> pc.Cfg:
    if kind == "two_layer":
        return pc.Cfg(**CELLS[cell], scheme=2, nof_layers=2, qm=[qm, qm], tbs=[tbs, tbs], rv=[rv, rv], pmi=n % 2,
                      prb=_prb(cell, n), csi_enable=bool(n % 2))
    return pc.Cfg(**CELLS[cell], scheme=2, nof_layers=1, qm=[qm], tbs=[tbs], rv=[rv, rv], pmi=n % 4,
                  prb=_prb(cell, n), csi_enable=bool(n % 2))


@functools.lru_cache(maxsize=None)
def _job(kind: str, cell: int, n: int, qm: int, tbs: int):
    """(subframe, oracle LLRs per TB) of one job, computed once for every rv"""
    cfg = _cfg(kind, cell, n, qm, tbs)
    sf = pc.synth_subframe(cfg, np.random.default_rng([61, cell, n, qm, tbs, KINDS.index(kind)]), snr_db=25,
                           channel="static")
    _d, _csi, e = pc.rx_front(cfg, sf.y, sf.ce, sf.noise)
    for a in e:
        a.setflags(write=False)
    return sf, e


def test_allocations_cover():
    """Every size but LEFT_OUT has an allocation; both cells, the four modulations, E from a twentieth of N to nearly N,
    and E both below and above the 16-window sizes' sparse interval occur."""
    left, cells, qms, ratio, sparse = [], set(), set(), [], set()
    for i, K in enumerate(TI.CB_SIZES):
        a = allocation(i)
        if a is None:
            left.append(K)
            continue
        cell, n, qm = a
        E = _nre(cell, n) * qm
        assert E + qm <= RI.N_of(K)
        cells.add(cell)
        qms.add(qm)
        ratio.append(E / RI.N_of(K))
        for rv in RI.RVS:
            sparse.add((TI.nsb(K), RI.features(K, rv, E, 0)["sparse"]))
    assert tuple(left) == LEFT_OUT and all(RI.N_of(K) < 218 for K in LEFT_OUT)
    assert cells == {6, 15} and qms == {2, 4, 6, 8}
    assert min(ratio) < 0.3 and max(ratio) > 0.95, (min(ratio), max(ratio))
    assert sparse == {(0, False), (8, False), (16, False), (16, True)}


def _run_jobs(kind: str, specs, rvs, max_cb: int, eqrm: bool):
    """specs: [(cell, n, qm, tbs)], job j at rvs[j] into fresh buffers, then the same I/Q as (rv + 2) % 4 combined.
    Buffers of the even jobs are read (and so materialized) after the first transmission too; those of the odd jobs
    only after the combine, which then meets the rows the fresh write left unwritten."""
    bad = []
    for cell in sorted({s[0] for s in specs}):
        idx = [j for j, s in enumerate(specs) if s[0] == cell]
        ntb = 2 if kind == "two_layer" else 1
        pool = SoftbufferPool(2 * len(idx), max_cb=max_cb)
        dirty_pool(pool)  # (rows a fresh write leaves unwritten hold -32768, not a new allocation's zeros)
        pd = P.Pdsch(cell_of(pc.Cfg(**CELLS[cell])), 2)
        pd.set_ce_invariant(True)
        sbs = {j: [oracle.Softbuffer(max_cb) for _ in range(ntb)] for j in idx}
        for tx in range(2):
            devs, cfgs = [], []
            for k, j in enumerate(idx):
                _c, n, qm, tbs = specs[j]
                cfg = _cfg(kind, cell, n, qm, tbs, (rvs[j] + 2 * tx) % 4)
                cfgs.append(cfg)
                devs.append(DevSubframe(cfg, _job(kind, *specs[j])[0], softbuffers=(2 * k, 2 * k + 1)))
            # pdsch_eq_rm runs one workgroup per (job, code block) that some TB of the job has yet to decode; one
            # ineligible job or one failed table look-up sends the whole call down the two-kernel path (0 groups)
            groups = sum(int(any(not sbs[j][t].cb_crc[c] for t in range(ntb)))
                         for j in idx for c in range(oracle.cbsegm(specs[j][3])["C"]))
            P.eqrm_profile(True)
            try:
                res = pd.decode(pool, [d.job for d in devs])
            finally:
                ran = int(P.eqrm_profile(False)[0])
            assert ran == (groups if eqrm else 0), (cell, tx, ran, groups)
            for k, j in enumerate(idx):
                want = pc.rx_decode(cfgs[k], _job(kind, *specs[j])[1], sbs[j])
                for t in range(ntb):
                    ret, _data, its = want[t]
                    r = res[2 * k + t]
                    if r.ret != 0 or bool(r.crc) != (ret == 0) or r.avg_iterations_block != np.float32(its):
                        bad.append((specs[j], tx, t, "result", r.ret, bool(r.crc), ret, r.avg_iterations_block, its))
                    if tx == 0 and j % 2:
                        continue
                    C = oracle.cbsegm(specs[j][3])["C"]
                    try:
                        pool_softbuffer_check(pool, 2 * k + t, sbs[j][t].buf[:C], specs[j][3], (specs[j], tx, t))
                    except AssertionError as e:
                        bad.append(("buffer",) + e.args)
        pd.close()
        pool.close()
    assert not bad, (len(bad), bad[:8])


def _eqrm_expected() -> bool:
    return not os.environ.get("MI355_NO_EQRM")


@gpu
@pytest.mark.parametrize("rv", RI.RVS)
@pytest.mark.parametrize("kind", KINDS)
def test_eq_rm_every_size(kind, rv):
    """The 184 sizes with an allocation, job of size number i at rv (rv + i) % 4 into fresh buffers and then combined
    as (rv + 2) % 4: return codes, CRCs, iteration counts and the decoder buffers are the oracle's; pdsch_eq_rm ran
    (its workgroup counter), unless MI355_NO_EQRM is set, in which case it did not."""
    specs, rvs = [], []
    for i, K in enumerate(TI.CB_SIZES):
        a = allocation(i)
        if a is not None:
            specs.append(a + (K - 24,))
            rvs.append((rv + i) % 4)
    assert len(specs) == 188 - len(LEFT_OUT)
    _run_jobs(kind, specs, rvs, 1, _eqrm_expected())


# (PRBs of the 15-PRB cell, qm, tbs): C = 5 and 7 with gamma = REs % C != 0 -- the E and E + Qm compact tables -- one
# of them with two code-block sizes
def _multi_specs():
    two5 = next(t for t in RI.two_size_tbs() if oracle.cbsegm(t)["C"] == 5)
    return [(15, 14, 8, RI.one_size_tbs(5)), (15, 14, 6, two5), (15, 15, 4, RI.one_size_tbs(7)),
            (15, 13, 2, RI.one_size_tbs(5))]


def test_multi_specs_cover():
    gam = []
    for cell, n, qm, tbs in _multi_specs():
        sg = oracle.cbsegm(tbs)
        nre = _nre(cell, n)
        gam.append(nre % sg["C"])
        kmin = min(sg["K1"], sg["K2"]) if sg["C2"] else sg["K1"]
        assert sg["F"] == 0 and qm * (nre // sg["C"]) + qm <= 3 * kmin + 12
    assert all(g > 0 for g in gam) and len(set(gam)) >= 3, gam
    assert sum(oracle.cbsegm(s[3])["C2"] > 0 for s in _multi_specs()) == 1


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_eq_rm_multi_block_gamma(kind):
    """TBs of 5 and 7 code blocks whose LLRs do not divide evenly (gamma != 0, the reference's `cb > C - gamma`), one
    with two code-block sizes, at rv 0..3 and then combined."""
    specs = _multi_specs()
    _run_jobs(kind, specs, list(range(len(specs))), 8, _eqrm_expected())


# ------------------------------------------------------------------ E within a size: the compact tables' keys

# 16-window sizes at which some whole-PRB E lies between a parity row's window-15 index and the smallest index of its
# other 15 windows (the row then holds exactly one LLR, in its last window), and the largest size
WITHIN_SIZES = (816, 848, 944, 976, 1008, 1568, 1696, 1952, 6144)


@functools.lru_cache(maxsize=None)
def within_specs(K: int):
    """Every (cell, PRBs, qm, tbs) of size K that pdsch_eq_rm takes: n = 1..nmax PRBs of both cells x the four Qm"""
    N = RI.N_of(K)
    return [(cell, n, qm, K - 24) for cell in (6, 15) for n in range(1, cell + 1) for qm in (2, 4, 6, 8)
            if (_nre(cell, n) + 1) * qm <= N]


def single_window_rows(K: int, rv: int, E: int, window: int = 15) -> int:
    """Parity rows of a fresh buffer whose only LLRs (index < E) sit in one given window"""
    inv = np.full(RI.buflen(K, 16), 0xffff, np.int64)
    inv[RI.table(K, rv)] = np.arange(RI.N_of(K))
    n = 0
    for s in (1, 2):
        rows = inv[s * (K + 32): s * (K + 32) + K].reshape(K // 16, 16)
        n += int(((rows[:, window] < E) & (np.delete(rows, window, axis=1).min(axis=1) >= E)).sum())
    return n


def test_within_size_cover():
    """34..84 allocations per size, 12..60 distinct E each, from under a twentieth of N up to N - Qm; the (K, rv, E) met
    include at least 30 in which a row's only LLRs sit in window 15 and 30 in which they sit in window 0."""
    last = first = 0
    for K in WITHIN_SIZES:
        sp = within_specs(K)
        Es = sorted({_nre(c, n) * q for c, n, q, _t in sp})
        assert 34 <= len(sp) <= 84 and 12 <= len(Es) <= 60, (K, len(sp), len(Es))
        assert Es[0] < RI.N_of(K) / 5 and Es[-1] > 0.85 * RI.N_of(K), (K, Es[0], Es[-1])
        for rv in RI.RVS:
            last += sum(single_window_rows(K, rv, E, 15) > 0 for E in Es)
            first += sum(single_window_rows(K, rv, E, 0) > 0 for E in Es)
    assert last >= 30 and first >= 30, (last, first)


@gpu
@pytest.mark.parametrize("rv", RI.RVS)
@pytest.mark.parametrize("K", WITHIN_SIZES)
def test_eq_rm_every_E_within_size(K, rv):
    """Two-layer jobs (compact image) at every whole-PRB E of size K, all at this rv, fresh and then combined: one
    compact table per (K, rv, E).  A table that misjudges a row fails its look-up and the call falls back to the
    two-kernel path, which the workgroup count of every decode call shows."""
    sp = within_specs(K)
    _run_jobs("two_layer", sp, [rv] * len(sp), 1, _eqrm_expected())


# ------------------------------------------------------------------ the other paths, in child processes

@gpu
@pytest.mark.parametrize("rv", RI.RVS)
@pytest.mark.parametrize("env", ["MI355_NO_EQRM=1", "MI355_EQRM_COMPACT=0"])
@pytest.mark.parametrize("kind", KINDS)
def test_same_jobs_in_child(kind, env, rv):
    """test_eq_rm_every_size[kind-rv] (and, with rv 0, the multi-block jobs) in a child process with MI355_NO_EQRM=1
    (pdsch_eq_llr + dlsch_rm_rx on real equaliser output) and with MI355_EQRM_COMPACT=0 (pdsch_eq_rm gathering
    through the inverse table; the switch is read once per process): the same comparison with the oracle must hold
    there.  Every size at every rv, one child per rv."""
    name, val = env.split("=")
    sel = f"test_eq_rm_every_size and {kind}-{rv}"
    if rv == 0:
        sel = f"({sel}) or (test_eq_rm_multi_block_gamma and {kind})"
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu",
                        os.path.join(HERE, "test_eq_rm_sweep_gpu.py"), "-k", sel],
                       env={**os.environ, name: val}, cwd=os.path.dirname(HERE), capture_output=True, text=True,
                       timeout=600)
    want = "\n2 passed" if rv == 0 else "\n1 passed"
    assert r.returncode == 0 and want in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-2000:])
