"""CPU: the PBCH restatement (tests/pbch_ref.py) on the real recording, and the product's PBCH host functions
(MIB pack / unpack, mi355_pbch_encode_host) against it.

Known answer: subframe 0 of tests/golden/signal_1.92M_amar.c64 (cell id 1) carries the MIB
000010101001000000000000 = 6 PRB, PHICH normal, Ng = 1, SFN 656, sent on one port in the first frame of its 40 ms
period (sfn_offset 0) -- the configuration tests/test_real_signal.py writes by hand."""
import os

import numpy as np
import pytest

import oracle
from oracle import ue_dl_chain as uc

import pbch_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
IQ = np.fromfile(os.path.join(HERE, "golden", "signal_1.92M_amar.c64"), np.complex64)
NPRB, CELL = 6, 1
SF_LEN = 15 * uc.symbol_sz(NPRB)
MIB_BITS = "000010101001000000000000"

_FRONT = {}


def _front(sf, nof_ports):
    """grid and estimates of one subframe of the recording (computed once per (sf, ports), never modified)"""
    if (sf, nof_ports) not in _FRONT:
        grid = uc.ofdm_rx_sf(IQ[sf * SF_LEN:(sf + 1) * SF_LEN], NPRB)[None, :]
        ce, res = uc.chest_estimate(grid, NPRB, nof_ports, CELL, sf)
        _FRONT[(sf, nof_ports)] = (grid[0], ce, res["noise_estimate"])
    return _FRONT[(sf, nof_ports)]


def _variants():
    return [False, True] if oracle.ref_available() else [False]


@pytest.mark.parametrize("nof_ports", [0, 1])
def test_real_signal_mib(nof_ports):
    """search-all on a 4-port estimate and 1 port configured: the known MIB from subframe 0, nothing from subframe 5;
    the restatement over liboracle's stages and over the reference's own agree bit for bit."""
    outs = []
    for use_ref in _variants():
        q = R.PbchRef(NPRB, CELL, nof_ports, use_ref=use_ref)
        grid, ce, noise = _front(0, 4 if nof_ports == 0 else 1)
        ret, nant, off, pay = q.decode(grid, ce, noise)
        assert (ret, nant, off) == (1, 1, 0)
        assert "".join(map(str, pay)) == MIB_BITS
        assert q.last_hit == (1, 0, 0, 0) and q.frame_idx == 0
        llr0 = q.last_llr[1].copy()
        grid, ce, noise = _front(5, 4 if nof_ports == 0 else 1)
        ret5 = q.decode(grid, ce, noise)
        assert ret5[0] == 0 and q.frame_idx == 1
        outs.append((pay, llr0, [q.decode_bits(0, d, 1) for d in range(4)]))
    for o in outs[1:]:
        assert np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1])
        assert all(np.array_equal(a, b) for a, b in zip(o[2], outs[0][2]))


def test_extraction_order_is_the_skip_rule():
    """the pointer arithmetic of srslte_pbch_cp (with its extra step for id % 3 == 2) visits, in order, the 72 central
    subcarriers of symbols 7..10 minus k % 3 == id % 3 in symbols 7 and 8"""
    for nof_prb in (6, 15, 25):
        for cid in (0, 1, 2, 503):
            want = [(7 + l) * 12 * nof_prb + nof_prb * 6 - 36 + k for l in range(4) for k in range(72)
                    if l >= 2 or k % 3 != cid % 3]
            assert R.pbch_re(nof_prb, cid).tolist() == want


def test_mib_pack_unpack():
    from srsran_amd import pbch as B
    from srsran_amd import pdsch as P
    for nof_prb in (6, 15, 25, 50, 75, 100):
        for plen in (0, 1):
            for ng in range(4):
                for sfn in (0, 4, 656, 1020):
                    cell = P.make_cell(nof_prb, 1, 0, phich_length=plen, phich_resources=ng)
                    bits = B.mib_pack(cell, sfn)
                    assert bits.size == 24 and int(bits[14:].sum()) == 0
                    c2, sfn2 = B.mib_unpack(bits)
                    assert (c2.nof_prb, c2.phich_length, c2.phich_resources, sfn2) == (nof_prb, plen, ng, sfn)
    # the SFN's two low bits are not in the MIB
    assert B.mib_unpack(B.mib_pack(P.make_cell(6), 659))[1] == 656
    cell, sfn = B.mib_unpack(R.bits_of(MIB_BITS))
    assert (cell.nof_prb, cell.phich_length, cell.phich_resources, sfn) == (6, 0, 2, 656)
    assert "".join(map(str, B.mib_pack(P.make_cell(6, 1, CELL, phich_resources=2), 656))) == MIB_BITS


@pytest.mark.parametrize("nof_ports", [1, 2, 4])
@pytest.mark.parametrize("nof_prb", [6, 15])
def test_host_encoder(nof_ports, nof_prb):
    """mi355_pbch_encode_host equals the restatement's encoder RE for RE (float equality: the same modulation and
    precoding formulas), touches nothing outside the PBCH, and the restatement decodes each frame on a first call to
    the payload with the right port count and sfn_offset == frame_idx."""
    from srsran_amd import pbch as B
    from srsran_amd import pdsch as P
    G = 14 * 12 * nof_prb
    rng = np.random.default_rng(7)
    for cid in (0, 1, 503):
        cell = P.make_cell(nof_prb, nof_ports, cid)
        payload = rng.integers(0, 2, 24).astype(np.uint8)
        payload[0] = 1
        re = R.pbch_re(nof_prb, cid)
        for fi in range(4):
            bg = (rng.standard_normal((nof_ports, G)) + 1j * rng.standard_normal((nof_ports, G))).astype(np.complex64)
            got, want = bg.copy(), bg.copy()
            B.pbch_encode_host(cell, payload, got, fi)
            R.pbch_encode(nof_prb, cid, nof_ports, payload, want, fi)
            assert np.array_equal(got.view(np.float32), want.view(np.float32))
            outside = np.ones(G, bool)
            outside[re] = False
            assert np.array_equal(got[:, outside], bg[:, outside])
            assert not np.array_equal(got[0, re], bg[0, re])
            # round trip over an ideal channel (h = 1 on every port: the ports' symbols add up at the receiver)
            q = R.PbchRef(nof_prb, cid, nof_ports)
            tx = np.zeros((nof_ports, G), np.complex64)
            B.pbch_encode_host(cell, payload, tx, fi)
            ret, nant, off, pay = q.decode(tx.sum(axis=0), np.ones((nof_ports, G), np.complex64), 0.0)
            assert (ret, nant, off) == (1, nof_ports, fi) and np.array_equal(pay, payload)
