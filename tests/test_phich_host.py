"""CPU: the host functions of include/srsran_amd/phich.h -- PHICH group count and resource calculation, the PHICH
encoder through the restated decoder (tests/phich_ref.py), and DCI format 0 packing / unpacking."""
import itertools

import numpy as np
import pytest

from oracle import pdcch_chain as pd

import phich_ref as R

PRBS = [6, 15, 25, 50, 75, 100]


def _cell(nof_prb, nof_ports=1, cell_id=0, res=2, ext=0):
    from srsran_amd import pdsch as P
    return P.make_cell(nof_prb, nof_ports, cell_id, phich_length=ext, phich_resources=res)


@pytest.mark.parametrize("nof_prb", PRBS)
def test_ngroups_equals_the_reg_map(nof_prb):
    """mi355_phich_ngroups == the reference map's group count, Ng in {1/6, 1/2, 1, 2} x {normal, extended}."""
    from srsran_amd import phich as H
    for res, ext in itertools.product(range(4), range(2)):
        rg = R.regs(nof_prb, 2, 7, res, ext)
        assert H.ngroups(_cell(nof_prb, 2, 7, res, ext)) == rg.phich.shape[0] == R.ngroups_formula(nof_prb, res)


@pytest.mark.parametrize("nof_prb", PRBS)
def test_phich_calc(nof_prb):
    """mi355_phich_calc == phich.c:138-139 over every n_prb_lowest < nof_prb, n_dmrs < 8, I_phich in {0, 1}."""
    from srsran_amd import phich as H
    for res in range(4):
        cell = _cell(nof_prb, 1, 3, res)
        ng = R.ngroups_formula(nof_prb, res)
        for lo, dm, ip in itertools.product(range(nof_prb), range(8), range(2)):
            assert H.calc(cell, lo, dm, ip) == R.phich_calc(ng, lo, dm, ip)


def test_phich_calc_no_group():
    from srsran_amd import phich as H
    assert H.calc(_cell(0), 0, 0) is None
    assert H.ngroups(_cell(0)) == 0


@pytest.mark.parametrize("ext", [0, 1])
@pytest.mark.parametrize("nof_ports", [1, 2, 4])
def test_encode_loopback_all_sequences(nof_ports, ext):
    """Every (group, sequence) of a 15-PRB Ng = 2 cell (4 groups x 8) encoded into one grid with random ACKs, an
    identity channel: the restated decoder returns every ACK -- the eight sequences of a group are orthogonal -- with
    the closed-form distance 1 (a unit BPSK symbol correlates fully with its code word)."""
    from srsran_amd import phich as H
    nof_prb, cell_id, sf_idx = 15, 40 + nof_ports, 3 + ext
    cell = _cell(nof_prb, nof_ports, cell_id, 3, ext)
    rg = R.regs(nof_prb, nof_ports, cell_id, 3, ext)
    G = 14 * 12 * nof_prb
    rng = np.random.default_rng(nof_ports * 10 + ext)
    acks = rng.integers(0, 2, (rg.phich.shape[0], R.NSEQ))
    tx = np.zeros((nof_ports, G), np.complex64)
    for g in range(acks.shape[0]):
        for s in range(R.NSEQ):
            assert H.phich_encode_host(cell, sf_idx, g, s, int(acks[g, s]), tx) == 0
    # what a receive antenna sees through h = 1 from every port
    grids = tx.sum(axis=0, keepdims=True).astype(np.complex64)
    ce = np.ones((nof_ports, 1, G), np.complex64)
    for g in range(acks.shape[0]):
        for s in range(R.NSEQ):
            ack, dist = R.phich_decode(grids, ce, rg.phich[g], cell_id, sf_idx, s, 0.0)
            assert ack == acks[g, s], (g, s)
            # BPSK (+-(1 + j) / sqrt2) -> soft bit -+1 -> correlation 1 with its code word
            assert abs(dist - 1.0) < 1e-5, (g, s, dist)


def test_encode_refuses_bad_resources():
    from srsran_amd import phich as H
    cell = _cell(6, 1, 0, 0)  # one group
    tx = np.zeros((1, 14 * 72), np.complex64)
    assert H.phich_encode_host(cell, 0, 1, 0, 1, tx) == H.ERROR_INVALID_INPUTS
    assert H.phich_encode_host(cell, 0, 0, 8, 1, tx) == H.ERROR_INVALID_INPUTS
    assert not tx.any()


def test_encode_superposes():
    """Two PHICHs of one group add (srslte_regs_phich_add), they do not overwrite."""
    from srsran_amd import phich as H
    cell = _cell(6, 1, 5, 0)
    G = 14 * 72
    a, b, ab = (np.zeros((1, G), np.complex64) for _ in range(3))
    H.phich_encode_host(cell, 2, 0, 1, 1, a)
    H.phich_encode_host(cell, 2, 0, 6, 0, b)
    H.phich_encode_host(cell, 2, 0, 1, 1, ab)
    H.phich_encode_host(cell, 2, 0, 6, 0, ab)
    assert np.array_equal(ab, a + b) and np.count_nonzero(a) == 12


# ------------------------------------------------------------------ format 0

FLAGS = ["cif_enabled", "multiple_csi_request_enabled", "srs_request_enabled", "ra_format_enabled", "is_not_ue_ss"]


def _cfgs(flags):
    from srsran_amd import pdcch as D
    c = D.DciCfg()
    for f in flags:
        setattr(c, f, 1)
    o = pd.DciCfg(**{f: True for f in flags if f != "ra_format_enabled"})
    return c, o


@pytest.mark.parametrize("nof_prb", [6, 25, 50, 100])
def test_format0_round_trip(nof_prb):
    """pack -> unpack over random fields, every subset of the five configuration flags: the payload equals the Python
    restatement's bit for bit, its size is pdcch_chain.dci_sizeof(FORMAT0), the unpacked fields equal the
    restatement's and, where the reference's packer and unpacker agree on a field's place, what was packed."""
    from srsran_amd import pdcch as D
    from srsran_amd import phich as H
    rng = np.random.default_rng(nof_prb)
    cell = _cell(nof_prb, 2, 1)
    nriv = pd.riv_nbits(nof_prb)
    for k in range(len(FLAGS) + 1):
        for flags in itertools.combinations(FLAGS, k):
            c, o = _cfgs(flags)
            ue = "is_not_ue_ss" not in flags
            for _ in range(6):
                hop = int(rng.integers(-1, 2 if nof_prb < 50 else 4))
                nhop = 0 if hop < 0 else (1 if nof_prb < 50 else 2)
                f = dict(cif_present=int("cif_enabled" in flags), cif=int(rng.integers(0, 8)), freq_hop_fl=hop,
                         riv=int(rng.integers(0, 1 << (nriv - nhop))), mcs_idx=int(rng.integers(0, 32)),
                         ndi=int(rng.integers(0, 2)), tpc_pusch=int(rng.integers(0, 4)), n_dmrs=int(rng.integers(0, 8)),
                         cqi_request=int(rng.integers(0, 2)), srs_request=int(rng.integers(0, 2)),
                         srs_request_present=int(rng.integers(0, 2)))
                d = H.DciUl()
                d.rnti, d.format = 0x1234, D.FORMAT0
                d.location = D.DciLocation(1, 2)
                d.cif_present, d.cif, d.freq_hop_fl = f["cif_present"], f["cif"], hop
                d.type2_alloc.riv, d.tb.mcs_idx, d.tb.ndi = f["riv"], f["mcs_idx"], f["ndi"]
                d.tpc_pusch, d.n_dmrs, d.cqi_request = f["tpc_pusch"], f["n_dmrs"], f["cqi_request"]
                d.srs_request, d.srs_request_present = f["srs_request"], f["srs_request_present"]
                m = H.pack_pusch(cell, d, c)
                bits = D.msg_bits(m)
                want = R.format0_pack(f, nof_prb, 2, o)
                assert m.nof_bits == pd.dci_sizeof(pd.FORMAT0, nof_prb, 2, o) == D.dci_sizeof(cell, D.FORMAT0, c)
                assert np.array_equal(bits, want), (flags, f)
                assert (m.rnti, m.location.L, m.location.ncce) == (0x1234, 1, 2)
                u = H.unpack_pusch(cell, m, c)
                assert u is not None and u.format == D.FORMAT0 and u.rnti == 0x1234
                got = H.ul_fields(u)
                assert got == R.format0_unpack(want, nof_prb, o, "ra_format_enabled" in flags), (flags, f)
                for key in ("freq_hop_fl", "riv", "mcs_idx", "ndi", "tpc_pusch", "n_dmrs"):
                    assert got[key] == f[key], (flags, key)
                if "cif_enabled" in flags:
                    assert (got["cif_present"], got["cif"]) == (1, f["cif"])
                if "multiple_csi_request_enabled" in flags and ue:
                    assert (got["multiple_csi_request_present"], got["multiple_csi_request"]) == (1, 2 * f["cqi_request"])
                else:
                    assert got["cqi_request"] == f["cqi_request"]
                if "srs_request_enabled" in flags and ue:
                    assert got["srs_request"] == (f["srs_request"] & f["srs_request_present"])
                assert got["ra_type_present"] == int("ra_format_enabled" in flags)


@pytest.mark.parametrize("nof_prb", [6, 25, 50, 100])
def test_format0_refuses_1a(nof_prb):
    """A 1A payload (flag bit 1, behind the CIF when there is one) is refused as dci.c:510-513 does."""
    from srsran_amd import pdcch as D
    from srsran_amd import phich as H
    cell = _cell(nof_prb, 1, 0)
    for flags in ((), ("cif_enabled",)):
        c, o = _cfgs(flags)
        d1a = dict(format=pd.FORMAT1A, rnti=0x1234, mode=0, n_gap=0, riv=3, pid=1, n_prb1a=0,
                   tb=[dict(mcs_idx=5, rv=0, ndi=1, cw_idx=0)])
        bits = pd.dci_pack(d1a, nof_prb, 1, o)
        if flags:
            bits = np.concatenate([np.zeros(3, np.uint8), bits])[:bits.size]
        assert H.unpack_pusch(cell, D.dci_msg(bits, D.FORMAT0, 0x1234), c) is None
        assert R.format0_unpack(bits, nof_prb, o) is None
