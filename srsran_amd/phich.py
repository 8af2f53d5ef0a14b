"""Python mirror of include/srsran_amd/phich.h -- PHICH decoding (lib/src/phy/phch/phich.c) and the UL grants (DCI
format 0, phch/dci.c) of the UE receiver, with the host functions: PHICH resource calculation, a PHICH encoder for
synthesising test subframes and format-0 packing / unpacking."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import check
from .pdcch import MAX_DCI_MSG, DciCfg, DciLocation, DciMsg, DciTb, UeDlCfg, _Type2, _declare as _declare_pdcch
from .pdsch import Cell, DlSfCfg
from .ue_dl import ChestRes, DlSfJob

PHICH_NBITS, NSEQUENCES, NSF, MAX_NSYMB = 3, 8, 4, 12
HOP_DISABLED = -1
ERROR_INVALID_INPUTS = -2


class PhichGrant(C.Structure):
    _fields_ = [("n_prb_lowest", C.c_uint32), ("n_dmrs", C.c_uint32), ("I_phich", C.c_uint32)]


class PhichResource(C.Structure):
    _fields_ = [("ngroup", C.c_uint32), ("nseq", C.c_uint32)]


class PhichRes(C.Structure):
    _fields_ = [("ret", C.c_int32), ("ack_value", C.c_uint32), ("distance", C.c_float)]


class PhichJob(C.Structure):
    _fields_ = [("sf", C.c_uint32), ("grant", PhichGrant)]


class DciUl(C.Structure):
    _fields_ = [("rnti", C.c_uint16), ("format", C.c_uint32), ("location", DciLocation), ("ue_cc_idx", C.c_uint32),
                ("type2_alloc", _Type2), ("freq_hop_fl", C.c_int32), ("tb", DciTb), ("n_dmrs", C.c_uint32),
                ("cqi_request", C.c_uint32), ("dai", C.c_uint32), ("ul_idx", C.c_uint32), ("is_tdd", C.c_uint32),
                ("tpc_pusch", C.c_uint8), ("cif", C.c_uint32), ("cif_present", C.c_uint32),
                ("multiple_csi_request", C.c_uint8), ("multiple_csi_request_present", C.c_uint32),
                ("srs_request", C.c_uint32), ("srs_request_present", C.c_uint32), ("ra_type", C.c_uint32),
                ("ra_type_present", C.c_uint32)]


# the fields dci_format0_unpack sets, for field-by-field comparisons
UL_FIELDS = ("cif", "cif_present", "freq_hop_fl", "riv", "mcs_idx", "ndi", "tpc_pusch", "n_dmrs", "cqi_request",
             "multiple_csi_request", "multiple_csi_request_present", "srs_request", "srs_request_present", "ra_type",
             "ra_type_present")


def ul_fields(d: DciUl) -> dict:
    out = {k: int(getattr(d, k)) for k in UL_FIELDS if k not in ("riv", "mcs_idx", "ndi")}
    out.update(riv=int(d.type2_alloc.riv), mcs_idx=int(d.tb.mcs_idx), ndi=int(d.tb.ndi))
    return out


def _declare():
    L = _declare_pdcch()
    if getattr(L, "_phich_declared", False):
        return L
    vp, u32, u16 = C.c_void_p, C.c_uint32, C.c_uint16
    P = C.POINTER
    L.mi355_phich_ngroups.restype = u32
    L.mi355_phich_ngroups.argtypes = [P(Cell)]
    L.mi355_phich_calc.argtypes = [P(Cell), P(PhichGrant), P(PhichResource)]
    L.mi355_phich_encode_host.argtypes = [P(Cell), P(DlSfCfg), PhichResource, C.c_uint8, P(vp)]
    L.mi355_dci_msg_unpack_pusch.argtypes = [P(Cell), P(DlSfCfg), P(DciCfg), P(DciMsg), P(DciUl)]
    L.mi355_dci_msg_pack_pusch.argtypes = [P(Cell), P(DlSfCfg), P(DciCfg), P(DciUl), P(DciMsg)]
    L.mi355_ue_dl_decode_phich_batch.argtypes = [vp, P(DlSfJob), P(DlSfCfg), P(ChestRes), u32, P(PhichJob), u32,
                                                 P(PhichRes), vp]
    L.mi355_ue_dl_find_ul_dci_batch.argtypes = [vp, P(DlSfCfg), P(UeDlCfg), P(u16), u32, P(C.c_int32), P(DciUl)]
    L._phich_declared = True
    return L


# ------------------------------------------------------------------ host functions

def ngroups(cell: Cell) -> int:
    return int(_declare().mi355_phich_ngroups(C.byref(cell)))


def calc(cell: Cell, n_prb_lowest: int, n_dmrs: int, I_phich: int = 0) -> tuple[int, int] | None:
    """srslte_phich_calc: (ngroup, nseq), None when the cell has no group."""
    g, r = PhichGrant(n_prb_lowest, n_dmrs, I_phich), PhichResource()
    if _declare().mi355_phich_calc(C.byref(cell), C.byref(g), C.byref(r)):
        return None
    return int(r.ngroup), int(r.nseq)


def phich_encode_host(cell: Cell, tti: int, ngroup: int, nseq: int, ack: int, grids: np.ndarray) -> int:
    """srslte_phich_encode, added into host tx grids (ports, 14 * 12 * nof_prb) complex64 in place; the return code."""
    assert grids.dtype == np.complex64 and grids.flags["C_CONTIGUOUS"] and grids.shape[0] >= cell.nof_ports
    ptrs = (C.c_void_p * 4)(*[grids[p].ctypes.data for p in range(cell.nof_ports)] + [None] * (4 - cell.nof_ports))
    sf = DlSfCfg(tti, 1)
    return int(_declare().mi355_phich_encode_host(C.byref(cell), C.byref(sf), PhichResource(ngroup, nseq), ack, ptrs))


def pack_pusch(cell: Cell, dci: DciUl, cfg: DciCfg | None = None) -> DciMsg:
    m, sf = DciMsg(), DlSfCfg(0, 1)
    check(_declare().mi355_dci_msg_pack_pusch(C.byref(cell), C.byref(sf), C.byref(cfg) if cfg else None,
                                              C.byref(dci), C.byref(m)), "dci_msg_pack_pusch")
    return m


def unpack_pusch(cell: Cell, msg: DciMsg, cfg: DciCfg | None = None) -> DciUl | None:
    d, sf = DciUl(), DlSfCfg(0, 1)
    rc = _declare().mi355_dci_msg_unpack_pusch(C.byref(cell), C.byref(sf), C.byref(cfg) if cfg else None,
                                                C.byref(msg), C.byref(d))
    return d if rc == 0 else None


# ------------------------------------------------------------------ GPU batches

def decode_phich(ue, sfjobs: list[DlSfJob], chest, jobs, stream=None, check_rc: bool = True):
    """mi355_ue_dl_decode_phich_batch on a UeDl: jobs are (sf, n_prb_lowest, n_dmrs, I_phich); the scrambling of
    subframe i is sfjobs[i].tti % 10.  Returns the PhichRes array."""
    L = _declare()
    nsf, n = len(sfjobs), len(jobs)
    if not isinstance(chest, C.Array):
        chest = (ChestRes * max(nsf, 1))(*chest)
    sfs = (DlSfCfg * max(nsf, 1))(*[DlSfCfg(j.tti, 0) for j in sfjobs])
    arr = (PhichJob * max(n, 1))(*[PhichJob(int(j[0]), PhichGrant(int(j[1]), int(j[2]), int(j[3]))) for j in jobs])
    res = (PhichRes * max(n, 1))()
    rc = L.mi355_ue_dl_decode_phich_batch(ue.h, (DlSfJob * max(nsf, 1))(*sfjobs), sfs, chest, nsf, arr, n, res, stream)
    if check_rc:
        check(rc, "decode_phich_batch")
    return res


def find_ul_dci(ue, ttis: list[int], rntis: list[int], cfgs: list[UeDlCfg]) -> list[list[DciUl]]:
    """mi355_ue_dl_find_ul_dci_batch for the jobs of the previous control-stage call on ue: per job the UL grants."""
    L = _declare()
    n = len(ttis)
    sfs = (DlSfCfg * n)(*[DlSfCfg(t, 0) for t in ttis])
    nof = (C.c_int32 * n)()
    dci = (DciUl * (n * MAX_DCI_MSG))()
    check(L.mi355_ue_dl_find_ul_dci_batch(ue.h, sfs, (UeDlCfg * n)(*cfgs), (C.c_uint16 * n)(*rntis), n, nof, dci),
          "find_ul_dci_batch")
    assert all(nof[i] >= 0 for i in range(n))
    return [[dci[i * MAX_DCI_MSG + k] for k in range(nof[i])] for i in range(n)]
