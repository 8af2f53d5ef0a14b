"""Python mirror of include/srsran_amd/pbch.h -- the PBCH receiver (batched MIB acquisition, lib/src/phy/phch/pbch.c)
and its host functions: MIB packing and a PBCH encoder for synthesising test frames."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import check
from .pdsch import Cell
from .ue_dl import ChestRes, DlSfJob, _declare as _declare_ue_dl

BCH_PAYLOAD_LEN, PBCH_NOF_RE = 24, 240
INDEPENDENT, SEQUENCE = 0, 1


class PbchRes(C.Structure):
    _fields_ = [("ret", C.c_int32), ("nof_tx_ports", C.c_uint32), ("sfn_offset", C.c_int32),
                ("bch_payload", C.c_uint8 * BCH_PAYLOAD_LEN)]

    def bits(self) -> np.ndarray:
        return np.frombuffer(bytes(self.bch_payload), np.uint8).copy()


def _declare():
    L = _declare_ue_dl()
    if getattr(L, "_pbch_declared", False):
        return L
    vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int
    P = C.POINTER
    L.mi355_pbch_mib_unpack.restype = None
    L.mi355_pbch_mib_unpack.argtypes = [vp, P(Cell), P(u32)]
    L.mi355_pbch_mib_pack.restype = None
    L.mi355_pbch_mib_pack.argtypes = [P(Cell), u32, vp]
    L.mi355_pbch_encode_host.argtypes = [P(Cell), vp, P(vp), u32]
    L.mi355_pbch_create.argtypes = [P(vp), P(Cell), i32]
    L.mi355_pbch_destroy.restype = None
    L.mi355_pbch_destroy.argtypes = [vp]
    L.mi355_pbch_decode_reset.restype = None
    L.mi355_pbch_decode_reset.argtypes = [vp]
    L.mi355_pbch_decode_batch.argtypes = [vp, P(DlSfJob), P(ChestRes), u32, u32, P(PbchRes), vp]
    L.mi355_pbch_llr.argtypes = [vp, u32, u32, vp]
    L._pbch_declared = True
    return L


# ------------------------------------------------------------------ host functions

def mib_unpack(bits) -> tuple[Cell, int]:
    """srslte_pbch_mib_unpack: (cell with nof_prb / phich_length / phich_resources set, sfn) from 24 unpacked bits."""
    b = np.ascontiguousarray(bits, np.uint8)
    assert b.size == BCH_PAYLOAD_LEN
    cell, sfn = Cell(), C.c_uint32(0)
    _declare().mi355_pbch_mib_unpack(b.ctypes.data, C.byref(cell), C.byref(sfn))
    return cell, int(sfn.value)


def mib_pack(cell: Cell, sfn: int) -> np.ndarray:
    """srslte_pbch_mib_pack: the 24 unpacked MIB bits."""
    out = np.zeros(BCH_PAYLOAD_LEN, np.uint8)
    _declare().mi355_pbch_mib_pack(C.byref(cell), sfn, out.ctypes.data)
    return out


def pbch_encode_host(cell: Cell, bits, grids: np.ndarray, frame_idx: int) -> None:
    """srslte_pbch_encode into host tx grids (ports, 14 * 12 * nof_prb) complex64, in place."""
    assert grids.dtype == np.complex64 and grids.flags["C_CONTIGUOUS"] and grids.shape[0] >= cell.nof_ports
    b = np.ascontiguousarray(bits, np.uint8)
    assert b.size == BCH_PAYLOAD_LEN
    ptrs = (C.c_void_p * 4)(*[grids[p].ctypes.data for p in range(cell.nof_ports)] + [None] * (4 - cell.nof_ports))
    check(_declare().mi355_pbch_encode_host(C.byref(cell), b.ctypes.data, ptrs, frame_idx), "pbch_encode")


# ------------------------------------------------------------------ GPU batches

class Pbch:
    """srslte_pbch_t on one MI355X.  cell.nof_ports == 0 searches 1, 2 and 4 ports (the estimates cover 4)."""

    def __init__(self, cell: Cell, device: int = 0):
        self.L = _declare()
        h = C.c_void_p()
        check(self.L.mi355_pbch_create(C.byref(h), C.byref(cell), device), "pbch_create")
        self.h, self.cell, self.device = h, cell, device

    def decode(self, sfjobs: list[DlSfJob], chest, mode: int = INDEPENDENT, stream=None):
        """mi355_pbch_decode_batch: one PbchRes per job.  chest: ChestRes array (or list) of the jobs."""
        n = len(sfjobs)
        if not isinstance(chest, C.Array):
            chest = (ChestRes * n)(*chest)
        res = (PbchRes * n)()
        check(self.L.mi355_pbch_decode_batch(self.h, (DlSfJob * n)(*sfjobs), chest, n, mode, res, stream),
              "pbch_decode_batch")
        return res

    def reset(self):
        self.L.mi355_pbch_decode_reset(self.h)

    def llr(self, i: int, nant: int) -> np.ndarray:
        """The 480 LLRs of job i of the previous decode under port hypothesis nant (inspection)."""
        out = np.zeros(2 * PBCH_NOF_RE, np.float32)
        if self.L.mi355_pbch_llr(self.h, i, nant, out.ctypes.data) != out.size:
            raise RuntimeError("pbch_llr failed")
        return out

    def close(self):
        if getattr(self, "h", None):
            self.L.mi355_pbch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
