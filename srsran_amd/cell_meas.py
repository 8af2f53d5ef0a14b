"""Python mirror of include/srsran_amd/cell_meas.h -- neighbour-cell measurement (batched srslte_refsignal_dl_sync_*,
lib/src/phy/sync/refsignal_dl_sync.c): RSRP, RSRQ, RSSI, CFO and frame timing of cells named by their PCI."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import check
from .pdsch import Cell, make_cell
from .pdsch import _declare as _declare_pdsch

MAX_CELLS = 504
NOT_FOUND = 0xFFFFFFFF


class CellMeasCfg(C.Structure):
    _fields_ = [("nof_prb", C.c_uint32), ("max_nof_sf", C.c_uint32)]


class CellMeasJob(C.Structure):
    _fields_ = [("input", C.c_void_p), ("nsamples", C.c_uint32), ("cell", C.c_uint32)]


class CellMeasSf(C.Structure):
    _fields_ = [("sf_idx", C.c_uint32), ("rsrp", C.c_float), ("rssi", C.c_float), ("cfo", C.c_float),
                ("sss_strength", C.c_float), ("sss_strength_false", C.c_float), ("rsrp_false", C.c_float)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


class CellMeasRes(C.Structure):
    _fields_ = [("found", C.c_uint32), ("peak_index", C.c_uint32), ("rsrp_dBfs", C.c_float), ("rssi_dBfs", C.c_float),
                ("rsrq_dB", C.c_float), ("cfo_Hz", C.c_float), ("peak_value", C.c_float), ("rms_avg", C.c_float),
                ("stage1_peak", C.c_uint32), ("stage1_found", C.c_uint32), ("peak_shifted", C.c_uint32),
                ("sf_count", C.c_uint32), ("false_count", C.c_uint32), ("false_alarm", C.c_uint32)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


class CellMeasSfJob(C.Structure):
    _fields_ = [("input", C.c_void_p), ("cell", C.c_uint32), ("sf_idx", C.c_uint32)]


def _declare():
    L = _declare_pdsch()
    if getattr(L, "_cell_meas_declared", False):
        return L
    vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int
    P = C.POINTER
    L.mi355_cell_meas_create.argtypes = [P(vp), P(CellMeasCfg), i32]
    L.mi355_cell_meas_destroy.restype = None
    L.mi355_cell_meas_destroy.argtypes = [vp]
    L.mi355_cell_meas_sf_len.restype = u32
    L.mi355_cell_meas_sf_len.argtypes = [vp]
    L.mi355_cell_meas_set_cells.argtypes = [vp, P(Cell), u32]
    L.mi355_cell_meas_sequence.argtypes = [vp, u32, u32, vp]
    L.mi355_cell_meas_run_batch.argtypes = [vp, P(CellMeasJob), u32, P(CellMeasRes), P(CellMeasSf), vp]
    L.mi355_cell_meas_find_peak_batch.argtypes = [vp, P(CellMeasJob), u32, P(CellMeasRes), vp]
    L.mi355_cell_meas_measure_sf_batch.argtypes = [vp, P(CellMeasSfJob), u32, P(CellMeasSf), vp]
    L.mi355_cell_meas_decide.argtypes = [P(CellMeasSf), u32, u32, u32, P(CellMeasRes)]
    L.mi355_cell_meas_check_jobs.argtypes = [P(CellMeasJob), u32, u32, u32, u32]
    L._cell_meas_declared = True
    return L


def decide(sf, nof_prb: int, peak_idx: int) -> CellMeasRes:
    """mi355_cell_meas_decide (host only) over per-subframe records: CellMeasSf, or dicts / tuples of its fields."""
    recs = [s if isinstance(s, CellMeasSf) else (CellMeasSf(**s) if isinstance(s, dict) else CellMeasSf(*s)) for s in sf]
    n = len(recs)
    arr = (CellMeasSf * max(n, 1))(*recs)
    res = CellMeasRes()
    check(_declare().mi355_cell_meas_decide(arr, n, nof_prb, peak_idx, C.byref(res)), "cell_meas_decide")
    return res


def check_jobs(jobs, nof_prb: int, max_nof_sf: int, ncells: int) -> int:
    """mi355_cell_meas_check_jobs (host only) over (pointer, nsamples, cell index) triples: the return code"""
    n = len(jobs)
    arr = (CellMeasJob * max(n, 1))(*[CellMeasJob(p, ns, c) for p, ns, c in jobs])
    return _declare().mi355_cell_meas_check_jobs(arr, n, nof_prb, max_nof_sf, ncells)


class CellMeas:
    """mi355_cell_meas_t on one MI355X."""

    def __init__(self, nof_prb: int, max_nof_sf: int, device: int = 0):
        self.L = _declare()
        h = C.c_void_p()
        cfg = CellMeasCfg(nof_prb, max_nof_sf)
        check(self.L.mi355_cell_meas_create(C.byref(h), C.byref(cfg), device), "cell_meas_create")
        self.h, self.nof_prb, self.max_nof_sf = h, nof_prb, max_nof_sf
        self.sf_len = self.L.mi355_cell_meas_sf_len(h)

    def set_cells(self, cells) -> None:
        """cells: Cell structures, or (cell id, nof_ports) pairs at the object's bandwidth"""
        cs = [c if isinstance(c, Cell) else make_cell(self.nof_prb, c[1], c[0]) for c in cells]
        arr = (Cell * max(len(cs), 1))(*cs)
        check(self.L.mi355_cell_meas_set_cells(self.h, arr, len(cs)), "cell_meas_set_cells")

    def sequence(self, cell: int, sf_idx: int) -> np.ndarray:
        out = np.zeros(self.sf_len, np.complex64)
        check(self.L.mi355_cell_meas_sequence(self.h, cell, sf_idx, out.ctypes.data), "cell_meas_sequence")
        return out

    def _jobs(self, jobs):
        n = len(jobs)
        return n, (CellMeasJob * max(n, 1))(*[CellMeasJob(p, ns, c) for p, ns, c in jobs])

    def run(self, jobs, stream=None, with_sf: bool = True):
        """jobs: (device pointer, nsamples, cell index).  Returns (list of CellMeasRes, per job the list of its
        measured subframes' CellMeasSf, or None)."""
        n, arr = self._jobs(jobs)
        res = (CellMeasRes * max(n, 1))()
        sf = (CellMeasSf * max(n * self.max_nof_sf, 1))() if with_sf else None
        check(self.L.mi355_cell_meas_run_batch(self.h, arr, n, res, sf, stream), "cell_meas_run_batch")
        out = [res[i] for i in range(n)]
        if not with_sf:
            return out, None
        return out, [[sf[i * self.max_nof_sf + k] for k in range(res[i].sf_count)] for i in range(n)]

    def find_peak(self, jobs, stream=None):
        n, arr = self._jobs(jobs)
        res = (CellMeasRes * max(n, 1))()
        check(self.L.mi355_cell_meas_find_peak_batch(self.h, arr, n, res, stream), "cell_meas_find_peak_batch")
        return [res[i] for i in range(n)]

    def measure_sf(self, jobs, stream=None):
        """jobs: (device pointer, cell index, sf_idx)"""
        n = len(jobs)
        arr = (CellMeasSfJob * max(n, 1))(*[CellMeasSfJob(p, c, s) for p, c, s in jobs])
        out = (CellMeasSf * max(n, 1))()
        check(self.L.mi355_cell_meas_measure_sf_batch(self.h, arr, n, out, stream), "cell_meas_measure_sf_batch")
        return [out[i] for i in range(n)]

    def close(self):
        if getattr(self, "h", None):
            self.L.mi355_cell_meas_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
