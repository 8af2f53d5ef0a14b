"""Python mirror of include/srsran_amd/sync.h -- cell search (batched srslte_sync_find, lib/src/phy/sync/sync.c) and
its host functions: the PSS / SSS sequences, their put_slot functions and the cell-search vote."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import check
from .pdsch import _declare as _declare_pdsch

PSS_LEN, SSS_LEN = 62, 62
N_ID_2_ALL = 3
FOUND, FOUND_NOSPACE, NOFOUND = 1, 2, 0
SSS_FULL, SSS_PARTIAL_3, SSS_DIFF = 0, 1, 2
CP_NORM, CP_EXT = 0, 1
FDD, TDD = 0, 1
INDEPENDENT, SEQUENCE = 0, 1
CFO_I_ENABLE, CFO_CP_ENABLE, DECIMATE, KNOWN_N_ID_1, SSS_CHANNEL_EQUALIZE = 1, 2, 4, 8, 16


class SyncCfg(C.Structure):
    _fields_ = [("fft_size", C.c_uint32), ("max_offset", C.c_uint32), ("n_id_2", C.c_uint32),
                ("threshold", C.c_float), ("ema_alpha", C.c_float), ("cfo_ema_alpha", C.c_float),
                ("cfo_pss_enable", C.c_uint32), ("pss_filt_enable", C.c_uint32), ("sss_en", C.c_uint32),
                ("sss_alg", C.c_uint32), ("detect_cp", C.c_uint32), ("cp", C.c_uint32),
                ("detect_frame_type", C.c_uint32), ("frame_type", C.c_uint32), ("sss_corr_threshold", C.c_float),
                ("unsupported", C.c_uint32)]


class SyncJob(C.Structure):
    _fields_ = [("input", C.c_void_p), ("find_offset", C.c_uint32)]


class SyncRes(C.Structure):
    _fields_ = [("ret", C.c_int32), ("n_id_2", C.c_uint32), ("peak_pos", C.c_uint32), ("peak_value", C.c_float),
                ("peak_abs", C.c_float), ("cfo_pss", C.c_float), ("cfo_pss_mean", C.c_float),
                ("sss_available", C.c_uint32), ("sss_detected", C.c_uint32), ("m0", C.c_uint32), ("m1", C.c_uint32),
                ("m0_value", C.c_float), ("m1_value", C.c_float), ("sss_corr", C.c_float), ("n_id_1", C.c_uint32),
                ("sf_idx", C.c_uint32), ("cell_id", C.c_int32), ("cp", C.c_uint32), ("frame_type", C.c_uint32),
                ("M_norm_avg", C.c_float), ("M_ext_avg", C.c_float)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


class CellSearchRes(C.Structure):
    _fields_ = [("cell_id", C.c_uint32), ("cp", C.c_uint32), ("frame_type", C.c_uint32), ("peak", C.c_float),
                ("mode", C.c_float), ("psr", C.c_float), ("cfo", C.c_float)]


def sync_cfg(fft_size: int = 128, max_offset: int = 9600, n_id_2: int = N_ID_2_ALL, threshold: float = 2.0,
             ema_alpha: float = 1.0, cfo_ema_alpha: float = 0.1, cfo_pss_enable: bool = False,
             pss_filt_enable: bool = False, sss_en: bool = True, sss_alg: int = SSS_FULL, detect_cp: bool = True,
             cp: int = CP_NORM, detect_frame_type: bool = True, frame_type: int = FDD,
             sss_corr_threshold: float = 0.0, unsupported: int = 0) -> SyncCfg:
    """srslte_sync_init's defaults (detect_cp, sss_en, detect_frame_type on, SSS_FULL, cfo_ema_alpha 0.1); ema_alpha 1
    switches the correlation average off."""
    return SyncCfg(fft_size, max_offset, n_id_2, threshold, ema_alpha, cfo_ema_alpha, int(cfo_pss_enable),
                   int(pss_filt_enable), int(sss_en), sss_alg, int(detect_cp), cp, int(detect_frame_type), frame_type,
                   sss_corr_threshold, unsupported)


def _declare():
    L = _declare_pdsch()
    if getattr(L, "_sync_declared", False):
        return L
    vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int
    P = C.POINTER
    L.mi355_pss_generate.argtypes = [u32, vp]
    L.mi355_sss_generate.argtypes = [u32, vp, vp]
    L.mi355_pss_put_slot.restype = None
    L.mi355_pss_put_slot.argtypes = [vp, vp, u32, u32]
    L.mi355_sss_put_slot.restype = None
    L.mi355_sss_put_slot.argtypes = [vp, vp, u32, u32]
    L.mi355_cellsearch_pick.argtypes = [P(SyncRes), u32, P(CellSearchRes)]
    L.mi355_sync_create.argtypes = [P(vp), P(SyncCfg), i32]
    L.mi355_sync_destroy.restype = None
    L.mi355_sync_destroy.argtypes = [vp]
    L.mi355_sync_reset.argtypes = [vp]
    L.mi355_sync_find_batch.argtypes = [vp, P(SyncJob), u32, u32, P(SyncRes), vp]
    L._sync_declared = True
    return L


# ------------------------------------------------------------------ host functions

def pss_generate(n_id_2: int) -> np.ndarray:
    """srslte_pss_generate: 62 complex64 values."""
    out = np.zeros(PSS_LEN, np.complex64)
    check(_declare().mi355_pss_generate(n_id_2, out.ctypes.data), "pss_generate")
    return out


def sss_generate(cell_id: int) -> tuple[np.ndarray, np.ndarray]:
    """srslte_sss_generate: the 62 float32 values of subframe 0 and of subframe 5."""
    s0, s5 = np.zeros(SSS_LEN, np.float32), np.zeros(SSS_LEN, np.float32)
    check(_declare().mi355_sss_generate(cell_id, s0.ctypes.data, s5.ctypes.data), "sss_generate")
    return s0, s5


def _slot(slot: np.ndarray, nof_prb: int, cp: int) -> None:
    assert slot.dtype == np.complex64 and slot.flags["C_CONTIGUOUS"] and slot.size == (7 if cp == CP_NORM else 6) * 12 * nof_prb


def pss_put_slot(pss: np.ndarray, slot: np.ndarray, nof_prb: int, cp: int = CP_NORM) -> None:
    """srslte_pss_put_slot into one slot of a host grid (nsymb * 12 * nof_prb complex64), in place."""
    _slot(slot, nof_prb, cp)
    p = np.ascontiguousarray(pss, np.complex64)
    assert p.size == PSS_LEN
    _declare().mi355_pss_put_slot(p.ctypes.data, slot.ctypes.data, nof_prb, cp)


def sss_put_slot(sss: np.ndarray, slot: np.ndarray, nof_prb: int, cp: int = CP_NORM) -> None:
    """srslte_sss_put_slot into one slot of a host grid, in place."""
    _slot(slot, nof_prb, cp)
    s = np.ascontiguousarray(sss, np.float32)
    assert s.size == SSS_LEN
    _declare().mi355_sss_put_slot(s.ctypes.data, slot.ctypes.data, nof_prb, cp)


def cellsearch_pick(found) -> CellSearchRes:
    """get_cell's vote over the candidates (SyncRes)."""
    n = len(found)
    arr = (SyncRes * n)(*found)
    out = CellSearchRes()
    check(_declare().mi355_cellsearch_pick(arr, n, C.byref(out)), "cellsearch_pick")
    return out


# ------------------------------------------------------------------ GPU batches

class Sync:
    """srslte_sync_t (three of them for n_id_2 = N_ID_2_ALL) on one MI355X."""

    def __init__(self, cfg: SyncCfg, device: int = 0):
        self.L = _declare()
        h = C.c_void_p()
        check(self.L.mi355_sync_create(C.byref(h), C.byref(cfg), device), "sync_create")
        self.h, self.cfg, self.device = h, cfg, device
        self.nhyp = 3 if cfg.n_id_2 == N_ID_2_ALL else 1

    def find(self, inputs, find_offsets=0, mode: int = INDEPENDENT, stream=None) -> list[list[SyncRes]]:
        """mi355_sync_find_batch over device pointers: per job the list of its hypotheses' SyncRes."""
        n = len(inputs)
        if isinstance(find_offsets, int):
            find_offsets = [find_offsets] * n
        jobs = (SyncJob * max(n, 1))(*[SyncJob(p, o) for p, o in zip(inputs, find_offsets)])
        res = (SyncRes * max(n * self.nhyp, 1))()
        check(self.L.mi355_sync_find_batch(self.h, jobs, n, mode, res, stream), "sync_find_batch")
        return [[res[i * self.nhyp + h] for h in range(self.nhyp)] for i in range(n)]

    def reset(self):
        check(self.L.mi355_sync_reset(self.h), "sync_reset")

    def close(self):
        if getattr(self, "h", None):
            self.L.mi355_sync_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cell_search(iq_frames, fft_size: int = 128, frame_len: int | None = None, device: int = 0, stream=None):
    """srsUE's cell search over successive 5 ms frames resident in HBM (device pointers, each frame_len + fft_size
    samples readable): the three N_id_2 hypotheses in SEQUENCE mode with srslte_ue_sync_init's search settings
    (ue_sync.c:282-285, 382-393: threshold 2.0, correlation average off, cfo_ema_alpha 0.1, PSS-based CFO, SSS_FULL,
    CP and frame-type detection) minus the CP-based CFO stage; the FOUND results with a valid cell id of each hypothesis
    go to the vote.  Returns (per hypothesis CellSearchRes or None, the per-frame results)."""
    frame_len = frame_len or 75 * fft_size  # 5 subframes of 15 fft_size
    q = Sync(sync_cfg(fft_size=fft_size, max_offset=frame_len, n_id_2=N_ID_2_ALL, threshold=2.0, ema_alpha=1.0,
                      cfo_ema_alpha=0.1, cfo_pss_enable=True), device)
    try:
        res = q.find(list(iq_frames), 0, SEQUENCE, stream)
    finally:
        q.close()
    cells = []
    for h in range(3):
        cand = [r[h] for r in res if r[h].ret == FOUND and r[h].cell_id >= 0]
        cells.append(cellsearch_pick(cand) if cand else None)
    return cells, res
