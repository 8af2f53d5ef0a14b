"""Python mirror of include/srsran_amd/csi.h -- the UE's channel-state feedback: batched PMI / RI selection
(lib/src/phy/mimo/precoding.c), condition number (utils/mat.c) and wideband CQI (phch/cqi.c) from channel estimates in
HBM, with the host functions: SNR -> CQI, the sub-band count and the decisions from the SINR lists."""
from __future__ import annotations

import ctypes as C

from . import check
from .ue_dl import ChestRes, DlSfJob, _declare as _declare_ue_dl

ERROR_INVALID_INPUTS = -2
PMI_PRECISION = 24
RI_CN_DB = 17.0


class CsiRes(C.Structure):
    _fields_ = [("sinr_1l", C.c_float * 4), ("sinr_2l", C.c_float * 2), ("cn", C.c_float), ("cn_count", C.c_uint32),
                ("pmi_1l", C.c_uint32), ("pmi_2l", C.c_uint32), ("ri", C.c_uint32), ("pmi", C.c_uint32),
                ("sinr_db", C.c_float), ("ri_cn", C.c_uint32), ("cqi", C.c_uint32)]


def _declare():
    L = _declare_ue_dl()
    if getattr(L, "_csi_declared", False):
        return L
    vp, u32, f32 = C.c_void_p, C.c_uint32, C.c_float
    P = C.POINTER
    L.mi355_cqi_from_snr.restype = u32
    L.mi355_cqi_from_snr.argtypes = [f32]
    L.mi355_cqi_hl_get_no_subbands.argtypes = [u32]
    L.mi355_csi_decide.restype = None
    L.mi355_csi_decide.argtypes = [f32, f32, P(CsiRes)]
    L.mi355_ue_dl_csi_batch.argtypes = [vp, P(DlSfJob), P(ChestRes), u32, f32, P(CsiRes), vp]
    L._csi_declared = True
    return L


# ------------------------------------------------------------------ host functions

def cqi_from_snr(snr_db: float) -> int:
    return int(_declare().mi355_cqi_from_snr(snr_db))


def cqi_hl_get_no_subbands(nof_prb: int) -> int:
    return int(_declare().mi355_cqi_hl_get_no_subbands(nof_prb))


def decide(sinr_1l, sinr_2l, cn: float, noise_estimate: float = 0.0, offset: float = 0.0, cn_count: int = 0) -> CsiRes:
    """mi355_csi_decide on the given SINR lists and condition number: the filled CsiRes."""
    r = CsiRes()
    r.sinr_1l[:] = [float(x) for x in sinr_1l]
    r.sinr_2l[:] = [float(x) for x in sinr_2l]
    r.cn, r.cn_count = cn, cn_count
    _declare().mi355_csi_decide(noise_estimate, offset, C.byref(r))
    return r


# ------------------------------------------------------------------ GPU batch

def csi_batch(ue, jobs, chest, offset: float = 0.0, stream=None, check_rc: bool = True):
    """mi355_ue_dl_csi_batch on a UeDl: jobs are the DlSfJob (list or ctypes array) whose ce[port][rx] hold the
    estimates, chest their ChestRes (noise_estimate).  Returns the CsiRes array (check_rc False: (rc, array))."""
    L = _declare()
    n = len(jobs)
    if not isinstance(jobs, C.Array):
        jobs = (DlSfJob * max(n, 1))(*jobs)
    if not isinstance(chest, C.Array):
        chest = (ChestRes * max(n, 1))(*chest)
    res = (CsiRes * max(n, 1))()
    rc = L.mi355_ue_dl_csi_batch(ue.h, jobs, chest, n, offset, res, stream)
    if not check_rc:
        return rc, res
    check(rc, "ue_dl_csi_batch")
    return res
