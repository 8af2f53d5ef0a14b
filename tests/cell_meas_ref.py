"""float64 restatement of the reference's neighbour-cell measurement (lib/src/phy/sync/refsignal_dl_sync.c):
set_cell, find_peak, measure_sf, run and the stage-3 decision, plus a seeded capture synthesiser.  The GPU tests
(test_cell_meas_gpu.py) and the fixture script (golden/make_golden_cell_meas.py) compare against it.

Tolerances.  golden/make_golden_cell_meas.py compiles the reference (its FFT a double-precision stand-in) and prints, per
float field, the largest deviation of the compiled reference from this restatement relative to the field's scale, and
four times that.  TOL holds the 4 x figures of the recorded run; the 4 x margin is the project's standing allowance for a
GPU summation order that differs from the reference's AVX2 order.  dB fields and cfo are absolute (dB, Hz), linear
powers relative.  Nothing here was ever compared with the library to set a figure.

Decisions (found, peak_index, false_alarm, false_count, sf_count, and the stage-1 fields) are compared exactly.  safe()
tells whether every decision margin of a result lies outside its tolerance: best against second-best lag, peak against
4 rms_avg, the two half-frame comparisons, every stage-3 threshold.  The fixture script replaces a draw that is not
safe by the next seed; every case is synthetic, so none is excluded."""
from __future__ import annotations

import functools
import math

import numpy as np

import sync_ref as S

LIM = (6, 15, 25, 50, 75, 110)
SYMBOL_SZ = (128, 256, 384, 768, 1024, 1536)

# measured by golden/make_golden_cell_meas.py: 4 x the compiled reference's largest deviation from this restatement
TOL = {
    "rsrp_dBfs": 1.182e-5, "rssi_dBfs": 1.149e-5, "rsrq_dB": 1.983e-5, "cfo_Hz": 1.266e-4,  # absolute: dB, dB, dB, Hz
    "peak_value": 5.305e-7, "rms_avg": 7.504e-7,                                             # relative
    "rsrp": 8.225e-7, "rssi": 6.342e-7, "cfo": 3.845e-4,                                     # per subframe: rel, rel, Hz
    # relative to the larger of the value and the subframe's rsrp
    "sss_strength": 4.383e-7, "sss_strength_false": 1.329e-7, "rsrp_false": 7.830e-7,
    "sequence": 3.013e-7,                                                                    # relative to the sequence's peak
}
ABSOLUTE = ("rsrp_dBfs", "rssi_dBfs", "rsrq_dB", "cfo_Hz", "cfo")
RES_FLOAT = ("rsrp_dBfs", "rssi_dBfs", "rsrq_dB", "cfo_Hz", "peak_value", "rms_avg")
RES_INT = ("found", "peak_index", "stage1_peak", "stage1_found", "peak_shifted", "sf_count", "false_count",
           "false_alarm")
SF_FLOAT = ("rsrp", "rssi", "cfo", "sss_strength", "sss_strength_false", "rsrp_false")
NOT_FOUND = 0xFFFFFFFF


def symbol_sz(nof_prb: int) -> int:
    for lim, n in zip(LIM, SYMBOL_SZ):
        if nof_prb <= lim:
            return n
    raise ValueError(nof_prb)


def geometry(nof_prb: int):
    """(symbol size, cp0, cp1, sf_len): SRSLTE_CP_LEN_NORM rounds up, so at 25 PRB (384) the CPs are 30 and 27"""
    N = symbol_sz(nof_prb)
    return N, S.cp_len(N, 160), S.cp_len(N, 144), 15 * N


# ------------------------------------------------------------------ set_cell

def _lfsr(state: int, taps, length: int) -> np.ndarray:
    out = np.zeros(length, np.int64)
    for n in range(1600 + length):
        if n >= 1600:
            out[n - 1600] = state & 1
        f = 0
        for t in taps:
            f ^= state >> t
        state = (state >> 1) | ((f & 1) << 30)
    return out


@functools.lru_cache(maxsize=None)
def _gold_basis(length: int):
    """x1 and, per bit of c_init, x2 from that bit alone: x2 is linear in c_init over GF(2)"""
    return _lfsr(1, (3, 0), length), np.stack([_lfsr(1 << i, (3, 2, 1, 0), length) for i in range(31)])


def gold(c_init: int, length: int) -> np.ndarray:
    """36.211 7.2, Nc = 1600"""
    x1, basis = _gold_basis(length)
    bits = np.array([(c_init >> i) & 1 for i in range(31)], np.int64)
    return (x1 + bits @ basis) % 2


@functools.lru_cache(maxsize=4096)
def crs_symbol(cell_id: int, ns: int, l: int, nof_prb: int) -> np.ndarray:
    """the 2 nof_prb pilots of OFDM symbol l of slot ns (refsignal_dl.c:63-114), as the reference's float values"""
    c = gold(1024 * (7 * (ns + 1) + l + 1) * (2 * cell_id + 1) + 2 * cell_id + 1, 440)
    mp = np.arange(2 * nof_prb) + 110 - nof_prb
    k = np.float64(np.float32(math.sqrt(0.5)))
    return ((1 - 2 * c[2 * mp]) + 1j * (1 - 2 * c[2 * mp + 1])) * k


def _crs_v(port: int, l: int) -> int:
    if port < 2:
        return (0, 3)[l % 2] if port == 0 else (3, 0)[l % 2]
    return (0 if l == 0 else 3) if port == 2 else (3 if l == 0 else 0)


def crs_put(grid: np.ndarray, cell_id: int, nof_ports: int, sf: int, nof_prb: int) -> None:
    """srslte_refsignal_cs_put_sf for every port into one (14, nre) grid"""
    for p in range(nof_ports):
        for l in range(4 if p < 2 else 2):
            s = ((l // 2 + 1) * 7 - 3 if l % 2 else (l // 2) * 7) if p < 2 else 1 + l * 7
            f = (_crs_v(p, l) + cell_id % 6) % 6
            grid[s, f::6] = crs_symbol(cell_id, 2 * sf + s // 7, s % 7, nof_prb)


def ofdm_tx(grid: np.ndarray, nof_prb: int) -> np.ndarray:
    """srslte_ofdm_tx_sf without normalisation: the backward DFT's plain sum, CP from the symbol's tail"""
    N, cp0, cp1, L = geometry(nof_prb)
    nre = 12 * nof_prb
    out = np.zeros(L, np.complex128)
    pos = 0
    for s in range(14):
        X = np.zeros(N, np.complex128)
        X[N - nre // 2:] = grid[s, :nre // 2]
        X[1:nre // 2 + 1] = grid[s, nre // 2:]
        t = np.fft.ifft(X) * N
        cp = cp0 if s % 7 == 0 else cp1
        out[pos:pos + cp] = t[N - cp:]
        out[pos + cp:pos + cp + N] = t
        pos += cp + N
    return out


@functools.lru_cache(maxsize=64)
def set_cell(cell_id: int, nof_ports: int, nof_prb: int) -> np.ndarray:
    """srslte_refsignal_dl_sync_set_cell: (10, sf_len) complex128"""
    N, cp0, cp1, L = geometry(nof_prb)
    nre = 12 * nof_prb
    seq = np.zeros((10, L), np.complex128)
    scale = np.float64(np.float32(1.0) / np.float32(8 * nof_prb))
    for sf in range(10):
        g = np.zeros((14, nre), np.complex128)
        if sf % 5 == 0:
            S.put_sync(g, nof_prb, cell_id, sf)
        crs_put(g, cell_id, nof_ports, sf, nof_prb)
        seq[sf] = ofdm_tx(g, nof_prb) * scale
    seq.setflags(write=False)
    return seq


# ------------------------------------------------------------------ measure_sf, find_peak, run

def _rel(a: float, b: float) -> float:
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def crs_offsets(nof_prb: int):
    N, cp0, cp1, L = geometry(nof_prb)
    return [cp0 + (N + cp1) * s + (cp0 - cp1 if l >= 2 else 0) for l, s in enumerate((0, 4, 7, 11))]


def measure_sf(seq: np.ndarray, buf: np.ndarray, sf_idx: int, nof_prb: int):
    """srslte_refsignal_dl_sync_measure_sf: rsrp, rssi, cfo"""
    N, cp0, cp1, L = geometry(nof_prb)
    s = seq[sf_idx % 10]
    corr, rssi = [], 0.0
    for off in crs_offsets(nof_prb):
        corr.append(np.vdot(s[off:off + N], buf[off:off + N]))
        rssi += np.vdot(buf[off:off + N], buf[off:off + N]).real
    rsrp = sum(abs(c) ** 2 for c in corr) * 4
    rssi = nof_prb * rssi / 4 * np.float64(np.float32(7.41))
    d1 = (cp1 + N) * 4.0
    d2 = (cp1 + N) * 3.0 + (cp0 - cp1)

    def ang(a, b):
        return np.angle(corr[a] * np.conj(corr[b]))
    cfo = (ang(2, 0) + ang(3, 1)) / (2 * math.pi * 7.5) * 15000.0 * 0.25
    cfo += (ang(1, 0) + ang(3, 2)) / (2 * math.pi * d1) * (15000.0 * N) * np.float64(np.float32(0.3) / np.float32(2.0))
    cfo += ang(2, 1) / (2 * math.pi * d2) * (15000.0 * N) * np.float64(np.float32(0.2))
    return float(rsrp), float(rssi), float(cfo)


def sss_strength(seq: np.ndarray, buf: np.ndarray, sf_idx: int, nof_prb: int):
    """refsignal_dl_pss_sss_strength: sss_strength, sss_strength_false"""
    N, cp0, cp1, L = geometry(nof_prb)
    n = cp0 + cp1 * 5 + N * 5
    k = np.float64(np.float32(8 * nof_prb) / np.float32(62.0))
    a = np.vdot(seq[sf_idx % 10][n:n + N], buf[n:n + N])
    b = np.vdot(seq[(sf_idx + 5) % 10][n:n + N], buf[n:n + N])
    return float(k * abs(a) ** 2), float(k * abs(b) ** 2)


def find_peak(seq: np.ndarray, x: np.ndarray, nsamples: int, nof_prb: int) -> dict:
    """srslte_refsignal_dl_sync_find_peak; the correlation of block n at lag i < sf_len is
    sum_k x[n + i + k] conj(seq0[k]), k < sf_len (the 2 sf_len-point transform reads 2 sf_len samples: no lag is cut)"""
    L = seq.shape[1]
    F = np.conj(np.fft.fft(np.concatenate([seq[0], np.zeros(L)])))
    lim = min(nsamples - L, 10 * L)
    peak_value, peak_idx, rms_avg = 0.0, 0, 0.0
    mags = []
    for n in range(0, lim, L):
        c = np.fft.ifft(np.fft.fft(x[n:n + 2 * L]) * F)[:L]
        p = np.abs(c)
        mags.append(p)
        i = int(np.argmax(p))
        rms_avg += math.sqrt(float(np.mean(p ** 2)))
        if p[i] > peak_value:
            peak_value, peak_idx = float(p[i]), i + n
    rms_avg /= math.floor(lim / L)
    allp = np.sort(np.concatenate(mags))
    margin = dict(peak=_rel(allp[-1], allp[-2]), threshold=_rel(peak_value, 4 * rms_avg))
    found = peak_value > 4 * rms_avg
    r = dict(peak_value=peak_value, rms_avg=rms_avg, stage1_peak=peak_idx, stage1_found=int(found), peak_shifted=0,
             ret=peak_idx if found else -1, margin=margin)
    if r["ret"] > 0:
        buf = x[peak_idx:peak_idx + L]
        s, sf = sss_strength(seq, buf, 0, nof_prb)
        r0 = measure_sf(seq, buf, 0, nof_prb)[0]
        r5 = measure_sf(seq, buf, 5, nof_prb)[0]
        margin["half_sss"], margin["half_rsrp"] = _rel(s, sf), _rel(r0, r5)
        if sf > s and r5 > r0:
            r["ret"] += 5 * L
            r["peak_shifted"] = 1
    return r


def decide(sf: list, nof_prb: int, peak_idx: int) -> dict:
    """stage 3 (refsignal_dl_sync.c:430-511) over the per-subframe records (dicts)"""
    n = len(sf)
    rsrp = [s["rsrp"] for s in sf]
    cfo = [s["cfo"] for s in sf]
    sel = [s for s in sf if s["sf_idx"] % 5 == 0]
    div = 2.0 * n / 10
    rsrp_lin, rssi_lin, cfo_acc = sum(rsrp) / n, sum(s["rssi"] for s in sf) / n, sum(cfo) / n
    sss = sum(s["sss_strength"] for s in sel) / div
    sssf = sum(s["sss_strength_false"] for s in sel) / div
    rf = sum(s["rsrp_false"] for s in sel) / div

    def dbm(v):
        return 10 * math.log10(v) + 30 if v > 0 else -math.inf
    d_cfo = max(cfo) - min(cfo)
    d_rsrp = dbm(max(rsrp)) - dbm(min(rsrp))
    d_false = dbm(rsrp_lin) - dbm(rf)
    alarm, count = False, 0
    margin = {}
    for name, val, severe, mild, below in (("sss", sss, sssf * 1.5, sssf * 15.0, True),
                                           ("cfo", d_cfo, 2000.0, 1000.0, False),
                                           ("rsrp", d_rsrp, 10.0, 6.0, False),
                                           ("false", d_false, 3.0, 4.0, True)):
        if (val < severe) if below else (val > severe):
            alarm = True
        elif (val < mild) if below else (val > mild):
            count += 1
        margin[name] = (val, severe, mild)
    if count > 1:
        alarm = True
    r = dict(sf_count=n, false_count=count, false_alarm=int(alarm), found=int(not alarm), margin3=margin)
    if alarm:
        r.update(peak_index=NOT_FOUND, rsrp_dBfs=math.nan, rssi_dBfs=math.nan, rsrq_dB=math.nan, cfo_Hz=math.nan)
    else:
        r.update(peak_index=peak_idx, rsrp_dBfs=dbm(rsrp_lin), rssi_dBfs=dbm(rssi_lin), cfo_Hz=cfo_acc,
                 rsrq_dB=10 * math.log10(nof_prb) + dbm(rsrp_lin) - dbm(rssi_lin))
    return r


def run(seq: np.ndarray, x: np.ndarray, nsamples: int, nof_prb: int) -> dict:
    """srslte_refsignal_dl_sync_run: the result fields, the per-subframe records (sf) and the margins"""
    x = np.asarray(x, np.complex128)
    L = seq.shape[1]
    r = find_peak(seq, x, nsamples, nof_prb)
    r["sf"] = []
    if r["ret"] < 0:
        r.update(found=0, peak_index=NOT_FOUND, rsrp_dBfs=math.nan, rssi_dBfs=math.nan, rsrq_dB=math.nan,
                 cfo_Hz=math.nan, sf_count=0, false_count=0, false_alarm=0, margin3={})
        return r
    peak = r["ret"]
    sf_idx, n = (20 - peak // L) % 10, peak % L
    while n < nsamples - L + 1:
        buf = x[n:n + L]
        rsrp, rssi, cfo = measure_sf(seq, buf, sf_idx, nof_prb)
        rec = dict(sf_idx=sf_idx, rsrp=rsrp, rssi=rssi, cfo=cfo, sss_strength=0.0, sss_strength_false=0.0,
                   rsrp_false=0.0)
        if sf_idx % 5 == 0:
            rec["sss_strength"], rec["sss_strength_false"] = sss_strength(seq, buf, sf_idx, nof_prb)
            rec["rsrp_false"] = measure_sf(seq, buf, sf_idx + 1, nof_prb)[0]
        r["sf"].append(rec)
        sf_idx, n = (sf_idx + 1) % 10, n + L
    r.update(decide(r["sf"], nof_prb, peak))
    return r


def safe(r: dict) -> bool:
    """every decision margin of this result lies outside one tolerance"""
    m = r["margin"]
    if m["peak"] <= TOL["peak_value"] or m["threshold"] <= TOL["peak_value"] + TOL["rms_avg"]:
        return False
    if "half_sss" in m and (m["half_sss"] <= 2 * TOL["sss_strength"] or m["half_rsrp"] <= 2 * TOL["rsrp"]):
        return False
    for name, (val, severe, mild) in r.get("margin3", {}).items():
        for thr in (severe, mild):
            if name == "sss":
                if thr > 0 and _rel(val, thr) <= 2 * TOL["sss_strength"]:
                    return False
            else:
                tol = 2 * TOL["cfo"] if name == "cfo" else 2 * TOL["rsrp_dBfs"]
                if math.isfinite(val) and abs(val - thr) <= tol:
                    return False
    return True


def compare(got: dict, want: dict, what: str = "", sf_got=None, share: float = 1.0) -> None:
    """got: result fields (and per-subframe records) against a restatement result or the compiled reference's recorded
    one, within TOL.  share < 1 asks for that fraction of TOL: the recorded values against the restatement lie within
    the measured deviation itself, a quarter of TOL."""
    assert share <= 1.0
    for f in RES_INT:
        assert got[f] == want[f], (what, f, got[f], want[f])
    for f in RES_FLOAT:
        g, w = got[f], want[f]
        if isinstance(w, float) and math.isnan(w):
            assert math.isnan(g), (what, f, g)
            continue
        d = abs(g - w) / (1.0 if f in ABSOLUTE else abs(w))
        print(f"{what} {f}: got {g!r} want {w!r} deviation {d:.3g} tolerance {share * TOL[f]:.3g}")
        assert d <= share * TOL[f], (what, f, g, w, d)
    if sf_got is not None:
        assert len(sf_got) == len(want["sf"]), (what, len(sf_got), len(want["sf"]))
        for i, (g, w) in enumerate(zip(sf_got, want["sf"])):
            compare_sf(g, w, f"{what} sf {i}", share=share)


def compare_sf(g: dict, w: dict, what: str = "", fields=SF_FLOAT, share: float = 1.0) -> None:
    assert g["sf_idx"] % 10 == w["sf_idx"] % 10, (what, g["sf_idx"], w["sf_idx"])
    for f in fields:
        scale = 1.0 if f in ABSOLUTE else max(abs(w[f]), abs(w["rsrp"]) if f != "rssi" else 0.0)
        d = abs(g[f] - w[f]) / scale
        assert d <= share * TOL[f], (what, f, g[f], w[f], d, share * TOL[f])


# ------------------------------------------------------------------ synthetic captures

@functools.lru_cache(maxsize=32)
def _cell_frame(cell_id: int, nof_ports: int, nof_prb: int, seed: int) -> np.ndarray:
    """one 10 ms frame of a cell: random QPSK on every RE, PSS / SSS and the CRS of every port put over it"""
    rng = np.random.default_rng([seed, cell_id, nof_ports, nof_prb])
    nre = 12 * nof_prb
    out = []
    for sf in range(10):
        b = rng.integers(0, 2, (2, 14, nre)) * 2 - 1
        g = (b[0] + 1j * b[1]) / math.sqrt(2)
        if sf % 5 == 0:
            S.put_sync(g, nof_prb, cell_id, sf)
        crs_put(g, cell_id, nof_ports, sf, nof_prb)
        out.append(ofdm_tx(g, nof_prb) / (8 * nof_prb))
    f = np.concatenate(out)
    f.setflags(write=False)
    return f


def synth_capture(nof_prb: int, nsf: int, cells, cfo_hz: float = 0.0, snr_db: float = 20.0, seed: int = 0) -> np.ndarray:
    """nsf subframes of complex64: the sum of the cells' periodic 10 ms frames, each cell (cell_id, nof_ports, delay,
    amplitude) with its subframe 0 starting at sample `delay` (mod 10 sf_len) of the capture, rotated by a common CFO,
    plus white noise snr_db below the power of an amplitude-1 cell.  Regenerated bit for bit from its arguments."""
    N, cp0, cp1, L = geometry(nof_prb)
    t = np.arange(nsf * L)
    x = np.zeros(nsf * L, np.complex128)
    pw = None
    for cell_id, nof_ports, delay, amp in cells:
        f = _cell_frame(cell_id, nof_ports, nof_prb, seed)
        if pw is None:
            pw = float(np.mean(np.abs(f) ** 2))
        x += amp * f[(t - delay) % (10 * L)]
    if pw is None:
        pw = 1.0 / (8 * nof_prb) ** 2 * 12 * nof_prb
    x *= np.exp(2j * np.pi * cfo_hz * t / (15000.0 * N))
    rng = np.random.default_rng([seed, 77, nsf, nof_prb])
    sigma = math.sqrt(pw / 2 * 10 ** (-snr_db / 10))
    x += sigma * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))
    return x.astype(np.complex64)
