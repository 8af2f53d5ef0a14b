"""Float64 restatement of the cell-search stage (srslte_sync_find and the routines under it: sync/sync.c:452-850,
pss.c:34-63, 413-540, 594-640, find_sss.c, sss.c:128-157, gen_sss.c) -- test infrastructure, like pbch_ref.py.  One
SyncRef is one srslte_sync_t with one N_id_2; find() is one srslte_sync_find call and returns the fields of
mi355_sync_res_t plus the margins of its decisions (`margin`), which the tests use to leave out cases whose decision
lies inside the tolerance band.

Tolerances.  tests/golden/make_golden_sync.py measures, per float field, the largest deviation of the compiled
reference from this restatement relative to the field's scale (the value itself; 1 subcarrier for the CFO fields, 1 for
the CP metrics, 31^2 = 961 for the SSS correlations, whose sum of two is sss_corr), over the fixture's 236 calls (one
synthetic draw with a decision inside the tolerance band was replaced by the next seed, none is left).  The reference's
FFT is a double-precision DFT stand-in there, so its correlation outputs carry one rounding each.  The test tolerance
is 4 x the measurement:

    field          measured    4 x
    peak_value     2.746e-07   1.098e-06
    peak_abs       2.002e-07   8.007e-07
    cfo_pss        4.666e-08   1.866e-07
    cfo_pss_mean   4.921e-08   1.968e-07
    m0_value       3.909e-07   1.564e-06
    m1_value       2.675e-07   1.070e-06
    sss_corr       3.921e-07   1.569e-06
    M_norm_avg     8.595e-09   3.438e-08
    M_ext_avg      9.742e-09   3.897e-08"""
from __future__ import annotations

import numpy as np

FOUND, FOUND_NOSPACE, NOFOUND = 1, 2, 0
FULL, PARTIAL_3, DIFF = 0, 1, 2
CP_NORM, CP_EXT = 0, 1
FDD, TDD = 0, 1
N_ID_1_NONE = 1000

# field: (tolerance relative to max(|value|, scale), scale) -- the table above
TOL = {"peak_value": (1.098e-06, 0.0), "peak_abs": (8.007e-07, 0.0), "cfo_pss": (1.866e-07, 1.0),
       "cfo_pss_mean": (1.968e-07, 1.0), "m0_value": (1.564e-06, 961.0), "m1_value": (1.070e-06, 961.0),
       "sss_corr": (1.569e-06, 961.0), "M_norm_avg": (3.438e-08, 1.0), "M_ext_avg": (3.897e-08, 1.0)}
FLOAT_FIELDS = TOL
RTOL = TOL["peak_value"][0]               # the PSR against the threshold, the top two correlation values
ATOL_M = TOL["M_norm_avg"][0]             # M_norm_avg against M_ext_avg
ATOL_SSS = 961.0 * TOL["sss_corr"][0]     # the top two SSS correlations, FDD against TDD sss_corr
DECISION_FIELDS = ("ret", "peak_pos", "sss_available", "sss_detected", "m0", "m1", "n_id_1", "sf_idx", "cell_id", "cp",
                   "frame_type")
# a decision is inside the tolerance band when its margin is at most this many tolerances
MARGIN = 1.0


def cp_len(N: int, c: int) -> int:
    return int(np.ceil(np.float32(c) * np.float32(N) / np.float32(2048.0)))


def cp_sz(N: int, cp: int) -> int:
    return cp_len(N, 144 if cp == CP_NORM else 512)


def central_bins() -> np.ndarray:
    """DFT bins of the 62 central subcarriers under the reference's mirror / dc placement: -31 .. -1, 1 .. 31"""
    return np.concatenate([np.arange(-31, 0), np.arange(1, 32)])


# ------------------------------------------------------------------ sequences

def pss_generate(n_id_2: int) -> np.ndarray:
    """srslte_pss_generate with its float32 argument (so the values are the library's to the last bit but one)"""
    root = np.float32((25.0, 29.0, 34.0)[n_id_2])
    i = np.arange(62, dtype=np.float32)
    prod = np.where(i < 31, i.astype(np.float64) * (i.astype(np.float64) + 1.0),
                    (i.astype(np.float64) + 2.0) * (i.astype(np.float64) + 1.0))
    arg = (-1.0 * np.pi * float(root) * prod / 63.0).astype(np.float32)
    return np.cos(arg.astype(np.float64)) + 1j * np.sin(arg.astype(np.float64))


def m_sequences():
    def run(taps):
        x = [0] * 31
        x[4] = 1
        for i in range(26):
            x[i + 5] = sum(x[i + t] for t in taps) % 2
        return 1 - 2 * np.array(x)
    return run((2, 0)), run((3, 0)), run((4, 2, 1, 0))  # s~, c~, z~


def m0m1(n_id_1: int) -> tuple[int, int]:
    qp = n_id_1 // 30
    q = (n_id_1 + qp * (qp + 1) // 2) // 30
    mp = n_id_1 + q * (q + 1) // 2
    m0 = mp % 31
    return m0, (m0 + mp // 31 + 1) % 31


def sss_tables():
    s_t, c_t, z_t = m_sequences()
    i = np.arange(31)
    s = np.array([s_t[(i + m) % 31] for m in range(31)], np.float64)
    z1 = np.array([z_t[(i + m % 8) % 31] for m in range(31)], np.float64)
    sd = s[:, 1:] * s[:, :-1]
    c = np.array([[c_t[(i + id2) % 31], c_t[(i + id2 + 3) % 31]] for id2 in range(3)], np.float64)
    tab = np.zeros((30, 30), np.int64)
    for id1 in range(168):
        a, b = m0m1(id1)
        tab[a, b - 1] = id1
    return s, z1, sd, c, tab


def sss_generate(cell_id: int) -> tuple[np.ndarray, np.ndarray]:
    s, z1, _sd, c, _ = sss_tables()
    a, b = m0m1(cell_id // 3)
    c0, c1 = c[cell_id % 3]
    sf0, sf5 = np.zeros(62), np.zeros(62)
    sf0[0::2], sf0[1::2] = s[a] * c0, s[b] * c1 * z1[a]
    sf5[0::2], sf5[1::2] = s[b] * c0, s[a] * c1 * z1[b]
    return sf0, sf5


def put_sync(grid: np.ndarray, nof_prb: int, cell_id: int, sf_idx: int, cp: int = CP_NORM, frame_type: int = FDD):
    """PSS and SSS into one subframe's grid (2 nsymb, 12 nof_prb) in numpy: FDD as the put_slot functions do (slot 0,
    last and second last symbol); TDD with the SSS in the last symbol of slot 1 of subframe 0 / 5 and the PSS in the
    third symbol of the next subframe (36.211 6.11), for which grid is (2, 2 nsymb, nre): both subframes."""
    nsymb, nre = (7 if cp == CP_NORM else 6), 12 * nof_prb
    k = nre // 2 - 31
    pss = pss_generate(cell_id % 3)
    sss = sss_generate(cell_id)[0 if sf_idx == 0 else 1]

    def put(row, seq):
        row[k - 5:k] = 0
        row[k:k + 62] = seq
        row[k + 62:k + 67] = 0
    if frame_type == FDD:
        g = grid.reshape(2 * nsymb, nre)
        put(g[nsymb - 1], pss)
        put(g[nsymb - 2], sss)
    else:
        g = grid.reshape(2, 2 * nsymb, nre)
        put(g[0, 2 * nsymb - 1], sss)
        put(g[1, 2], pss)


# ------------------------------------------------------------------ the object

class SyncRef:
    def __init__(self, fft_size=128, max_offset=9600, n_id_2=0, threshold=2.0, ema_alpha=1.0, cfo_ema_alpha=0.1,
                 cfo_pss_enable=False, pss_filt_enable=False, sss_en=True, sss_alg=FULL, detect_cp=True, cp=CP_NORM,
                 detect_frame_type=True, frame_type=FDD, sss_corr_threshold=0.0):
        self.M, self.N, self.id2 = fft_size, max_offset, n_id_2
        self.threshold, self.ema_alpha, self.cfo_ema_alpha = threshold, float(np.float32(ema_alpha)), float(np.float32(cfo_ema_alpha))
        self.cfo_pss_enable, self.pss_filt, self.sss_en, self.sss_alg = cfo_pss_enable, pss_filt_enable, sss_en, sss_alg
        self.detect_cp, self.cp0, self.detect_ft, self.ft0 = detect_cp, cp, detect_frame_type, frame_type
        self.sss_thr = sss_corr_threshold
        M = self.M
        n = np.arange(M)
        self.bins = central_bins()
        self.E = np.exp(2j * np.pi * np.outer(n, self.bins) / M)  # [n, bin]: inverse DFT of the central bins
        t = self.E @ pss_generate(n_id_2) / np.sqrt(M)
        self.h = np.conj(t) / 62.0
        self.s, self.z1, self.sd, self.c, self.tab = sss_tables()
        self.reset()

    def reset(self):
        self.avg = np.zeros(self.N + self.M + 1)
        self.cfo_mean, self.cfo_set = 0.0, False
        self.Mn, self.Me = 0.0, 0.0
        self.cp = self.cp0

    # -------------------------------------------------------------- PSS
    def _correlate(self, x):
        M, N = self.M, self.N
        if N >= M:
            return np.convolve(x[:N], self.h)  # N + M - 1 outputs
        return np.array([np.dot(self.h, x[i:i + M]) for i in range(N)])

    def _psr(self, p, ln):
        a = self.avg
        ub = p + 1
        while a[ub + 1] <= a[ub] and ub < ln:
            ub += 1
        lb = 0
        if p > 2:
            lb = p - 1
            while a[lb - 1] <= a[lb] and lb > 1:
                lb -= 1
        dr = max(ln - 1 - ub, 0)
        right = a[ub:ub + dr].max() if dr > 0 else a[ub]
        left = a[:lb].max() if lb > 0 else a[0]
        side = right if right > left else left
        with np.errstate(all="ignore"):
            return a[p] / side

    def _filter(self, x):
        X = np.conj(self.E).T @ x
        return self.E @ X

    # -------------------------------------------------------------- SSS
    def _sss(self, sym):
        Y = np.conj(self.E).T @ sym
        y = [Y[0::2].copy(), Y[1::2].copy()]
        for i in range(2):
            pw = np.mean(np.abs(y[i]) ** 2)
            y[i] = y[i] / (np.sqrt(pw) if pw != 0 else 1.0) * self.c[self.id2][i]

        def corr(z):
            if self.sss_alg == DIFF:
                yp = z[1:] * np.conj(z[:-1])
                return np.abs(self.sd @ yp) ** 2
            parts = 3 if self.sss_alg == PARTIAL_3 else 1
            nm = 31 // parts
            return sum(np.abs(self.s[:, j * nm:(j + 1) * nm] @ z[j * nm:(j + 1) * nm]) ** 2 for j in range(parts))
        c0 = corr(y[0])
        m0 = int(np.argmax(c0))
        c1 = corr(y[1] * self.z1[m0])
        m1 = int(np.argmax(c1))
        gap = min(np.sort(c0)[-1] - np.sort(c0)[-2], np.sort(c1)[-1] - np.sort(c1)[-2])
        return m0, float(c0[m0]), m1, float(c1[m1]), float(gap)

    def _n_id_1(self, m0, m1, corr):
        if corr > self.sss_thr:
            if m1 > m0:
                if m0 < 30 and m1 - 1 < 30:
                    return int(self.tab[m0, m1 - 1])
            elif m1 < 30 and 0 <= m0 - 1 < 30:
                return int(self.tab[m1, m0 - 1])
        return None

    # -------------------------------------------------------------- one srslte_sync_find
    def find(self, inp, find_offset=0) -> dict:
        inp = np.asarray(inp, np.complex128)
        M, N = self.M, self.N
        x = inp[find_offset:]
        short = N < M
        conv = self._correlate(x)
        ln = len(conv)  # conv_output_len
        ab = np.abs(conv[:ln - 1]) ** 2
        if 0.0 < self.ema_alpha < 1.0:
            self.avg[:ln - 1] = ab * self.ema_alpha + self.avg[:ln - 1] * (1 - self.ema_alpha)
        else:
            self.avg[:ln - 1] = ab
        a = self.avg[:ln - 1]
        p = int(np.argmax(a)) if not np.isnan(a).any() else 0
        top2 = np.sort(a)[-2:]
        r = dict(ret=NOFOUND, n_id_2=self.id2, peak_pos=p + (M if short else 0), peak_value=0.0, peak_abs=float(a[p]),
                 cfo_pss=0.0, cfo_pss_mean=self.cfo_mean, sss_available=0, sss_detected=0, m0=0, m1=0, m0_value=0.0,
                 m1_value=0.0, sss_corr=0.0, n_id_1=N_ID_1_NONE, sf_idx=0, cell_id=-1, cp=self.cp, frame_type=self.ft0,
                 M_norm_avg=self.Mn, M_ext_avg=self.Me)
        # relative margins of this call's decisions (inf where a decision was not taken)
        mg = dict(threshold=np.inf, peak=float((top2[1] - top2[0]) / top2[1]) if top2[1] > 0 else 0.0, sss=np.inf,
                  cp=np.inf, frame_type=np.inf)
        if self.threshold > 0:
            r["peak_value"] = float(self._psr(p, ln))
            mg["threshold"] = abs(r["peak_value"] - self.threshold) / self.threshold
        r["margin"] = mg
        peak_pos = r["peak_pos"]
        if not (r["peak_value"] >= self.threshold or self.threshold == 0):
            return r
        if self.cfo_pss_enable and peak_pos >= M:
            sym = inp[find_offset + peak_pos - M:find_offset + peak_pos]
            if self.pss_filt:
                sym = self._filter(sym)
            y0, y1 = np.dot(self.h[:M // 2], sym[:M // 2]), np.dot(self.h[M // 2:], sym[M // 2:])
            r["cfo_pss"] = float(np.angle(np.conj(y0) * y1) / np.pi)
            if not self.cfo_set:
                self.cfo_mean, self.cfo_set = r["cfo_pss"], True
            elif 15000 * abs(r["cfo_pss"]) < 7000:
                self.cfo_mean = self.cfo_ema_alpha * r["cfo_pss"] + (1 - self.cfo_ema_alpha) * self.cfo_mean
            r["cfo_pss_mean"] = self.cfo_mean
        pp = peak_pos + find_offset
        if pp < 2 * (M + cp_len(M, 512)):
            r["ret"] = FOUND_NOSPACE
            return r
        r["ret"] = FOUND
        if self.sss_en:
            trials = [FDD, TDD] if self.detect_ft else [self.ft0]
            out, r["sss_available"], gaps = [], 1, []
            for ft in trials:
                idx = pp - (2 if ft == FDD else 4) * (M + cp_sz(M, self.cp)) + cp_sz(M, self.cp)
                if idx < 0:
                    r["sss_available"] = 0
                    out.append(None)
                    continue
                sym = inp[idx:idx + M]
                if self.cfo_pss_enable:
                    sym = sym * np.exp(2j * np.pi * (-self.cfo_mean / M) * np.arange(M))
                m0, v0, m1, v1, gap = self._sss(sym)
                r.update(m0=m0, m1=m1, m0_value=v0, m1_value=v1)
                gaps.append(gap)
                out.append(dict(corr=v0 + v1, sf=0 if m1 > m0 else 5, id=self._n_id_1(m0, m1, v0 + v1), gap=gap))
            det = [o is not None and o["id"] is not None for o in out]
            r["sss_detected"] = int(any(det))
            w, take = 0, True
            if self.detect_ft:
                cs = [o["corr"] if o else 0.0 for o in out]
                w = 0 if cs[0] > cs[1] else 1
                r["frame_type"] = FDD if w == 0 else TDD
                mg["frame_type"] = abs(cs[0] - cs[1])
            else:
                take = any(det)
            if take:
                o = out[w] or dict(corr=0.0, sf=0, id=None, gap=np.inf)
                r["sf_idx"] = o["sf"] + (1 if r["frame_type"] == TDD else 0)
                r["n_id_1"] = o["id"] if o["id"] is not None else N_ID_1_NONE
                r["sss_corr"] = o["corr"]
            if gaps:  # m0 / m1 of every trial that ran are decisions: the last one's are reported
                mg["sss"] = min(gaps)
            if r["n_id_1"] < 168:
                r["cell_id"] = 3 * r["n_id_1"] + self.id2
        if self.detect_cp:
            cpn, cpe = cp_len(M, 144), cp_len(M, 512)
            nsym = min(3, pp // (M + cpe))
            if nsym > 0:
                def metric(cpl):
                    R = C = 0.0
                    b = pp - nsym * (M + cpl)
                    for s in range(nsym):
                        u, v = inp[b + M:b + M + cpl], inp[b:b + cpl]
                        R += np.real(np.dot(u, np.conj(v)))
                        C += np.sum(np.abs(v) ** 2)
                        b += M + cpl
                    return R, (R / C if C > 0 else 0.0)
                Rn, mn = metric(cpn)
                Re, me = metric(cpe)
                self.Mn = 0.1 * (mn / nsym) + 0.9 * self.Mn
                self.Me = 0.1 * (me / nsym) + 0.9 * self.Me
                if self.Mn > self.Me:
                    self.cp = CP_NORM
                elif self.Mn < self.Me:
                    self.cp = CP_EXT
                else:
                    self.cp = CP_NORM if Rn > Re else CP_EXT
                mg["cp"] = abs(self.Mn - self.Me)
            else:
                self.cp = CP_NORM
            r.update(cp=self.cp, M_norm_avg=self.Mn, M_ext_avg=self.Me)
        return r


def safe(r: dict) -> bool:
    """no decision of this call lies inside the tolerance band"""
    m = r["margin"]
    return (m["threshold"] > MARGIN * RTOL and m["peak"] > MARGIN * RTOL and m["sss"] > MARGIN * ATOL_SSS and
            m["cp"] > MARGIN * ATOL_M and m["frame_type"] > MARGIN * ATOL_SSS)


def compare(got: dict, want: dict, what="") -> None:
    """decision fields exactly, float fields within FLOAT_FIELDS"""
    for f in DECISION_FIELDS:
        assert got[f] == want[f], (what, f, got[f], want[f])
    for f, (rt, at) in FLOAT_FIELDS.items():
        d = abs(got[f] - want[f])
        print(f"{what} {f}: got {got[f]!r} want {want[f]!r} |d| {d:.3g}")
        assert d <= rt * max(abs(want[f]), at), (what, f, got[f], want[f], d)


# ------------------------------------------------------------------ synthetic frames

def synth_frame(cell_id, sf_idx, cp=CP_NORM, frame_type=FDD, nof_prb=6, nsf=5, lead=0, cfo=0.0, snr_db=20.0, seed=0,
                tail=256, put=None):
    """`lead` noise samples, then nsf subframes starting with subframe sf_idx (0 or 5) of the cell: QPSK on every RE,
    PSS / SSS put over it, OFDM-modulated in numpy (oracle.ue_dl_chain.ofdm_tx_sf), rotated by `cfo` subcarriers, noise
    at snr_db below the signal power, `tail` more samples of noise.  complex64.  put(grid, sf_idx): another way to
    place the FDD signals into the first subframe's (2 nsymb * nre) complex64 grid, e.g. the library's."""
    from oracle import ue_dl_chain as uc
    rng = np.random.default_rng(seed)
    N = uc.symbol_sz(nof_prb)
    nsymb, nre = (7 if cp == CP_NORM else 6), 12 * nof_prb
    g = ((rng.integers(0, 2, (nsf, 2 * nsymb, nre)) * 2 - 1) + 1j * (rng.integers(0, 2, (nsf, 2 * nsymb, nre)) * 2 - 1)) / np.sqrt(2)
    if frame_type == FDD and put is not None:
        g0 = np.ascontiguousarray(g[0].reshape(1, -1), np.complex64)
        put(g0, sf_idx)
        g[0] = g0.reshape(2 * nsymb, nre)
    elif frame_type == FDD:
        put_sync(g[0], nof_prb, cell_id, sf_idx, cp, FDD)
    else:
        put_sync(g[0:2], nof_prb, cell_id, sf_idx, cp, TDD)
    sig = np.concatenate([uc.ofdm_tx_sf(g[i].astype(np.complex64), nof_prb, cp == CP_EXT).astype(np.complex128)
                          for i in range(nsf)])
    pw = np.mean(np.abs(sig) ** 2)
    x = np.concatenate([np.zeros(lead), sig, np.zeros(tail)]).astype(np.complex128)
    x = x * np.exp(2j * np.pi * cfo * np.arange(x.size) / N)
    sigma = np.sqrt(pw / 2 * 10 ** (-snr_db / 10))
    x = x + sigma * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))
    return x.astype(np.complex64)
