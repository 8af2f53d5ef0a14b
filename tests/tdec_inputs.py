"""TEST INFRASTRUCTURE ONLY: inputs for the turbo decoders at every one of the 188 code-block sizes of 36.212 table
5.1.3-3, shared by tests/test_tdec_sweep_gpu.py (the 16-bit window / generic kernels against the oracle),
tests/test_tdec_sweep_oracle.py (the oracle against the reference's own decoders), tests/test_dlsch_gpu.py (the DL-SCH
at every size on the latency and the throughput path) and tests/test_tdec8_gpu.py (the 8-bit decoder against digests
recorded from the reference, tests/golden/tdec8_sweep.npz).

16-bit: every (K, class of CLASSES) is one block, deterministic, seeded from K: encoder-order LLRs ("lin", 3K + 12
int16, the generic decoder's layout) and the AUTO decoder's buffer of them ("buf", oracle.tdec_pack_input).
8-bit: every (K, class of CLASSES8) from an integer generator written out below (no numpy.random), packed as
tests/golden/make_golden.py pack8 does."""
from __future__ import annotations

import functools
import hashlib

import numpy as np

import oracle

# 36.212 table 5.1.3-3
CB_SIZES = tuple(list(range(40, 512, 8)) + list(range(512, 1024, 16)) + list(range(1024, 2048, 32)) +
                 list(range(2048, 6145, 64)))
NHALF = 8
SEED = 3
TDEC_SEG = 8          # tdec_internal.h:11
TDEC_GEN_CB_L = 12    # tdec_internal.h:87
LAT_RING = 2          # tdec_win_lat.hip:190
SB_STRIDE = 18600     # dlsch_internal.h:6: int16 per softbuffer slot, the input stride of every DL-SCH decode

# (Eb/N0 in oracle.make_cb's convention, scale) of the codeword classes; the others are built in block()
EBNO_A, EBNO_B, EBNO_C = 3.0, 4.5, 6.0
CLASSES = ("a_fail", "b_slow", "c_fast", "d_sat", "e_rand", "f_zero", "g_seven")
NBLOCKS = 19  # per K in the GPU sweep: CLASSES repeated


def nsb(K: int) -> int:
    """mi355_tdec_autoimp_get_subblocks (tdec_runtime.cpp:149-154)"""
    if K % 16 == 0 and K > 800:
        return 16
    if K % 8 == 0 and K > 400:
        return 8
    return 0


WINDOW_SIZES = tuple(K for K in CB_SIZES if nsb(K))
SMALL_SIZES = tuple(K for K in CB_SIZES if not nsb(K))


@functools.lru_cache(maxsize=None)
def block(K: int, cls: str):
    """(sent bits or None, lin, buf) of one class; read-only arrays (shared between tests)"""
    rng = np.random.default_rng([SEED, K, CLASSES.index(cls)])
    bits = None
    if cls in ("a_fail", "b_slow", "c_fast", "d_sat"):
        eb = {"a_fail": EBNO_A, "b_slow": EBNO_B, "c_fast": EBNO_C, "d_sat": EBNO_C}[cls]
        bits, lin, _ = oracle.make_cb(rng, K, eb, scale=900.0 if cls == "d_sat" else 100.0)
    elif cls == "e_rand":
        lin = rng.integers(-32768, 32768, 3 * K + 12, dtype=np.int16)
    else:
        lin = np.full(3 * K + 12, 0 if cls == "f_zero" else 7, np.int16)
    buf = oracle.tdec_pack_input(lin, K)
    for v in (bits, lin, buf):
        if v is not None:
            v.setflags(write=False)
    return bits, lin, buf


def decision_bytes(bits) -> np.ndarray:
    return np.packbits(np.asarray(bits, np.uint8))


@functools.lru_cache(maxsize=None)
def window_traces(K: int):
    """{class: (NHALF, K/8) decision bytes of the oracle's AUTO decoder after each half-iteration}"""
    out = {}
    for c in CLASSES:
        tr = oracle.tdec_run(block(K, c)[2], K, NHALF, trace=True)[1]
        tr.setflags(write=False)
        out[c] = tr
    return out


@functools.lru_cache(maxsize=None)
def generic_traces(K: int):
    """The same of the oracle's generic decoder on the linear layout"""
    out = {}
    for c in CLASSES:
        tr = oracle.tdec_run_generic(block(K, c)[1], K, NHALF, trace=True)[1]
        tr.setflags(write=False)
        out[c] = tr
    return out


def first_correct(trace, bits) -> int:
    """The first half-iteration (1-based) whose decisions equal the sent bits; NHALF + 1 if none does"""
    want = decision_bytes(bits)
    for h in range(trace.shape[0]):
        if np.array_equal(trace[h], want):
            return h + 1
    return trace.shape[0] + 1


def lat_lds(K: int, n: int) -> int:
    """tdec_lat_lds (tdec_win_lat.hip:259-263)"""
    L, NL = K // n, n // 2
    return K // 2 * 4 * 4 + L * NL * 8 * 4 + 2 * LAT_RING * 64 * 8 * 4 + 256 * 4 + (K + 31) // 32 * 4


def features(K: int) -> dict:
    """Every choice the kernels make from K alone.  Window decoder entries are None for the generic sizes."""
    n = nsb(K)
    f = {"nsb": n,
         "gen_seg_rem": K % TDEC_SEG,                          # tdec_runtime.cpp:58-59 (Kp, nseg of the pair kernel)
         "gen_cb_chunks": -(-K // TDEC_GEN_CB_L),              # tdec_gen_cb.hip:386: one lane per chunk of 12 steps
         "gen_cb_waves": (-(-K // TDEC_GEN_CB_L) + 63) // 64,  # tdec_gen_cb.hip:386: workgroup size / 64
         "gen_cb_full": K % TDEC_GEN_CB_L == 0}                # tdec_gen_cb.hip:392: no short last chunk
    win = dict.fromkeys(("seg_rem", "full", "fuse_capable", "spec_ok", "tx_capable", "decide_rows", "lat_odd",
                         "lat_bytes1", "lat_tail_fwd", "lat_tail_bwd", "lat_fits"))
    if n:
        L = K // n
        PB = 64 // (n // 2)                                    # tdec_win_lat.hip:271
        H = L // 2                                             # tdec_win_lat.hip:279
        win = {"seg_rem": (n, L % TDEC_SEG),                   # tdec_runtime.cpp:52-54: the last beta segment's rows
               "full": (n, L % TDEC_SEG == 0),                 # tdec_kernels.hip:1084-1092
               # tdec_runtime.cpp:277 (without the caller's out_stride / pointer alignment)
               "fuse_capable": (n, L % 8 == 0 or (K % 64 == 0 and (K // 8) % (n // 2) == 0)),
               "spec_ok": n == 16 and L % TDEC_SEG == 0,       # tdec_kernels.hip:1065
               "tx_capable": n == 16 and L % TDEC_SEG == 0,    # tdec_kernels.hip:1038 (then by alignment, :1039)
               "decide_rows": (n, L % 8 == 0),                 # tdec_kernels.hip:1099
               "lat_odd": (n, L % 2),                          # uneven split H | L - H
               "lat_bytes1": n == 16 and L % 16 == 0,          # tdec_win_lat.hip:393
               "lat_tail_fwd": (n, (L - H) % PB),              # tdec_win_lat.hip:646: min(PB, L - k0) of the last chunk
               "lat_tail_bwd": (n, H % PB),                    # tdec_win_lat.hip:658: min(PB, k0)
               "lat_fits": lat_lds(K, n) <= 160 * 1024 - 64}   # tdec_win_lat.hip:765, dlsch_runtime.cpp launch_latency
    f.update(win)
    return f


# every value each feature takes over the 188 sizes (tests/test_tdec_sweep_gpu.py::test_sweep_covers_every_path)
FEATURE_VALUES = {
    "nsb": {0, 8, 16},
    "gen_seg_rem": {0},
    "gen_cb_chunks": {-(-K // 12) for K in CB_SIZES},
    "gen_cb_waves": {1, 2, 3, 4, 5, 6, 7, 8},
    "gen_cb_full": {False, True},
    "seg_rem": {None} | {(8, r) for r in range(8)} | {(16, r) for r in range(8)},
    "full": {None, (8, False), (8, True), (16, False), (16, True)},
    "fuse_capable": {None, (8, False), (8, True), (16, False), (16, True)},
    "spec_ok": {None, False, True},
    "tx_capable": {None, False, True},
    "decide_rows": {None, (8, False), (8, True), (16, False), (16, True)},
    "lat_odd": {None, (8, 0), (8, 1), (16, 0), (16, 1)},
    "lat_bytes1": {None, False, True},
    "lat_tail_fwd": {None} | {(8, r) for r in range(16)} | {(16, r) for r in range(8)},
    "lat_tail_bwd": {None} | {(8, r) for r in range(16)} | {(16, r) for r in range(8)},
    "lat_fits": {None, True},
}


# ------------------------------------------------------------------ 8-bit decoder

CLASSES8 = ("rand", "waterfall", "high")
# (codeword amplitude, noise multiplier): the noise is ((sum of 4 bytes) - 510) * mult >> 6, standard deviation
# 147.8 * mult / 64
LEVELS8 = {"waterfall": (16, 7), "high": (16, 3)}
_M64 = (1 << 64) - 1


def nsb8(K: int) -> int:
    """tdec_subblocks_8bit: 32 windows for K % 32 == 0 and K > 2048, 16 for K % 16 == 0 and K > 800, else none"""
    if K % 32 == 0 and K > 2048:
        return 32
    if K % 16 == 0 and K > 800:
        return 16
    return 0


SIZES8 = tuple(K for K in CB_SIZES if nsb8(K))


def mix64(seed: int, n: int) -> np.ndarray:
    """n 64-bit words: word i is the splitmix64 output of state seed + (i + 1) * 0x9E3779B97F4A7C15 (a Weyl sequence
    through a xorshift-multiply finaliser), in wrapping uint64 arithmetic"""
    z = (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed & _M64))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def pack8(lin: np.ndarray, K: int, n: int) -> np.ndarray:
    """Encoder-order int8 LLRs -> the 8-bit decoder's buffer (make_golden.pack8: stream s at s (K + 32), step w L + j
    of window w at j nsb + w, tails at 3 (K + 32) in encoder order)"""
    L = K // n
    buf = np.zeros(3 * (K + 32) + 12, np.int8)
    m = np.arange(K)
    pos = (m % L) * n + m // L
    for s in range(3):
        buf[s * (K + 32) + pos] = lin[s: 3 * K: 3]
    buf[3 * (K + 32):] = lin[3 * K:]
    return buf


@functools.lru_cache(maxsize=None)
def block8(K: int, cls: str):
    """(sent bits or None, the 8-bit decoder buffer) of one class"""
    n = 3 * K + 12
    w = mix64((K << 8) | CLASSES8.index(cls), n + K)
    bits = None
    if cls == "rand":
        lin = (w[:n] >> np.uint64(56)).astype(np.uint8).view(np.int8)
    else:
        amp, mult = LEVELS8[cls]
        bits = ((w[n:] >> np.uint64(63)) & np.uint64(1)).astype(np.uint8)
        enc = oracle.tcod_encode(bits, K).astype(np.int64)
        b = [((w[:n] >> np.uint64(8 * k)) & np.uint64(255)).astype(np.int64) for k in range(4)]
        noise = ((b[0] + b[1] + b[2] + b[3] - 510) * mult) >> 6
        lin = np.clip((2 * enc - 1) * amp + noise, -127, 127).astype(np.int8)
        bits.setflags(write=False)
    buf = pack8(lin, K, nsb8(K))
    buf.setflags(write=False)
    return bits, buf


def digest(row) -> np.ndarray:
    """16-byte truncated SHA-256 of decision bytes"""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(row, np.uint8).tobytes()).digest()[:16], np.uint8)


def ref_tdec8_traces(K: int):
    """{class: (NHALF, K/8) decision bytes of the reference's 8-bit decoder}; needs oracle/_ref"""
    R = oracle.ref()
    h = R.ref_tdec8_new(6144)
    out = {}
    for c in CLASSES8:
        work = np.array(block8(K, c)[1], np.int8)
        o = np.zeros(K // 8, np.uint8)
        tr = np.zeros((NHALF, K // 8), np.uint8)
        assert R.ref_tdec8_run(h, work, K, NHALF, o, tr.ctypes.data) == 0
        out[c] = tr
    R.ref_tdec8_free(h)
    return out
