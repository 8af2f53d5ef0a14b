"""GPU parity of the 16-bit turbo decoders at EVERY code-block size of 36.212 (188 sizes) against the oracle
(oracle/orc_tdec.c, pinned to the reference at the same sizes and inputs by tests/test_tdec_sweep_oracle.py): decision
bytes after each half-iteration 1..8, bit for bit, on 19 blocks per K -- the input classes of tests/tdec_inputs.py
repeated: a codeword that never decodes, one that converges slowly, one that converges at once, a saturating one,
full-range random int16, all zero, constant 7.

tests/test_tdec_gpu.py runs 19 sizes at one input / output form each.  Here the window decoder (tdec_kernels.hip) runs
every one of its 142 sizes -- so every remainder L % 8 of the last beta-checkpoint segment for both window counts -- and
every size both with the in-kernel decision packing and with the separate decide pass, and with the 16-byte-load (TX)
instantiation on and off; the generic decoder (tdec_gen_cb.hip, tdec_gen.hip) runs all 188 sizes in each of its
schedules."""
import numpy as np
import pytest

import oracle
import tdec_inputs as TI
from golden_io import load

gpu = pytest.mark.gpu  # (the tests on the generator, the oracle and the committed digests run anywhere)

PAD_OUT = 768  # a decision row of the largest size: a multiple of 8 for every K
ODD_OUT = 771  # not a multiple of 8: the in-kernel packing's 8-byte stores are not taken


# ------------------------------------------------------------------ the sweep itself (CPU)

def test_sweep_covers_every_path():
    """Every value of every K-dependent choice of the kernels occurs over the 188 sizes (computed from K alone); a
    change of the size list or of a kernel's dispatch has to change tests/tdec_inputs.py with it."""
    assert list(TI.CB_SIZES) == oracle.cb_sizes()
    assert (len(TI.CB_SIZES), len(TI.WINDOW_SIZES), len(TI.SMALL_SIZES), len(TI.SIZES8)) == (188, 142, 46, 110)
    assert all(TI.nsb(K) == oracle.tdec_nsb(K) for K in TI.CB_SIZES)
    seen = {k: set() for k in TI.FEATURE_VALUES}
    for K in TI.CB_SIZES:
        f = TI.features(K)
        assert set(f) == set(seen)
        for k, v in f.items():
            seen[k].add(v)
    assert seen == TI.FEATURE_VALUES
    F = {K: TI.features(K) for K in TI.WINDOW_SIZES}
    # the sizes that decode both ways below
    assert sum(F[K]["fuse_capable"][1] for K in F) == 90 and sum(bool(F[K]["tx_capable"]) for K in F) == 42
    assert sum(not F[K]["full"][1] for K in F) == 94 and sum(F[K]["lat_odd"][1] for K in F) == 14


def test_reference_conditions():
    """Asserted on the oracle alone, so the GPU comparison cannot pass vacuously.  Over the 142 window sizes (observed
    with these seeds): class a is still wrong after 8 half-iterations at 142 sizes (>= 90 % asked); class b first
    equals the sent bits at half-iteration 3 / 4 / 5 / 6 / 7 at 12 / 52 / 64 / 13 / 1 sizes, never earlier (>= 90 %
    at 3 or later asked); class c at half-iteration 1 / 2 / 3 / 4 at 1 / 77 / 60 / 4 sizes (all by 4 asked)."""
    first = {c: np.array([TI.first_correct(TI.window_traces(K)[c], TI.block(K, c)[0]) for K in TI.WINDOW_SIZES])
             for c in ("a_fail", "b_slow", "c_fast")}
    n = len(TI.WINDOW_SIZES)
    assert (first["a_fail"] > TI.NHALF).sum() >= 0.9 * n
    assert ((first["b_slow"] >= 3) & (first["b_slow"] <= TI.NHALF)).sum() >= 0.9 * n
    assert (first["c_fast"] <= 4).all()
    # the small sizes: AUTO is the generic decoder there
    for K in TI.SMALL_SIZES:
        for c in TI.CLASSES:
            assert np.array_equal(TI.window_traces(K)[c], TI.generic_traces(K)[c]), (K, c)
    # the adversarial classes keep the recursion busy: random input changes its decisions between half-iterations
    live = sum(not np.array_equal(TI.window_traces(K)["e_rand"][6], TI.window_traces(K)["e_rand"][7])
               for K in TI.WINDOW_SIZES)
    assert live >= n // 2


def test_tdec8_sweep_fixture_is_live():
    """On the committed digests alone: the high class equals its sent bits after 2 half-iterations at every K (the
    reference decodes what the generator encoded, in the layout pack8 gives it), and at least half of the random-class
    traces still change between half-iterations 7 and 8 (live recursions, not converged ones are compared)."""
    z = load("tdec8_sweep.npz")
    Ks, cls, dig = z["K"], z["cls"], z["digest"]
    assert [int(k) for k in Ks[::3]] == list(TI.SIZES8) and [str(c) for c in cls[:3]] == list(TI.CLASSES8)
    live = 0
    for i in range(len(Ks)):
        K, c = int(Ks[i]), str(cls[i])
        if c == "high":
            assert np.array_equal(dig[i, 1], TI.digest(TI.decision_bytes(TI.block8(K, c)[0]))), K
        if c == "rand":
            live += not np.array_equal(dig[i, 6], dig[i, 7])
    assert live >= len(TI.SIZES8) // 2


# ------------------------------------------------------------------ GPU

def _expected(traces):
    """(NHALF, NBLOCKS, K/8): block i is class i % 7"""
    return np.stack([traces[TI.CLASSES[i % len(TI.CLASSES)]] for i in range(TI.NBLOCKS)], axis=1)


class _Bench:
    """One device input and output buffer large enough for every K and form"""

    def __init__(self):
        from srsran_amd.tdec import DeviceBuffer
        self.d_in = DeviceBuffer(TI.NBLOCKS * TI.SB_STRIDE * 2)
        self.d_out = DeviceBuffer(TI.NBLOCKS * ODD_OUT + 64)

    def load(self, rows, stride):
        host = np.zeros((TI.NBLOCKS, stride), np.int16)
        for i in range(TI.NBLOCKS):
            r = rows[i % len(rows)]
            host[i, : r.size] = r
        self.d_in.upload(host)

    def poison(self):
        from srsran_amd import lib
        lib().mi355_memset_dev(self.d_out.ptr, 0xA5, self.d_out.nbytes)

    def read(self, K, out_stride):
        return self.d_out.download(np.zeros((TI.NBLOCKS, out_stride), np.uint8))[:, : K // 8]

    def trace(self, dec, K, in_stride, out_stride, want, tag, bad):
        """Half-iterations 0..7 one launch each, the decisions after each against want[h]"""
        self.poison()
        for h in range(TI.NHALF):
            dec.halfit_dev(self.d_in.ptr, in_stride, TI.NBLOCKS, K, h, self.d_out.ptr, out_stride)
            got = self.read(K, out_stride)
            if not np.array_equal(got, want[h]):
                cbs = [i for i in range(TI.NBLOCKS) if not np.array_equal(got[i], want[h][i])]
                bad.append((K, tag, h + 1, cbs))
                return

    def whole(self, dec, K, in_stride, out_stride, nhalf, want, tag, bad):
        """nhalf half-iterations in one call (no decisions but the last's)"""
        self.poison()
        dec.run_dev(self.d_in.ptr, in_stride, TI.NBLOCKS, K, nhalf, self.d_out.ptr, out_stride)
        got = self.read(K, out_stride)
        if not np.array_equal(got, want[nhalf - 1]):
            bad.append((K, tag, nhalf, [i for i in range(TI.NBLOCKS) if not np.array_equal(got[i], want[nhalf - 1][i])]))


@pytest.fixture(scope="module")
def bench():
    return _Bench()


def window_forms(K):
    """(tag, input stride, output stride, decisions packed in the kernel, 16-byte loads) of every form K decodes in"""
    f = TI.features(K)
    plain = oracle.tdec_buf_len(K)  # 3 K + 108 int16: never a multiple of 16 bytes for a window size
    assert (2 * plain) % 16 and (2 * TI.SB_STRIDE) % 16 == 0
    cap, tx = f["fuse_capable"][1], bool(f["tx_capable"])
    forms = [("plain/K8", plain, K // 8, cap and (K // 8) % 8 == 0, False),
             ("slot/padded", TI.SB_STRIDE, PAD_OUT, cap, tx)]
    if cap:
        forms.append(("slot/odd", TI.SB_STRIDE, ODD_OUT, False, tx))
    if tx:
        forms.append(("plain/padded", plain, PAD_OUT, cap, False))
    return forms


@gpu
def test_window_decoder_every_size_every_form(bench):
    """142 sizes.  Each decodes from its plain buffers with output stride K/8 (what TdecBatch.run passes) and from
    softbuffer-slot strides into padded rows; every fuse-capable size also into rows of 771 bytes, so that it is
    decoded once by the in-kernel decision packing and once by the decide pass; every 16-window size with L % 8 == 0
    from a 16-byte-multiple input stride and from one that is not (TX on and off).  Every form must give the
    oracle's decisions after each half-iteration, so the forms agree with each other too."""
    from srsran_amd.tdec import TdecBatch
    dec = TdecBatch(0)
    bad, both_pack, both_tx = [], 0, 0
    for K in TI.WINDOW_SIZES:
        want = _expected(TI.window_traces(K))
        rows = [TI.block(K, c)[2] for c in TI.CLASSES]
        forms = window_forms(K)
        both_pack += {True, False} <= {fm[3] for fm in forms}
        both_tx += {True, False} <= {fm[4] for fm in forms}
        loaded = None
        for tag, ins, outs, _packed, _tx in sorted(forms, key=lambda fm: fm[1]):
            if loaded != ins:
                bench.load(rows, ins)
                loaded = ins
            bench.trace(dec, K, ins, outs, want, tag, bad)
            if tag in ("plain/K8", "slot/padded"):  # and without decisions in between: an even and an odd count
                bench.whole(dec, K, ins, outs, 8, want, tag + "/run8", bad)
                bench.whole(dec, K, ins, outs, 5, want, tag + "/run5", bad)
    dec.close()
    assert (both_pack, both_tx) == (90, 42)
    assert not bad, (len(bad), sorted({b[0] for b in bad}), bad[:12])


@gpu
@pytest.mark.parametrize("per_cb,warm", [(1, 32), (1, 0), (0, 32)], ids=["per_cb_warm32", "per_cb_warm0", "pair_lanes"])
def test_generic_decoder_every_size(bench, per_cb, warm):
    """All 188 sizes through the generic decoder on the linear layout: a workgroup per code block with the default
    warm-up and with none (every chunk but the first then starts from a wrong guess and is rerun), and two code
    blocks per lane (19 blocks: an unpaired last lane)."""
    from srsran_amd.tdec import TdecBatch
    dec = TdecBatch(0)
    dec.set_impl(1)
    dec.set_generic(per_cb, warm)
    dec.generic_reruns()  # arm the counter
    bad, no_rerun = [], []
    for K in TI.CB_SIZES:
        want = _expected(TI.generic_traces(K))
        stride = (3 * K + 12 + 7) // 8 * 8
        bench.load([TI.block(K, c)[1] for c in TI.CLASSES], stride)
        bench.trace(dec, K, stride, K // 8, want, f"per_cb={per_cb} warm={warm}", bad)
        if per_cb == 1 and warm == 0 and dec.generic_reruns() == 0:
            no_rerun.append(K)
    dec.close()
    assert not bad, (len(bad), sorted({b[0] for b in bad}), bad[:12])
    assert not no_rerun, no_rerun


@gpu
def test_auto_small_sizes_default_dispatch(bench):
    """The 46 sizes <= 400 as a caller with no knob set decodes them (AUTO picks the generic decoder and its schedule)"""
    from srsran_amd.tdec import TdecBatch
    dec = TdecBatch(0)
    bad = []
    for K in TI.SMALL_SIZES:
        want = _expected(TI.window_traces(K))
        stride = oracle.tdec_buf_len(K)
        bench.load([TI.block(K, c)[2] for c in TI.CLASSES], stride)
        bench.trace(dec, K, stride, K // 8, want, "auto", bad)
        bench.whole(dec, K, stride, K // 8, 8, want, "auto/run8", bad)
    dec.close()
    assert not bad, (len(bad), sorted({b[0] for b in bad}), bad[:12])
