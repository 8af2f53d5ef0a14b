"""bench.py's options on CPU: --full gates every secondary leg, --dump-outputs samples the same rows in every run."""
import numpy as np
import pytest

import bench


def test_plain_run_switches_every_secondary_leg_off():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert not a.full and a.no_cpu and a.no_roofline and a.no_waterfall
    assert a.steps == 7 and a.warmup == 3 and a.dump_outputs is None


def test_full_keeps_the_legs_and_their_off_switches():
    a = bench.parse(["--full"])
    assert a.full and not (a.no_cpu or a.no_roofline or a.no_waterfall)
    a = bench.parse(["--full", "--no-cpu"])
    assert a.no_cpu and not a.no_roofline and not a.no_waterfall


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--workload", "enb", "--dump-outputs", "d"],
                                  ["--total-subframes", "600", "--dump-outputs", "d"]])
def test_rejected_arguments(argv):
    with pytest.raises(SystemExit):
        bench.parse(argv)


def test_dump_sample_is_fixed_sorted_and_distinct():
    assert np.array_equal(bench.dump_sample(5, 16), np.arange(5))
    s = bench.dump_sample(2048, 256)
    assert s.size == 256 and np.all(np.diff(s) > 0) and s[0] >= 0 and s[-1] < 2048
    assert np.array_equal(s, bench.dump_sample(2048, 256))


def test_dump_outputs_writes_float_arrays_within_the_limit(tmp_path):
    bench.dump_outputs(str(tmp_path / "o"), {"a": np.arange(6, dtype=np.uint8).reshape(2, 3),
                                             "b": np.array([1.5, np.nan], np.float64)})
    a, b = np.load(tmp_path / "o" / "a.npy"), np.load(tmp_path / "o" / "b.npy")
    assert a.dtype == np.float32 and a.shape == (2, 3) and a[1, 2] == 5
    assert b.dtype == np.float64 and b[0] == 1.5 and np.isnan(b[1])
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path / "p"), {"big": np.zeros((bench.DUMP_LIMIT // 4) + 1, np.float32)})
