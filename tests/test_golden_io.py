"""tests/golden_io.py: a fixture too large for one committed file is stored in parts and read back as one archive."""
import os

import numpy as np

import golden_io as G


def test_no_fixture_file_exceeds_the_limit():
    big = [(f, os.path.getsize(os.path.join(G.GOLDEN, f))) for f in os.listdir(G.GOLDEN)
           if os.path.getsize(os.path.join(G.GOLDEN, f)) > G.PART_LIMIT]
    assert not big, big


def test_split_fixtures_read_as_one_archive():
    for name in ("tdec8.npz", "pdcch.npz"):
        z = G.load(name)
        assert len(G.part_paths(name)) >= 2 and len(z.files) == len(set(z.files)) > 100
    assert "locations" in G.load("pdcch.npz") and G.load("pdcch.npz")["locations"].shape[1] == 36


def test_save_split_round_trip(tmp_path, monkeypatch):
    rng = np.random.default_rng(5)
    data = {f"a{i}": rng.integers(0, 256, 5000, dtype=np.uint8) for i in range(7)}
    data["n"] = np.int64(7)
    assert G.save_split(str(tmp_path), "one.npz", data) == [str(tmp_path / "one.npz")]
    monkeypatch.setattr(G, "PART_LIMIT", 16000)
    paths = G.save_split(str(tmp_path), "many.npz", data, raw_budget=11000)
    assert [os.path.basename(p) for p in paths] == [f"many.part{i}.npz" for i in range(4)]
    monkeypatch.setattr(G, "GOLDEN", str(tmp_path))
    for name in ("one.npz", "many.npz"):
        z = G.load(name)
        assert list(z.files) == list(data)
        assert all(np.array_equal(z[k], v) and z[k].dtype == np.asarray(v).dtype for k, v in data.items())
    # writing the whole form again removes the parts
    monkeypatch.setattr(G, "PART_LIMIT", 1 << 20)
    G.save_split(str(tmp_path), "many.npz", data)
    assert sorted(os.listdir(tmp_path)) == ["many.npz", "one.npz"]
