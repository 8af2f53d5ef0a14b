"""Readers for the committed golden vectors (tests/golden/*.npz, made by tests/golden/make_golden.py
from the srsLTE reference compiled from its own sources)."""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


PART_LIMIT = 1 << 20  # no committed fixture file is larger than 1 MiB


class Parts:
    """A fixture stored as <stem>.part<i>.npz files, read as the one archive it would be (z[key], z.files)."""

    def __init__(self, paths):
        self.where = {}
        for p in paths:
            z = np.load(p, allow_pickle=False)
            for k in z.files:
                assert k not in self.where, (p, k)
                self.where[k] = z
        self.files = list(self.where)

    def __getitem__(self, key):
        return self.where[key][key]

    def __contains__(self, key):
        return key in self.where


def part_paths(name, directory=GOLDEN):
    stem = os.path.join(directory, name[: -len(".npz")])
    return sorted(glob.glob(glob.escape(stem) + ".part[0-9]*.npz"))


def load(name):
    path = os.path.join(GOLDEN, name)
    if os.path.exists(path):
        return np.load(path, allow_pickle=False)
    parts = part_paths(name, GOLDEN)
    if not parts:
        raise FileNotFoundError(path)
    return Parts(parts)


def save_split(directory, name, data, raw_budget=800_000):
    """np.savez_compressed(directory/name, **data) when that stays under PART_LIMIT; otherwise the arrays go, in
    order, into <stem>.part0.npz, .part1.npz ... of at most raw_budget array bytes each (these vectors hardly
    compress), every part checked against PART_LIMIT.  load(name) reads either form.  Returns the paths written."""
    for old in [os.path.join(directory, name)] + part_paths(name, directory):
        if os.path.exists(old):
            os.remove(old)
    whole = os.path.join(directory, name)
    np.savez_compressed(whole, **data)
    if os.path.getsize(whole) <= PART_LIMIT:
        return [whole]
    os.remove(whole)
    groups, size = [{}], 0
    for k, v in data.items():
        n = np.asarray(v).nbytes + 400  # + the entry's .npy header and archive records
        if groups[-1] and size + n > raw_budget:
            groups.append({})
            size = 0
        groups[-1][k] = v
        size += n
    paths = []
    for i, g in enumerate(groups):
        p = os.path.join(directory, f"{name[: -len('.npz')]}.part{i}.npz")
        np.savez_compressed(p, **g)
        assert os.path.getsize(p) <= PART_LIMIT, (p, os.path.getsize(p))
        paths.append(p)
    return paths


def tdec_auto_cases():
    z = load("tdec_auto.npz")
    out = []
    for i in range(int(z["ncases"])):
        out.append(dict(K=int(z[f"c{i}_K"]), kind=str(z[f"c{i}_kind"]), ebno=float(z[f"c{i}_ebno"]),
                        bits=z[f"c{i}_bits"], buf=z[f"c{i}_buf"], trace=z[f"c{i}_trace"]))
    return out


def tdec_generic_cases():
    z = load("tdec_generic.npz")
    return [dict(K=int(z[f"c{i}_K"]), lin=z[f"c{i}_lin"], bits=z[f"c{i}_bits"], trace=z[f"c{i}_trace"])
            for i in range(int(z["ncases"]))]


def rm_init_softbuffer():
    """Deterministic non-zero softbuffer content used when the rm_turbo goldens were made."""
    i = np.arange(18600, dtype=np.int64)
    return ((i * 7919) % 60001 - 30000).astype(np.int16)


def rm_cases():
    z = load("rm_turbo.npz")
    return [dict(K=int(z[f"c{i}_K"]), rv=int(z[f"c{i}_rv"]), e=z[f"c{i}_e"], out=z[f"c{i}_out"])
            for i in range(int(z["ncases"]))]


def rm_harq():
    z = load("rm_turbo.npz")
    return dict(K=int(z["harq_K"]), e0=z["harq_e0"], e2=z["harq_e2"], out=z["harq_out"])
