"""bench.py --dump-outputs without a GPU: dump_outputs() on a stand-in workload that hands over host arrays the way a workload's
outputs() does (per-pair record fields, plus arrays of other shapes)."""
import os

import numpy as np

import bench


class _Stand:
    def __init__(self, n, seed=3):
        rng = np.random.default_rng(seed)
        self.n = n
        self.rec = rng.integers(-2**31, 2**31 - 1, size=(n, 4), dtype=np.int64).astype(np.int32)
        self.off = np.cumsum(rng.integers(0, 2**20, size=n + 1, dtype=np.int64)) + 2**40

    def outputs(self, k):
        per_pair = {f: self.rec[:, i] for i, f in enumerate(("score", "end_query", "end_ref", "flags"))}
        per_pair["length"] = self.off[1:] - self.off[:-1]
        return per_pair, {"offsets": self.off[:17]}


def _load(d, names):
    return {name: np.load(os.path.join(d, name + ".npy")) for name in names}


def test_dump_writes_every_output_exactly_in_float64(tmp_path):
    w = _Stand(1000)
    names = bench.dump_outputs(w, 7, str(tmp_path))
    assert names == sorted(["score", "end_query", "end_ref", "flags", "length", "offsets"])
    got = _load(str(tmp_path), names)
    per_pair, other = w.outputs(7)
    for name, want in list(per_pair.items()) + list(other.items()):
        assert got[name].dtype == np.float64 and got[name].shape == want.shape, name
        assert (got[name].astype(np.int64) == want).all(), name
    assert sorted(os.listdir(str(tmp_path))) == sorted(n + ".npy" for n in names)


def test_dump_past_the_limit_is_a_fixed_seeded_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT", 256 << 10)
    w = _Stand(20000)
    runs = []
    for k in range(2):
        d = str(tmp_path / str(k))
        names = bench.dump_outputs(w, 0, d)
        assert "sample_index" in names
        runs.append(_load(d, names))
        assert sum(x.nbytes for x in runs[-1].values()) <= bench.DUMP_LIMIT
    a, b = runs
    assert sorted(a) == sorted(b) and all((a[n] == b[n]).all() for n in a)
    idx = a["sample_index"].astype(np.int64)
    assert len(idx) > 1000 and (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < w.n
    per_pair, other = w.outputs(0)
    for name, want in per_pair.items():
        assert (a[name].astype(np.int64) == want[idx]).all(), name
    assert (a["offsets"].astype(np.int64) == other["offsets"]).all()
