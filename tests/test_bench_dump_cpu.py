"""bench.py --dump-outputs, the file side: what dump_outputs writes from the per-site tracks and the regional totals, without a GPU
(host arrays stand in for the device buffers)."""

import os

import numpy as np

import bench
from ferromic_amd import _abi


class _HostBuffer:
    def __init__(self, a):
        self.a = a

    def to_numpy(self, dtype, count):
        assert self.a.dtype == dtype and self.a.size == count
        return self.a.copy()


def _tracks(S, seed=3):
    rng = np.random.default_rng(seed)
    bufs = {n: _HostBuffer(rng.random(S)) for n in ("dxy", "pi1", "pi2", "num", "den")}
    bufs["alt"] = _HostBuffer(rng.integers(0, 2500, 2 * S, dtype=np.uint32))
    bufs["called"] = _HostBuffer(np.full(2 * S, 2500, dtype=np.uint32))
    t = _abi.HudsonTotals()
    t.numerator_sum, t.denominator_sum, t.sites_with_components = 1.25, 40.5, S
    t.pop[0].segregating_sites, t.pop[1].segregating_sites, t.pop[1].pi_sum = 7, 9, 0.5
    return bufs, t


def test_dump_is_a_seeded_sample_within_64_mb(tmp_path):
    S = 3_000_000
    bufs, t = _tracks(S)
    bench.dump_outputs(str(tmp_path / "a"), bufs, S, 0, t)
    bench.dump_outputs(str(tmp_path / "b"), bufs, S, 0, t)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    got = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    for n, x in got.items():
        assert x.dtype == np.float64
        assert np.array_equal(x, np.load(tmp_path / "b" / (n + ".npy"))), n
    idx = got["site_index"].astype(np.int64)
    assert len(idx) == bench.DUMP_SITES and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < S
    assert np.array_equal(got["sites_pi1"], bufs["pi1"].a[idx])
    assert np.array_equal(got["sites_alt"], bufs["alt"].a.reshape(2, S)[:, idx].astype(np.float64))
    assert got["totals_numerator_sum"].tolist() == [1.25] and got["totals_sites_with_components"].tolist() == [S]
    assert got["totals_pop_segregating_sites"].tolist() == [7, 9] and got["totals_pop_pi_sum"].tolist() == [0.0, 0.5]
    fields = {f for f, _ in _abi.HudsonTotals._fields_ if f != "pop"} | {"pop_" + f for f, _ in _abi.PopTotals._fields_}
    assert {n[len("totals_"):] for n in got if n.startswith("totals_")} == fields


def test_small_cohort_is_dumped_whole_and_ranks_keep_their_slabs(tmp_path):
    S = 1000
    bufs, t = _tracks(S)
    bench.dump_outputs(str(tmp_path), bufs, S, 0, t)
    assert np.array_equal(np.load(tmp_path / "site_index.npy"), np.arange(S, dtype=np.float64))
    assert np.array_equal(np.load(tmp_path / "sites_den.npy"), bufs["den"].a)
    bench.dump_outputs(str(tmp_path / "two"), bufs, S, 5000, t, rank=1, world=2)
    assert np.array_equal(np.load(tmp_path / "two" / "rank1_site_index.npy"), np.arange(5000, 5000 + S, dtype=np.float64))
    assert not any(n.startswith("rank0_") for n in os.listdir(tmp_path / "two"))
