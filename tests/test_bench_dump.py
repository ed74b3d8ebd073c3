"""bench.py --dump-outputs: what every rank writes together stays under the stated bound whatever the number of ranks, in
float64, and the same inputs give the same files."""
import os

import numpy as np
import pytest

import bench


class _Shard:
    """Stands in for a solved rp.Batch of n F3 problems: the two read-backs dump_outputs uses."""

    def __init__(self, n, rank):
        rng = np.random.RandomState(rank)
        self.state = rng.standard_normal((n, 16))
        self.iters = rng.randint(0, 200, n).astype(np.int32)

    def get_state(self):
        return self.state.copy()

    def get_iters(self):
        return self.iters.copy(), np.zeros(len(self.iters), dtype=np.uint32)


@pytest.mark.parametrize("world, per_rank", [(1, 1 << 20), (1, (1 << 20) + 7), (2, 1 << 20), (8, 1 << 20)])
def test_dump_stays_under_60_mb_for_any_number_of_ranks(tmp_path, world, per_rank):
    summary = np.arange(4, dtype=np.float64)
    names = []
    for rank in range(world):
        names += bench.dump_outputs(_Shard(per_rank, rank), summary, str(tmp_path), rank, world)
    files = sorted(os.listdir(tmp_path))
    assert files == sorted(names) and names.count("summary.npy") == 1
    assert sum(os.path.getsize(tmp_path / f) for f in files) < 60e6
    for f in files:
        assert np.load(tmp_path / f).dtype == np.float64
    again = tmp_path / "again"
    bench.dump_outputs(_Shard(per_rank, world - 1), summary, str(again), world - 1, world)
    for f in os.listdir(again):
        assert np.array_equal(np.load(again / f), np.load(tmp_path / f))
