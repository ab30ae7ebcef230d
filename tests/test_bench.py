"""bench.py's own plumbing on the host: the inputs it generates in worker processes are those synth.make_region builds, and
--dump-outputs writes what it says it writes (the GPU runs of bench.py are in tests/test_hip_dist.py)."""
import os

import numpy as np

import backends as B
import bench
from poreseq_amd import synth
from poreseq_amd.util import DEFAULT_PARAMS


def same_object(a, b):
    assert type(a) is type(b)
    if isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    elif hasattr(a, "__dict__"):
        assert sorted(vars(a)) == sorted(vars(b))
        for k in vars(a):
            same_object(getattr(a, k), getattr(b, k))
    else:
        assert a == b


def test_split_generation_equals_make_region():
    P = dict(DEFAULT_PARAMS, verbose=0)
    jobs = [(300, 5, 1002, 0.04), (420, 6, 101003, 0.04), (1000, 4, 5000, 0.04)]
    parts = list(bench._unaligned_regions(jobs))
    assert len(parts) == len(jobs)
    for (L, E, seed, _), part in zip(jobs, parts):
        want = synth.make_region(L, E, seed, B.oracle_swalign, P)
        got = bench._align_region(part, B.oracle_swalign)
        assert got[0] == want[0] and got[2] == want[2] and len(got[1]) == len(want[1]) == E
        for g, w in zip(got[1], want[1]):
            same_object(g, w)


def test_worker_processes_keep_the_order():
    jobs = [(200, 2, 7 + k, 0.04) for k in range(6)]
    serial = [bench._region_unaligned(j) for j in jobs]
    pooled = list(bench._unaligned_regions(jobs))
    assert len(pooled) == len(jobs)
    for s, p in zip(serial, pooled):
        assert s[0] == p[0] and s[2] == p[2]
        for a, b in zip(s[1], p[1]):
            same_object(a, b)


def test_dump_outputs(tmp_path):
    res = [("ACGT" * 3, 99.5), ("TTGCA", 100.0), ("", 97.25)]
    bench.dump_outputs(str(tmp_path), res)
    assert sorted(os.listdir(tmp_path)) == ["consensus_accuracy.npy", "consensus_bases.npy", "consensus_lengths.npy", "region_index.npy"]
    bases = np.load(tmp_path / "consensus_bases.npy")
    lens = np.load(tmp_path / "consensus_lengths.npy")
    acc = np.load(tmp_path / "consensus_accuracy.npy")
    idx = np.load(tmp_path / "region_index.npy")
    assert bases.dtype == np.float32 and bases.shape == (3, 12)
    assert lens.dtype == acc.dtype == idx.dtype == np.float64
    assert idx.tolist() == [0, 1, 2] and lens.tolist() == [12, 5, 0] and acc.tolist() == [99.5, 100.0, 97.25]
    for row, (s, _) in zip(bases, res):
        assert bytes(row[:len(s)].astype(np.uint8)).decode() == s and not row[len(s):].any()


def test_dump_outputs_samples_above_the_limit(tmp_path):
    res = [("ACGT" * 250, float(k)) for k in range(40)]
    bench.dump_outputs(str(tmp_path / "a"), res, limit_bytes=40000)
    bench.dump_outputs(str(tmp_path / "b"), res, limit_bytes=40000)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    idx = np.load(tmp_path / "a" / "region_index.npy")
    assert total <= 40000 and 0 < idx.size < 40 and np.all(np.diff(idx) > 0)
    assert np.array_equal(idx, np.load(tmp_path / "b" / "region_index.npy"))            # a fixed sample
    assert np.array_equal(np.load(tmp_path / "a" / "consensus_accuracy.npy"), idx)      # the rows of the regions named
