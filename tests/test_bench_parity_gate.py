"""
``bench.py``'s ``cpu_baseline`` leg is also its parity gate: the oracle's answers for the timed workload are compared
bit for bit with what the GPU returned, and a difference ends the run non-zero.  (CPU tier: the "GPU" answer is handed in.)
"""

import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_fails_loudly_when_results_differ_from_the_oracle():
    """`cpu_baseline` is also the parity gate of the bench: a wrong GPU answer must end the run non-zero."""
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench

    class Args:
        rows, nbytes, metric, k, cpu_queries, queries = 200_000, 8, "hamming", 10, 16, 16

    q, _ = bench.make_queries(16, Args.rows, 1)
    from oracle import oracle_splitmix64_fill, oracle_topk

    words = oracle_splitmix64_fill(Args.rows, bench.SEED_CODES, stride=4).reshape(-1, 1)
    good = oracle_topk(0, np.arange(Args.rows, dtype=np.uint64), words, None, q, None, 10, fixed_nbytes=8)
    assert bench.cpu_baseline(Args, q, 1, good)["parity_checked_queries"] == 16
    bad = tuple(a.copy() for a in good)
    bad[0][5, 3] ^= np.uint64(1)
    with pytest.raises(SystemExit, match="PARITY FAILURE"):
        bench.cpu_baseline(Args, q, 1, bad)


def test_dump_outputs_writes_float_arrays_and_caps_their_size(tmp_path, monkeypatch):
    """`--dump-outputs`: the four arrays of an answer as float64 / float32 .npy; above the cap, a fixed seeded sample of rows."""
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench

    rng = np.random.default_rng(7)
    nq, k = 300, 10
    answer = (rng.integers(0, 2**40, size=(nq, k), dtype=np.uint64), rng.integers(0, 64, size=(nq, k), dtype=np.uint32),
              rng.integers(0, 64, size=(nq, k), dtype=np.uint16), np.full(nq, k, dtype=np.uint32))
    info = bench.dump_outputs(str(tmp_path / "all"), 3, answer)
    assert info["batch"] == 3 and info["queries_written"] == nq and "query_index.npy" not in info["files"]
    for name, a in zip(("keys", "hamming", "prefix_bits", "count"), answer):
        got = np.load(tmp_path / "all" / f"{name}.npy")
        assert got.dtype in (np.float32, np.float64)
        assert np.array_equal(got.astype(np.uint64), a.astype(np.uint64))
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 100 * (8 + 4 + 4) * k)
    sizes = []
    for run in ("a", "b"):
        info = bench.dump_outputs(str(tmp_path / run), 0, answer)
        sizes.append(sum(os.path.getsize(tmp_path / run / f) for f in info["files"]))
        assert 0 < info["queries_written"] < nq
    rows = np.load(tmp_path / "a" / "query_index.npy").astype(np.int64)
    assert np.array_equal(rows, np.load(tmp_path / "b" / "query_index.npy").astype(np.int64))
    assert np.array_equal(np.load(tmp_path / "a" / "keys.npy").astype(np.uint64), answer[0][rows])
    assert sizes[0] - 4 * 128 <= bench.DUMP_LIMIT_BYTES   # (.npy headers aside)
