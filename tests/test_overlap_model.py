"""
The host model of ``isccsearch_join_overlaps`` (``tests/overlap_model.py``) against cases worked by hand and against a plain
triple loop (CPU tier).  The GPU tier (``test_gpu_overlaps.py``) and ``test_shared_content.py`` rest on this model.
"""

import numpy as np
import pytest

from overlap_model import ENOSPC, chunk_keys, doc_freq, model_overlaps


def code(*bits):
    """A 64-bit code with the given bits set."""
    return sum(1 << b for b in bits)


def table(rows):
    """rows: [(asset, code)] -> (keys, words); a chunk's offset is its position in ``rows``."""
    return chunk_keys([a for a, _ in rows]), np.array([[c] for _, c in rows], dtype=np.uint64)


def as_tuples(records):
    return [tuple(int(r[f]) for f in ("src", "dst", "matched", "sum_hamming", "chunk_pairs")) for r in records]


def test_two_assets_sharing_two_of_three_chunks():
    x, y, z = code(1, 9), code(2, 17, 40), code(3, 30, 50, 60)
    keys, words = table([(10, x), (10, y), (10, z), (20, x), (20, y ^ 1), (20, code(5, 6, 7, 8, 55, 56, 57))])
    rc, rec, chunks, info = model_overlaps(keys, words, [10, 20], 1)
    assert rc == 0
    # (10 -> 20): rows x (distance 0) and y (distance 1) of asset 10 have a match; and the same from 20's side
    assert as_tuples(rec) == [(0, 1, 2, 1, 2), (1, 0, 2, 1, 2)]
    assert chunks.tolist() == [3, 3]
    assert info == {"chunk_pairs": 2, "records": 2, "live_rows": 6, "stop_chunks": 0}
    rc, rec, _, info = model_overlaps(keys, words, [10, 20], 0)
    assert as_tuples(rec) == [(0, 1, 1, 0, 1), (1, 0, 1, 0, 1)] and info["chunk_pairs"] == 1


def test_smallest_distance_of_three_candidates():
    s = code(0, 20, 40)
    cands = [s ^ code(1, 2, 3, 4, 5), s ^ code(6, 7), s ^ code(8, 9)]          # distances 5, 2, 2 to s; 7, 7, 4 among themselves
    keys, words = table([(1, s)] + [(2, c) for c in cands])
    rc, rec, chunks, info = model_overlaps(keys, words, [1, 2], 5)
    assert rc == 0
    # (1 -> 2): ONE matched row with its smallest distance 2, three chunk pairs; (2 -> 1): three matched rows, 5 + 2 + 2
    assert as_tuples(rec) == [(0, 1, 1, 2, 3), (1, 0, 3, 9, 3)]
    assert chunks.tolist() == [1, 3] and info["chunk_pairs"] == 3
    # the same candidates spread over two destination assets: per destination its own smallest distance
    keys, words = table([(1, s), (2, cands[0]), (2, cands[1]), (3, cands[2])])
    rc, rec, chunks, info = model_overlaps(keys, words, [1, 2, 3], 5)
    assert as_tuples(rec) == [(0, 1, 1, 2, 2), (0, 2, 1, 2, 1), (1, 0, 2, 7, 2), (1, 2, 1, 4, 1), (2, 0, 1, 2, 1), (2, 1, 1, 4, 1)]
    assert info["chunk_pairs"] == 4


def test_same_asset_repeat_is_no_pair():
    x = code(7, 8)
    keys, words = table([(5, x), (5, x), (5, x), (6, x)])
    rc, rec, chunks, info = model_overlaps(keys, words, [5, 6], 0)
    # three rows of asset 5 match the one row of asset 6; their three pairs among themselves do not exist
    assert as_tuples(rec) == [(0, 1, 3, 0, 3), (1, 0, 1, 0, 3)]
    assert chunks.tolist() == [3, 1] and info["chunk_pairs"] == 3
    rc, rec, chunks, info = model_overlaps(keys, words, [5], 0, capacity=0)
    assert rc == 0 and len(rec) == 0 and chunks.tolist() == [3] and info == {"chunk_pairs": 0, "records": 0, "live_rows": 3, "stop_chunks": 0}


def test_unlisted_asset_takes_no_part():
    x = code(11)
    keys, words = table([(1, x), (2, x), (3, x)])
    rc, rec, chunks, info = model_overlaps(keys, words, [1, 3, 4], 0)        # 2 is not listed; 4 has no rows
    assert as_tuples(rec) == [(0, 1, 1, 0, 1), (1, 0, 1, 0, 1)]
    assert chunks.tolist() == [1, 1, 0] and info["live_rows"] == 2 and info["chunk_pairs"] == 1


def test_stop_chunk_exactly_at_and_above_max_doc_freq():
    boiler, other = code(1), code(2, 3)
    rows = [(a, boiler) for a in (1, 2, 3)] + [(1, other), (2, other)]
    keys, words = table(rows)
    assert doc_freq(keys, words, 1000).tolist() == [3, 3, 3, 2, 2]
    # max_doc_freq 3: the boilerplate chunk is held by exactly 3 assets -- not above the cut, it pairs
    rc, rec, chunks, info = model_overlaps(keys, words, [1, 2, 3], 0, max_doc_freq=3)
    assert info == {"chunk_pairs": 4, "records": 6, "live_rows": 5, "stop_chunks": 0}
    # max_doc_freq 2: above the cut; only `other` pairs, the stop chunks still count as chunks of their assets
    rc, rec, chunks, info = model_overlaps(keys, words, [1, 2, 3], 0, max_doc_freq=2)
    assert as_tuples(rec) == [(0, 1, 1, 0, 1), (1, 0, 1, 0, 1)]
    assert chunks.tolist() == [2, 2, 1] and info == {"chunk_pairs": 1, "records": 2, "live_rows": 5, "stop_chunks": 3}
    # 0: no cut
    assert model_overlaps(keys, words, [1, 2, 3], 0, max_doc_freq=0)[3]["chunk_pairs"] == 4
    # the frequency is counted over the first dup_limit rows by ascending key: with dup_limit 2 it is 2, and nothing is cut at 2
    assert doc_freq(keys, words, 2).tolist() == [2, 2, 2, 2, 2]
    assert model_overlaps(keys, words, [1, 2, 3], 0, max_doc_freq=2, dup_limit=2)[3]["stop_chunks"] == 0
    # several rows of ONE asset count once
    keys2, words2 = table([(1, boiler), (1, boiler), (2, boiler)])
    assert doc_freq(keys2, words2, 1000).tolist() == [2, 2, 2]


def test_capacity_outcome():
    x = code(4)
    keys, words = table([(1, x), (2, x), (3, x)])
    rc, rec, chunks, info = model_overlaps(keys, words, [1, 2, 3], 0, capacity=2)
    assert rc == ENOSPC and info["chunk_pairs"] == 3
    rc, rec, chunks, info = model_overlaps(keys, words, [1, 2, 3], 0, capacity=3)
    assert rc == 0 and info["records"] == 6


def test_empty_and_one_row_tables():
    rc, rec, chunks, info = model_overlaps(np.zeros((0, 2), np.uint64), np.zeros((0, 1), np.uint64), [1, 2], 64)
    assert rc == 0 and len(rec) == 0 and chunks.tolist() == [0, 0] and info == {"chunk_pairs": 0, "records": 0, "live_rows": 0, "stop_chunks": 0}
    keys, words = table([(2, code(1))])
    rc, rec, chunks, info = model_overlaps(keys, words, [1, 2], 64, max_doc_freq=1)
    assert rc == 0 and len(rec) == 0 and chunks.tolist() == [0, 1] and info == {"chunk_pairs": 0, "records": 0, "live_rows": 1, "stop_chunks": 0}


def triple_loop(keys, words, asset_keys, max_hamming, max_doc_freq, dup_limit):
    """The definition, spelled out with Python ints."""
    n = len(keys)
    asset_keys = [int(a) for a in asset_keys]
    asset = [int(k[0]) for k in keys]
    codes = [tuple(int(w) for w in row) for row in words]
    live = [a in asset_keys for a in asset]
    stop = [False] * n
    if max_doc_freq > 0:
        for i in range(n):
            same = sorted((j for j in range(n) if codes[j] == codes[i]), key=lambda j: (int(keys[j][0]), int(keys[j][1])))[:dup_limit]
            stop[i] = live[i] and len({asset[j] for j in same}) > max_doc_freq
    recs = {}
    total = 0
    for i in range(n):
        for j in range(n):
            if i == j or not (live[i] and live[j]) or stop[i] or stop[j] or asset[i] == asset[j]:
                continue
            h = sum(bin(a ^ b).count("1") for a, b in zip(codes[i], codes[j]))
            if h > max_hamming:
                continue
            total += i < j
            r = recs.setdefault((asset_keys.index(asset[i]), asset_keys.index(asset[j])), {})
            r[i] = min(r.get(i, h), h)
            r["pairs"] = r.get("pairs", 0) + 1
    out = []
    for (src, dst), r in sorted(recs.items()):
        pairs = r.pop("pairs")
        out.append((src, dst, len(r), sum(r.values()), pairs))
    chunks = [sum(1 for i in range(n) if live[i] and asset[i] == a) for a in asset_keys]
    return out, chunks, {"chunk_pairs": total, "records": len(out), "live_rows": sum(live), "stop_chunks": sum(stop)}


@pytest.mark.parametrize("seed", range(12))
def test_against_a_triple_loop(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 41))
    W = int(rng.choice([1, 2, 4]))
    pool = rng.integers(0, 2**64, size=(max(2, n // 5), W), dtype=np.uint64)
    words = pool[rng.integers(0, len(pool), size=n)].copy()
    flips = rng.integers(0, 4, size=n)
    for i in range(n):
        for _ in range(int(flips[i])):
            words[i, rng.integers(0, W)] ^= np.uint64(1) << np.uint64(rng.integers(0, 64))
    assets = rng.integers(1, max(2, n // 3) + 1, size=n)
    keys = chunk_keys(assets, offsets=rng.permutation(n))
    listed = np.unique(np.concatenate([assets[rng.random(n) < 0.8], [99]])).astype(np.uint64)
    for max_hamming, max_doc_freq, dup_limit in ((0, 0, 1000), (3, 0, 1000), (3, 2, 1000), (5, 1, 3), (64 * W, 3, 1000)):
        rc, rec, chunks, info = model_overlaps(keys, words, listed, max_hamming, max_doc_freq, dup_limit)
        exp_rec, exp_chunks, exp_info = triple_loop(keys, words, listed, max_hamming, max_doc_freq, dup_limit)
        assert rc == 0 and as_tuples(rec) == exp_rec and chunks.tolist() == exp_chunks and info == exp_info
        assert all(int(r["reserved"]) == 0 for r in rec)
