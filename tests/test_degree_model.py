"""
The host model of the degree and live-pair joins (``degree_model``) against a double Python loop over byte strings on tables of at most
64 rows, and against the pairs model of the join tests (``test_gpu_duplicates.np_join``) with its output filtered by the list (CPU tier).
"""

import numpy as np
import pytest

import degree_model as model
from test_gpu_duplicates import mask_lengths, np_join, planted


def loop_model(keys, words, nb, mh, live_keys):
    """(degree by key, links, pairs) by comparing the codes as byte strings, pair by pair"""
    code = [b"".join(int(w).to_bytes(8, "big") for w in row) for row in words]
    live = set(int(k) for k in live_keys)
    degree = {k: 0 for k in live}
    pairs = []
    for i in range(len(nb)):
        for j in range(len(nb)):
            a, b = int(keys[i]), int(keys[j])
            if i == j or a not in live or b not in live:
                continue
            p = int(min(nb[i], nb[j]))
            h = bin(int.from_bytes(code[i][:p], "big") ^ int.from_bytes(code[j][:p], "big")).count("1")
            if h <= int(mh[p]):
                degree[a] += 1
                if a < b:
                    pairs.append((a, b, h, 8 * p))
    return degree, len(pairs), sorted(pairs)


def tables():
    rng = np.random.default_rng(1)
    out = []
    for n, lengths in ((0, [8]), (1, [8]), (2, [8]), (17, [8]), (40, [32]), (64, [8, 16, 32]), (64, [12]), (50, [8, 12, 16, 24, 32])):
        words = planted(rng, n, 32, pool=4, flips=5) if n else np.zeros((0, 4), dtype=np.uint64)
        words[1:2] = words[:1]                               # one pair at distance 0 over any prefix in every table of two rows or more
        nb = rng.choice(lengths, size=n).astype(np.uint8)
        words = mask_lengths(words, nb) if n else words
        keys = rng.permutation(np.arange(100, 100 + n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
        mh = np.full(33, -1, dtype=np.int16)
        for p in lengths:
            mh[p] = 6
        out.append((keys, words, nb, mh))
    return out


def live_lists(rng, keys):
    srt = np.sort(keys)
    absent = np.array([1, 2, 3], dtype=np.uint64)            # below every key of the tables: the list stays ascending
    return [srt, srt[:0], srt[::2], np.concatenate([absent, srt[1::3]]), np.sort(rng.choice(srt, size=len(srt) // 2, replace=False))]


@pytest.mark.parametrize("case", range(8))
def test_against_the_double_loop(case):
    keys, words, nb, mh = tables()[case]
    rng = np.random.default_rng(case)
    found = 0
    for live in live_lists(rng, keys):
        degrees, links = model.join_degrees(keys, words, nb, mh, live)
        exp_degree, exp_links, exp_pairs = loop_model(keys, words, nb, mh, live)
        assert degrees.dtype == np.uint32 and degrees.tolist() == [exp_degree[int(k)] for k in live]
        assert links == exp_links and int(degrees.sum()) == 2 * links
        ka, kb, ham, pb = model.join_within_live(keys, words, nb, mh, live)
        assert (ka.dtype, kb.dtype, ham.dtype, pb.dtype) == (np.uint64, np.uint64, np.uint32, np.uint16)
        assert list(zip(ka.tolist(), kb.tolist(), ham.tolist(), pb.tolist())) == exp_pairs
        found += links
    assert found > 0 or len(nb) < 2


@pytest.mark.parametrize("case", range(2, 8))
def test_against_the_pairs_model_filtered_by_the_list(case):
    keys, words, nb, mh = tables()[case]
    rng = np.random.default_rng(100 + case)
    full = np_join(keys, words, nb, mh.astype(np.int64))
    for live in live_lists(rng, keys):
        keep = np.isin(full[0], live) & np.isin(full[1], live)
        got = model.join_within_live(keys, words, nb, mh, live)
        for g, e in zip(got, full):
            assert g.dtype == e.dtype and np.array_equal(g, e[keep])
        degrees, links = model.join_degrees(keys, words, nb, mh, live)
        assert links == int(keep.sum())
        ends = np.concatenate([full[0][keep], full[1][keep]])
        assert np.array_equal(degrees, np.bincount(np.searchsorted(live, ends), minlength=len(live)).astype(np.uint32))


def test_a_chain_and_a_hub():
    # a - b - c at 2 bits each, a and c 4 apart; five equal rows; radius 2
    x = 0x0123456789ABCDEF
    codes = [x, x ^ 0b11, x ^ 0b1111] + [0xFFFF0000FFFF0000] * 5
    keys = np.arange(10, 18, dtype=np.uint64)
    words = np.array(codes, dtype=np.uint64).reshape(8, 1)
    nb = np.full(8, 8, dtype=np.uint8)
    mh = np.full(33, -1, dtype=np.int16)
    mh[8] = 2
    degrees, links = model.join_degrees(keys, words, nb, mh, keys)
    assert degrees.tolist() == [1, 2, 1, 4, 4, 4, 4, 4] and links == 2 + 10
    # b unlisted: a and c lose their only partner; one of the five unlisted: the others lose one each
    live = np.array([10, 12, 13, 14, 15, 16], dtype=np.uint64)
    degrees, links = model.join_degrees(keys, words, nb, mh, live)
    assert degrees.tolist() == [0, 0, 3, 3, 3, 3] and links == 6
    assert [len(a) for a in model.join_within_live(keys, words, nb, mh, live)] == [6] * 4
