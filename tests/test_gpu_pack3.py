"""
``mfma_pack3_kernel`` (csrc/mfma_scan.hip: three row tiles per f32 accumulator, +-1 rows and queries, block threshold in the
start value, OR fold of indicator bits) against the oracle and against ``mfma_pack_kernel`` (option ``mfma_pack3=0``).

The kernel takes chunks of more than four query groups (> 128 queries).  Exercised here:
  * odd and even group counts (two instantiations: the even one carries the last group into the next step);
  * table sizes that are no multiple of the 192 rows a wave takes per step, masked prefixes (codes of 1..7 bytes);
  * planted near-duplicates: the thresholds of one chunk spread over 0..14, so the block threshold is loose for most queries
    and the candidate path's per-query test decides;
  * range-limited searches up to the radius that admits every row (the block threshold's "every row" mode);
  * several chunks walking stretches of rows (scans that start at row_begin > 0), k up to the largest (4 096).
"""

import numpy as np
import pytest

from oracle import np_within, oracle_topk

pytestmark = pytest.mark.gpu


def _table(engine, rng, n, nbytes=8):
    mask = np.uint64((0xFFFFFFFFFFFFFFFF << (8 * (8 - nbytes))) & 0xFFFFFFFFFFFFFFFF)
    words = rng.integers(0, 2**64, size=(n, 1), dtype=np.uint64) & mask
    words[rng.integers(0, n, size=8), 0] = np.uint64(0xFFFFFFFFFFFFFFFF) & mask
    words[rng.integers(0, n, size=8), 0] = np.uint64(1) << np.uint64(63)
    keys = rng.permutation(n).astype(np.uint64) + np.uint64(5)
    t = engine.open_table(0, 1, nbytes)
    t.add(keys, words)
    return t, keys, words, mask


def _queries(rng, words, nq, mask):
    """Random queries, and near-duplicates of table rows at 0..14 flipped bits (no all-zero query: that batch stays unpacked)."""
    q = rng.integers(0, 2**64, size=(nq, 1), dtype=np.uint64) & mask
    planted = nq // 2
    src = words[rng.integers(0, len(words), size=planted), 0].copy()
    for i in range(planted):
        for b in rng.choice(64, size=i % 15, replace=False):
            src[i] ^= np.uint64(1) << np.uint64(int(b))
    q[:planted, 0] = src & mask
    q[q[:, 0] == 0, 0] = np.uint64(1) << np.uint64(63)
    return q


def _assert_equal(got, exp, what):
    for g, e, name in zip(got, exp, ("keys", "hamming", "prefix_bits", "count")):
        np.testing.assert_array_equal(g, e, err_msg=f"{what}: {name}")


@pytest.fixture
def forced(hip_engine):
    with hip_engine.options(mfma=1, mfma_pack=1, mfma_pack3=1, mfma_min_queries=1, mfma_min_rows=1):
        yield hip_engine


def _both(engine, fn):
    with engine.options(mfma_pack3=1):
        a = fn()
    with engine.options(mfma_pack3=0):
        b = fn()
    return a, b


@pytest.mark.parametrize("n,k,nq,nbytes", [(191, 5, 160, 8), (193, 10, 200, 8), (70_003, 10, 160, 8), (100_003, 10, 192, 8),
                                           (150_001, 10, 224, 8), (300_001, 100, 256, 8), (200_000, 10, 1024, 8),
                                           (50_000, 10, 200, 1), (50_000, 10, 160, 3), (50_000, 10, 256, 5), (90_001, 20, 200, 7),
                                           (2_000_003, 10, 1024, 8), (2_000_003, 10, 160, 8), (1_000_001, 10, 1000, 8)])
def test_pack3_vs_oracle_and_pack(forced, n, k, nq, nbytes):
    rng = np.random.default_rng(5151 + n + nq + nbytes)
    t, keys, words, mask = _table(forced, rng, n, nbytes)
    try:
        q = _queries(rng, words, nq, mask)
        before = forced.stats()
        got, ref = _both(forced, lambda: t.search(q, None, k))
        assert forced.stats()["mfma_pack_launches"] > before["mfma_pack_launches"], "the batch did not run on the packed kernels"
        _assert_equal(got, oracle_topk(0, keys, words, None, q, None, k, fixed_nbytes=nbytes), "pack3 against the oracle")
        _assert_equal(got, ref, "pack3 against mfma_pack_kernel")
        with forced.options(self_tighten=0):                      # the level design (MODE_BOTH / MODE_STRETCH / MODE_COLLECT)
            levels = t.search(q, None, k)
        _assert_equal(levels, got, "levels against the single pass")
    finally:
        t.drop()


@pytest.mark.parametrize("radius,nq", [(0, 160), (1, 200), (12, 256), (14, 1024), (32, 160), (63, 200), (64, 160)])
def test_pack3_range_limited(forced, radius, nq):
    """Collect mode under GIVEN thresholds, up to the radius that admits every row (block threshold 65)."""
    rng = np.random.default_rng(77 + radius + nq)
    n = 3_000 if radius >= 31 else 150_000
    t, keys, words, mask = _table(forced, rng, n)
    try:
        q = _queries(rng, words, nq, mask)
        k = 4096 if radius >= 31 else 64
        got, ref = _both(forced, lambda: t.search_within(q, None, k, radius))
        for a, b in zip(got, ref):
            np.testing.assert_array_equal(a, b)
        gk, gh, gp, gc = got
        for i in range(len(q)):
            ek, eh, _ = np_within(words, 8, keys, q[i], 8, k, radius)
            assert int(gc[i]) == len(ek), (i, gc[i], len(ek))
            np.testing.assert_array_equal(gk[i, : len(ek)], ek)
            np.testing.assert_array_equal(gh[i, : len(ek)], eh)
    finally:
        t.drop()


@pytest.mark.parametrize("k,nq", [(64, 1100), (512, 1100), (4096, 160)])
def test_pack3_large_k_and_stretches(forced, k, nq):
    """Two chunks of queries walk 1 MB stretches (scans from row_begin > 0, a short last one); k up to the largest."""
    rng = np.random.default_rng(9000 + k)
    n = 600_001
    t, keys, words, mask = _table(forced, rng, n)
    try:
        q = _queries(rng, words, nq, mask)
        with forced.options(stretch_mb=1, mfma_stretch_factor=1):
            got, ref = _both(forced, lambda: t.search(q, None, k))
        _assert_equal(got, ref, "pack3 against mfma_pack_kernel")
        sel = np.arange(0, nq, 7)
        exp = oracle_topk(0, keys, words, None, q[sel], None, k, fixed_nbytes=8)
        _assert_equal(tuple(g[sel] for g in got), exp, "pack3 against the oracle")
    finally:
        t.drop()
