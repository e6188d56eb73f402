"""
The joins on the matrix cores (``mfma_join_kernel``, csrc/mfma_join_kernel.hip.h) on an MI355X.

Every forced case runs ``join_within`` / ``join_between`` under ``join_mfma=1, join_mfma_min_rows=0`` (every launch on the matrix
cores), compares the result for exact equality (keys, distances, prefix bits, order) with the numpy brute force over all row
pairs and with the same call under ``join_mfma=0`` (the XOR + popcount kernel), and reads the statistics: ``join_mfma_launches``
rose under the first setting and stayed put under the second.  ``mfma=1`` is set next to it, so that the file also passes in a
session that runs under ``ISCC_HIP_OPTS="mfma=0"``.
"""

import contextlib
import ctypes
import errno

import numpy as np
import pytest

from iscc_search_amd import _lib
from iscc_search_amd.index import HipIndex, HipOptions
from test_duplicates import build_assets
from test_gpu_duplicates import mask_lengths, np_join, planted, table_with
from test_gpu_matches import np_join_between, nphd_sides, only, two_sides
from test_matches import split_pool

pytestmark = pytest.mark.gpu

# csrc/mfma_scan.h and mfma_scan.hip (mfma_groups_per_chunk): a block holds a chunk of an even number of 32-row groups, at most
# CHUNK_W1 rows of 64-bit codes; a table of up to CHUNK_W1 rows is ONE chunk, a longer one is cut into equal chunks
CHUNK_W1 = 1024
STEP_ROWS = 64          # streamed rows per wave and step (MFMA_JOIN_STEP_ROWS)
WAVES = 4               # waves per block (MFMA_JOIN_WAVES)
STEPS_PER_WAVE = 16     # the grid rule (mfma_join_live_blocks): one block per WAVES * STEPS_PER_WAVE steps a chunk has left
# the smallest table whose first chunk takes a second block: its waves stride over 8 steps, wave 0 runs 9 trips of its step
# loop (steps 0, 8, .. 64), the last of them on the partial step that holds one row
N_TWO_BLOCKS = STEP_ROWS * WAVES * STEPS_PER_WAVE + 1

NAMES = ("keys_a", "keys_b", "hamming", "prefix_bits")


def forced(engine):
    return engine.options(mfma=1, join_mfma=1, join_mfma_min_rows=0)


def valu(engine):
    return engine.options(join_mfma=0)


def counters(engine):
    st = engine.stats()
    return st["join_launches"], st["join_mfma_launches"]


def both_kernels(engine, call, exp=None):
    """``call()`` on the matrix cores and on the VALU kernel: equal to each other (and to ``exp``), the counters saying which ran."""
    l0, m0 = counters(engine)
    with forced(engine):
        got = call()
    l1, m1 = counters(engine)
    with valu(engine):
        ref = call()
    l2, m2 = counters(engine)
    assert m1 > m0 and l1 - l0 == m1 - m0, "the forced call did not run on the matrix cores alone"
    assert m2 == m1 and l2 > l1, "the join_mfma=0 call did not run on the VALU kernel alone"
    for g, e, name in zip(got, ref, NAMES):
        assert g.shape == e.shape and g.dtype == e.dtype and np.array_equal(g, e), name + " (matrix cores against VALU)"
    if exp is not None:
        for g, e, name in zip(got, exp, NAMES):
            assert g.shape == e.shape and np.array_equal(g, e), name + " (matrix cores against numpy)"
    return len(got[2])


def check_within(engine, table, keys, words, nb, mh):
    return both_kernels(engine, lambda: table.join_within(mh, 10_000_000), np_join(keys, words, nb, np.asarray(mh, dtype=np.int64)))


def check_between(engine, ta, tb, side_a, side_b, mh):
    return both_kernels(engine, lambda: ta.join_between(tb, mh, 10_000_000), np_join_between(side_a, side_b, mh))


@contextlib.contextmanager
def dropping(*tables):
    try:
        yield tables
    finally:
        for t in tables:
            t.drop()


@pytest.mark.parametrize("n", [2, 31, 32, 33, 63, 64, 65, CHUNK_W1 - 1, CHUNK_W1, CHUNK_W1 + 1, 2 * CHUNK_W1 + 1, N_TWO_BLOCKS, 5000])
def test_hamming64_self_join(hip_engine, n):
    rng = np.random.default_rng(n)
    words = planted(rng, n, 8, pool=max(2, n // 30))
    keys = rng.permutation(np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    nb = np.full(n, 8, dtype=np.uint8)
    with dropping(table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, keys, words, nb)) as (t,):
        total = 0
        for tau in (0, 5, 64) if n <= CHUNK_W1 + 1 else (0, 5):
            found = check_within(hip_engine, t, keys, words, nb, only(8, tau))
            assert tau != 64 or found == n * (n - 1) // 2       # every pair: the ring fills and is walked many times per step
            total += found
        assert total > 0
        before = counters(hip_engine)
        with forced(hip_engine):
            assert [len(a) for a in t.join_within(np.full(33, -1, dtype=np.int16), 10)] == [0, 0, 0, 0]
        assert counters(hip_engine) == before                   # nothing to join: nothing launched


@pytest.mark.parametrize("tau", [0, 64])
def test_all_zero_and_all_one_rows(hip_engine, tau):
    """Rows of no set bit (popc 0: every product sums to 0) and of 64 set bits, duplicated, among ordinary rows: on the held side
    and on the streamed side of every chunk."""
    rng = np.random.default_rng(3)
    n = 1500
    words = planted(rng, n, 8, pool=30)
    zeros = rng.choice(n, size=40, replace=False)
    words[zeros[:20]] = 0
    words[zeros[20:], 0] = np.uint64(0xFFFFFFFFFFFFFFFF)
    keys = rng.permutation(n).astype(np.uint64) + np.uint64(1)
    nb = np.full(n, 8, dtype=np.uint8)
    with dropping(table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, keys, words, nb)) as (t,):
        found = check_within(hip_engine, t, keys, words, nb, only(8, tau))
        assert found == n * (n - 1) // 2 if tau == 64 else found >= 2 * (20 * 19 // 2)
    # ... and across two tables: A's extreme rows against B's
    wa, wb = words[:900], words[900:].copy()
    wb[:5] = 0
    wb[5:10, 0] = np.uint64(0xFFFFFFFFFFFFFFFF)
    side_a = (keys[:900], wa, nb[:900])
    side_b = (keys[900:], wb, nb[900:])
    with dropping(table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, *side_a), table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, *side_b)) as (ta, tb):
        assert check_between(hip_engine, ta, tb, side_a, side_b, only(8, tau)) > 0
        assert check_between(hip_engine, tb, ta, side_b, side_a, only(8, tau)) > 0


def test_hamming128_two_word_keys(hip_engine):
    rng = np.random.default_rng(5)
    n = 3000
    words = planted(rng, n, 16, pool=100)
    keys = np.stack([rng.integers(0, 4, size=n, dtype=np.uint64), rng.permutation(n).astype(np.uint64)], axis=1)
    nb = np.full(n, 16, dtype=np.uint8)
    with dropping(table_with(hip_engine, _lib.METRIC_HAMMING, 2, 16, keys, words, nb)) as (t,):
        assert check_within(hip_engine, t, keys, words, nb, only(16, 7)) > 0


@pytest.mark.parametrize("nbytes", [24, 32])
@pytest.mark.parametrize("n,every_pair", [(1500, False), (300, True)])
def test_hamming_three_and_four_words(hip_engine, nbytes, n, every_pair):
    rng = np.random.default_rng(nbytes + n)
    words = planted(rng, n, nbytes, pool=50, flips=8)
    keys = rng.permutation(n).astype(np.uint64) + np.uint64(7)
    nb = np.full(n, nbytes, dtype=np.uint8)
    with dropping(table_with(hip_engine, _lib.METRIC_HAMMING, 1, nbytes, keys, words, nb)) as (t,):
        found = check_within(hip_engine, t, keys, words, nb, only(nbytes, 8 * nbytes if every_pair else nbytes))
        assert found == n * (n - 1) // 2 if every_pair else found > 0


@pytest.mark.parametrize("nbytes", [12, 20])
def test_hamming_partial_last_word(hip_engine, nbytes):
    """12 and 20 bytes: the last compared word is half a word -- its mask in the fragments and in popc(held row)."""
    rng = np.random.default_rng(nbytes)
    n = 1000
    nb = np.full(n, nbytes, dtype=np.uint8)
    words = mask_lengths(planted(rng, n, nbytes, pool=40), nb)
    keys = rng.permutation(n).astype(np.uint64) + np.uint64(1)
    with dropping(table_with(hip_engine, _lib.METRIC_HAMMING, 1, nbytes, keys, words, nb)) as (t,):
        assert check_within(hip_engine, t, keys, words, nb, only(nbytes, nbytes // 2)) > 0
        assert check_within(hip_engine, t, keys, words, nb, only(nbytes, 8 * nbytes)) == n * (n - 1) // 2


@pytest.mark.parametrize("tau", [0, "p", "8p"])
def test_nphd_mixed_lengths_across_segments(hip_engine, tau):
    """Every (la, lb) pair of segments; the held side is the segment with more rows, which for some pairs is the longer code's."""
    rng = np.random.default_rng(11)
    n = 700 if tau == "8p" else 4000
    nb = rng.choice([8, 12, 16, 24, 32], size=n, p=[0.1, 0.15, 0.2, 0.25, 0.3]).astype(np.uint8)
    words = mask_lengths(planted(rng, n, 32, pool=80, flips=8), nb)
    keys = rng.permutation(n).astype(np.uint64) + np.uint64(10)
    mh = np.full(33, -1, dtype=np.int16)
    for p in range(1, 33):
        mh[p] = 0 if tau == 0 else (p if tau == "p" else 8 * p)
    with dropping(table_with(hip_engine, _lib.METRIC_NPHD, 1, 32, keys, words, nb)) as (t,):
        found = check_within(hip_engine, t, keys, words, nb, mh)
        assert found == n * (n - 1) // 2 if tau == "8p" else found > 0


SIZES_BETWEEN = [(1, 5000), (5000, 1), (33, 2049), (1500, 1100)]


@pytest.mark.parametrize("n_a,n_b", SIZES_BETWEEN)
def test_hamming64_cross_join(hip_engine, n_a, n_b):
    """The table with more rows is held in LDS: table B for (1, 5 000) and (33, 2 049), table A for the other two."""
    rng = np.random.default_rng(1000 * n_a + n_b)
    wa, wb = two_sides(rng, n_a, n_b, 8, pool=max(2, (n_a + n_b) // 60))
    keys = rng.permutation(np.arange(1, n_a + n_b + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    ka, kb = keys[:n_a].copy(), keys[n_a:].copy()
    # every third asset of the smaller table is in the other one too, key and code: it pairs with itself
    shared = np.arange(0, min(n_a, n_b), 3)
    kb[shared] = ka[shared]
    wb[shared] = wa[shared]
    side_a = (ka, wa, np.full(n_a, 8, dtype=np.uint8))
    side_b = (kb, wb, np.full(n_b, 8, dtype=np.uint8))
    with dropping(table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, *side_a), table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, *side_b)) as (ta, tb):
        for tau in (0, 5, 64) if n_a * n_b <= 150_000 else (0, 5):
            found = check_between(hip_engine, ta, tb, side_a, side_b, only(8, tau))
            assert found >= len(shared) and (tau != 64 or found == n_a * n_b)
        with forced(hip_engine):
            ga, gb, _, _ = ta.join_between(tb, only(8, 0), 10_000_000)
        assert set(ka[shared].tolist()) <= {a for a, b in zip(ga.tolist(), gb.tolist()) if a == b}


@pytest.mark.parametrize("n_a,n_b", SIZES_BETWEEN)
def test_nphd_mixed_lengths_cross_join(hip_engine, n_a, n_b):
    rng = np.random.default_rng(7 * n_a + n_b)
    side_a, side_b = nphd_sides(rng, n_a, n_b)
    mh = np.array([-1] + list(range(1, 33)), dtype=np.int16)
    with dropping(table_with(hip_engine, _lib.METRIC_NPHD, 1, 32, *side_a), table_with(hip_engine, _lib.METRIC_NPHD, 1, 32, *side_b)) as (ta, tb):
        found = check_between(hip_engine, ta, tb, side_a, side_b, mh)
        assert found > 0 or min(n_a, n_b) == 1
        if min(n_a, n_b) == 1:        # one row against 5 000: every pair, whatever the codes
            every = np.array([-1] + [8 * p for p in range(1, 33)], dtype=np.int16)
            assert check_between(hip_engine, ta, tb, side_a, side_b, every) == n_a * n_b


def test_rows_behind_a_segments_end(hip_engine):
    """Removed rows stay in the columns behind the segment's count: they pair with nothing, held or streamed."""
    rng = np.random.default_rng(2)
    n, n_b = 3000, 1100
    words, wb = two_sides(rng, n, n_b, 8, pool=60)
    keys = np.arange(1, n + 1, dtype=np.uint64)
    nb = np.full(n, 8, dtype=np.uint8)
    side_b = (np.arange(5001, 5001 + n_b, dtype=np.uint64), wb, np.full(n_b, 8, dtype=np.uint8))
    mh = only(8, 4)
    with dropping(table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, keys, words, nb), table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, *side_b)) as (t, tb):
        gone = rng.choice(n, size=700, replace=False)
        assert t.remove(keys[gone]) == 700
        keep = np.setdiff1d(np.arange(n), gone)
        assert check_within(hip_engine, t, keys[keep], words[keep], nb[keep], mh) > 0
        side = (keys[keep], words[keep], nb[keep])
        assert check_between(hip_engine, t, tb, side, side_b, mh) > 0        # the shrunk table held (2 300 rows against 1 100)
        t.remove(keys[keep[1:]])
        before = counters(hip_engine)
        with forced(hip_engine):
            assert [len(a) for a in t.join_within(only(8, 64), 10)] == [0, 0, 0, 0]     # one row: no pair, nothing launched
        assert counters(hip_engine) == before
        side =(keys[keep[:1]], words[keep[:1]], nb[keep[:1]])
        assert check_between(hip_engine, tb, t, side_b, side, only(8, 64)) == n_b      # ... and streamed: its one row left
        t.remove(keys[keep[:1]])
        before = counters(hip_engine)
        with forced(hip_engine):
            assert [len(a) for a in t.join_within(mh, 10)] == [0, 0, 0, 0]
            assert [len(a) for a in t.join_between(tb, mh, 10)] == [0, 0, 0, 0]
        assert counters(hip_engine) == before


def test_capacity_is_exact_on_the_matrix_cores(hip_engine):
    rng = np.random.default_rng(9)
    n = 2000
    words = planted(rng, n, 8, pool=20)
    keys = np.arange(1, n + 1, dtype=np.uint64)
    with dropping(table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, keys, words, None)) as (t,):
        mh = only(8, 3)
        full = t.join_within(mh, 10_000_000)          # the session's kernel choice: 2 000 rows are below every default
        total = len(full[2])
        assert total > 100
        call = hip_engine._lib.isccsearch_join_within
        got_total = ctypes.c_uint64()
        with forced(hip_engine):
            _, m0 = counters(hip_engine)
            cap = total // 3
            out = [np.empty(cap, np.uint64), np.empty(cap, np.uint64), np.empty(cap, np.uint32), np.empty(cap, np.uint16)]
            rc = call(hip_engine.handle, t.id, _lib.ptr(mh), cap, *(_lib.ptr(a) for a in out), ctypes.byref(got_total))
            assert rc == -errno.ENOSPC and got_total.value == total
            out = [np.empty(total, np.uint64), np.empty(total, np.uint64), np.empty(total, np.uint32), np.empty(total, np.uint16)]
            rc = call(hip_engine.handle, t.id, _lib.ptr(mh), total, *(_lib.ptr(a) for a in out), ctypes.byref(got_total))
            assert rc == 0 and got_total.value == total
            assert counters(hip_engine)[1] == m0 + 2
        for g, e in zip(out, full):
            assert np.array_equal(g, e)


def test_default_dispatch_large_table_takes_the_matrix_cores(hip_engine):
    rng = np.random.default_rng(21)
    n, m, tau = 300_000, 2000, 3
    with dropping(hip_engine.open_table(_lib.METRIC_HAMMING, 1, 8)) as (t,):
        t.add_synthetic(8, n, seed=77, first_row=0, key_base=1)
        _, cols = t.export_rows(8, 0, n)
        extra = cols[0, rng.integers(0, n, size=m)].copy()
        for _ in range(3):
            extra ^= np.left_shift(np.uint64(1), rng.integers(0, 64, size=m).astype(np.uint64)) * (rng.random(m) < 0.7)
        t.add(np.arange(n + 1, n + m + 1, dtype=np.uint64), extra[:, None])
        mh = only(8, tau)
        l0, m0 = counters(hip_engine)
        with hip_engine.options(mfma=1, join_mfma=1):
            got = t.join_within(mh, 1_000_000)
        l1, m1 = counters(hip_engine)
        with hip_engine.options(mfma=1, join_mfma=0):
            ref = t.join_within(mh, 1_000_000)
        l2, m2 = counters(hip_engine)
        assert m1 > m0 and l1 - l0 == m1 - m0 and m2 == m1 and l2 > l1
        assert len(got[2]) >= m
        for g, e, name in zip(got, ref, NAMES):
            assert np.array_equal(g, e), name


def test_default_dispatch_small_table_stays_on_the_valu_kernel(hip_engine):
    rng = np.random.default_rng(22)
    n = 5000
    words = planted(rng, n, 8, pool=100)
    keys = rng.permutation(n).astype(np.uint64) + np.uint64(1)
    with dropping(table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, keys, words, None)) as (t,):
        l0, m0 = counters(hip_engine)
        with hip_engine.options(mfma=1, join_mfma=1):
            got = t.join_within(only(8, 5), 10_000_000)
        l1, m1 = counters(hip_engine)
        with hip_engine.options(mfma=1, join_mfma=0):
            ref = t.join_within(only(8, 5), 10_000_000)
        assert m1 == m0 and l1 > l0 and counters(hip_engine)[1] == m0
        assert len(got[2]) > 0
        for g, e, name in zip(got, ref, NAMES):
            assert np.array_equal(g, e), name


def test_mfma_off_turns_the_joins_matrix_core_path_off(hip_engine):
    """Option mfma = 0 means no matrix cores anywhere: a join that join_mfma alone would send there stays on the VALU kernel."""
    rng = np.random.default_rng(23)
    n = 600
    words = planted(rng, n, 8, pool=20)
    keys = np.arange(1, n + 1, dtype=np.uint64)
    with dropping(table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, keys, words, None)) as (t,):
        l0, m0 = counters(hip_engine)
        with hip_engine.options(mfma=0, join_mfma=1, join_mfma_min_rows=0):
            got = t.join_within(only(8, 5), 10_000_000)
        l1, m1 = counters(hip_engine)
        assert m1 == m0 and l1 > l0
        exp = np_join(keys, words, np.full(n, 8, dtype=np.uint8), np.asarray(only(8, 5), dtype=np.int64))
        for g, e, name in zip(got, exp, NAMES):
            assert np.array_equal(g, e), name


def test_find_duplicates_and_find_matches_return_the_same_lists(hip_engine):
    idx = HipIndex(hip_engine, HipOptions())
    try:
        idx.add_assets(build_assets(np.random.default_rng(17), 2000))
        _, m0 = counters(hip_engine)
        with forced(hip_engine):
            got = idx.find_duplicates()
        _, m1 = counters(hip_engine)
        with valu(hip_engine):
            ref = idx.find_duplicates()
        assert m1 > m0 and counters(hip_engine)[1] == m1
        assert len(got) > 200 and got == ref
    finally:
        idx.close()
    a, b, _ = split_pool(hip_engine, np.random.default_rng(17), 2000, 20)
    try:
        _, m0 = counters(hip_engine)
        with forced(hip_engine):
            got = a.find_matches(b)
        _, m1 = counters(hip_engine)
        with valu(hip_engine):
            ref = a.find_matches(b)
        assert m1 > m0 and counters(hip_engine)[1] == m1
        assert len(got) > 100 and got == ref
    finally:
        a.close()
        b.close()


def test_options_read_back_and_refuse_values_outside_their_range(hip_engine):
    with hip_engine.options(join_mfma=0, join_mfma_min_rows=12345):
        assert hip_engine.get_option("join_mfma") == 0 and hip_engine.get_option("join_mfma_min_rows") == 12345
        with hip_engine.options(join_mfma=1, join_mfma_min_rows=0):
            assert hip_engine.get_option("join_mfma") == 1 and hip_engine.get_option("join_mfma_min_rows") == 0
        for name, bad in (("join_mfma", 2), ("join_mfma", -1), ("join_mfma_min_rows", -1)):
            rc = hip_engine._lib.isccsearch_set_option(hip_engine.handle, name.encode(), bad)
            assert rc == -errno.EINVAL and name in hip_engine._lib.isccsearch_last_error().decode()
        assert hip_engine.get_option("join_mfma") == 0 and hip_engine.get_option("join_mfma_min_rows") == 12345
