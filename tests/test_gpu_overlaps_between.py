"""
The device cross join of two simprint tables into asset overlaps (``isccsearch_join_overlaps_between`` through
``HipTable.join_overlaps_between``) and ``find_shared_matches`` on an MI355X.

Every case runs on both kernels -- ``forced(engine)`` (the launch on the matrix cores, ``mfma_join_kernel`` in its cross OVERLAP form) and
``valu(engine)`` (``join_scan_kernel`` in the same form), the ``join_launches`` / ``join_mfma_launches`` counters saying which
ran -- and compares records, both chunk arrays and info for exact equality with the host model (``tests/overlap_between_model.py``) and
with each other.  The shapes are the smallest at which the two emit paths and the held / streamed roles change: each table is held
(the one with more rows) in one case and streamed in the other, across the 1 024-row chunk, the 2 048-row slab and the second block.
"""

import errno

import numpy as np
import pytest

from iscc_search_amd import _lib, codec
from iscc_search_amd.index import HipIndex, HipOptions
from overlap_between_model import ENOSPC, INFO_NAMES, SKIP_SAME_ASSET, chunk_keys, model_overlaps_between
from test_gpu_duplicates import table_with
from test_gpu_join_mfma import N_TWO_BLOCKS, counters, dropping, forced, valu
from test_gpu_matches import two_sides
from test_shared_content import CT, library
from test_shared_matches import SharedOracleEngine

pytestmark = pytest.mark.gpu

MANY = 10_000_000
GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def sp_table(engine, nbytes, keys, words):
    return table_with(engine, _lib.METRIC_HAMMING, 2, nbytes, keys, words, None)


def raw_call(engine, ta, tb, max_hamming, keys_a, keys_b, capacity, max_doc_freq=0, dup_limit=1000, flags=SKIP_SAME_ASSET):
    """The C call itself: (rc, records, chunks_a, chunks_b, info array)."""
    keys_a = np.ascontiguousarray(keys_a, dtype=np.uint64)
    keys_b = np.ascontiguousarray(keys_b, dtype=np.uint64)
    records = np.zeros(2 * capacity, dtype=_lib.OVERLAP_DTYPE)
    chunks_a, chunks_b = np.zeros(len(keys_a), dtype=np.uint32), np.zeros(len(keys_b), dtype=np.uint32)
    info = np.zeros(6, dtype=np.uint64)
    rc = engine._lib.isccsearch_join_overlaps_between(
        engine.handle, ta.id, tb.id, max_hamming, max_doc_freq, dup_limit, len(keys_a), _lib.ptr(keys_a), len(keys_b), _lib.ptr(keys_b), flags,
        capacity, _lib.ptr(records) if capacity else None, _lib.ptr(chunks_a), _lib.ptr(chunks_b), _lib.ptr(info))
    return rc, records, chunks_a, chunks_b, info


def same_result(got, exp, what):
    (g_rec, g_a, g_b, g_info), (e_rec, e_a, e_b, e_info) = got, exp
    assert g_info == e_info, what
    assert g_rec.dtype == e_rec.dtype and g_rec.shape == e_rec.shape and g_rec.tobytes() == e_rec.tobytes(), what + ": records"
    assert np.array_equal(g_a, e_a) and np.array_equal(g_b, e_b), what + ": chunks"


def both_kernels(engine, call, exp=None, launches=True):
    """``call()`` on the matrix cores and on the VALU kernel: equal to each other (and to ``exp``), the counters saying which ran."""
    l0, m0 = counters(engine)
    with forced(engine):
        got = call()
    l1, m1 = counters(engine)
    with valu(engine):
        ref = call()
    l2, m2 = counters(engine)
    if launches:
        assert m1 == m0 + 1 and l1 == l0 + 1, "the forced call did not make its one launch on the matrix cores"
        assert m2 == m1 and l2 == l1 + 1, "the join_mfma=0 call did not make its one launch on the VALU kernel"
    else:
        assert (l2, m2) == (l0, m0), "an empty table launched a join kernel"
    same_result(got, ref, "matrix cores against VALU")
    if exp is not None:
        same_result(got, exp, "matrix cores against the model")
    return got


def check(engine, ta, tb, side_a, side_b, max_hamming, max_doc_freq=0, dup_limit=1000, skip=True, launches=True):
    (keys_a, words_a, listed_a), (keys_b, words_b, listed_b) = side_a, side_b
    rc, *exp = model_overlaps_between(keys_a, words_a, keys_b, words_b, listed_a, listed_b, max_hamming, max_doc_freq, dup_limit,
                                      SKIP_SAME_ASSET if skip else 0)
    assert rc == 0
    return both_kernels(engine, lambda: ta.join_overlaps_between(tb, max_hamming, listed_a, listed_b, max_doc_freq, MANY, dup_limit, skip),
                        tuple(exp), launches)


def deal(rng, n, ids):
    """n rows dealt to assets of 1-40 chunks (keys from ``ids``, consumed) in random row order: (asset per row, the assets)."""
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(int(rng.integers(1, 41)), n - sum(sizes)))
    mine = np.array([ids.pop() for _ in sizes], dtype=np.uint64)
    return rng.permutation(np.repeat(mine, sizes)), mine


def two_tables(rng, n_a, n_b, nbytes, pool, flips=6):
    """
    ((keys, words, listed) of A, the same of B): codes of both tables off one pool (``two_sides``), assets of 1-40 chunks in random row
    order with keys unrelated to it.  Row 0 of B copies row 0 of A (two different assets, both listed): a chunk pair at every radius.
    Every third asset of the smaller table is also in the other table, key and code.  Some assets are unlisted on each side, and each
    side lists an asset (5) that has no rows.
    """
    W = nbytes // 8
    wa, wb = (w[:, :W].copy() for w in two_sides(rng, n_a, n_b, nbytes, pool, flips))
    ids = (rng.choice(np.arange(1, 20 * (n_a + n_b) + 100, dtype=np.uint64), size=n_a + n_b, replace=False) * GOLDEN).tolist()
    (assets_a, ids_a), (assets_b, ids_b) = deal(rng, n_a, ids), deal(rng, n_b, ids)
    wb[0] = wa[0]
    small, large = ((assets_a, ids_a, wa), (assets_b, ids_b, wb)) if n_a <= n_b else ((assets_b, ids_b, wb), (assets_a, ids_a, wa))
    twins = small[1][::3]
    assert len(twins) < len(large[0])
    for x, asset in enumerate(twins.tolist()):
        src = int(np.nonzero(small[0] == asset)[0][0])
        large[0][1 + x] = asset
        large[2][1 + x] = small[2][src]
    sides = []
    for assets, own, words, extra in ((assets_a, ids_a, wa, twins if n_a > n_b else ()), (assets_b, ids_b, wb, twins if n_a <= n_b else ())):
        listed = [a for i, a in enumerate(own.tolist()) if len(own) <= 4 or i % 7 != 3 or a == int(assets[0])]
        listed = np.unique(np.array(listed + list(extra) + [int(assets[0]), 5], dtype=np.uint64))
        sides.append((chunk_keys(assets, offsets=rng.permutation(len(assets))), words, listed))
    return sides


SIZES = [(1, 5000), (5000, 1), (33, 2049), (1500, 1100), (N_TWO_BLOCKS, 300), (300, N_TWO_BLOCKS)]


@pytest.mark.parametrize("n_a,n_b", SIZES)
def test_simprints64(hip_engine, n_a, n_b):
    rng = np.random.default_rng(1000 * n_a + n_b)
    side_a, side_b = two_tables(rng, n_a, n_b, 8, pool=max(2, (n_a + n_b) // 60))
    with dropping(sp_table(hip_engine, 8, *side_a[:2]), sp_table(hip_engine, 8, *side_b[:2])) as (ta, tb):
        for tau in (0, 5):
            _, _, _, skipped = check(hip_engine, ta, tb, side_a, side_b, tau, skip=True)
            _, _, _, every = check(hip_engine, ta, tb, side_a, side_b, tau, skip=False)
            assert skipped["chunk_pairs"] >= 1 and skipped["records"] >= 2
            assert every["chunk_pairs"] > skipped["chunk_pairs"], "no pair of one asset key in the case"


@pytest.mark.parametrize("nbytes,tau", [(16, 7), (32, 9)])
def test_simprints128_and_256(hip_engine, nbytes, tau):
    rng = np.random.default_rng(nbytes)
    side_a, side_b = two_tables(rng, 3000, 2000, nbytes, pool=100, flips=8)
    with dropping(sp_table(hip_engine, nbytes, *side_a[:2]), sp_table(hip_engine, nbytes, *side_b[:2])) as (ta, tb):
        for max_hamming in (0, tau):
            _, _, _, info = check(hip_engine, ta, tb, side_a, side_b, max_hamming)
            assert info["chunk_pairs"] >= 1
        check(hip_engine, tb, ta, side_b, side_a, tau, skip=False)          # the sides exchanged: table A is the streamed one


def test_same_asset_pairs_take_no_slot(hip_engine):
    """1 025 identical chunks of asset 7 in either table: 1 050 625 row pairs within tau that are chunk pairs only without the flag."""
    n = 1025
    code = 0x0123456789ABCDEF
    ka, wa = chunk_keys(np.array([7] * n, dtype=np.uint64)), np.full((n, 1), code, dtype=np.uint64)
    kb, wb = chunk_keys(np.array([7] * n + [9, 9], dtype=np.uint64)), np.full((n + 2, 1), code, dtype=np.uint64)
    tuples = lambda rec: [tuple(int(v) for v in r) for r in rec.tolist()]
    with dropping(sp_table(hip_engine, 8, ka, wa), sp_table(hip_engine, 8, kb, wb)) as (ta, tb):
        for option in (forced, valu):
            with option(hip_engine):
                rc, rec, chunks_a, chunks_b, info = raw_call(hip_engine, ta, tb, 0, [7], [7, 9], 2 * n)
                assert rc == 0 and info.tolist() == [2 * n, 2, n, 0, n + 2, 0] and chunks_a.tolist() == [n] and chunks_b.tolist() == [n, 2]
                # only asset 7 of A against asset 9 of B: (src, dst, matched, reserved, sum_hamming, chunk_pairs)
                assert tuples(rec[:2]) == [(0, 1, n, 0, 0, 2 * n), (1, 0, 2, 1, 0, 2 * n)]
                rc, _, _, _, info = raw_call(hip_engine, ta, tb, 0, [7], [7, 9], 2 * n - 1)
                assert rc == -errno.ENOSPC and int(info[0]) == 2 * n
                # without asset 9 nothing takes a slot: capacity 0 is enough
                rc, _, chunks_a, chunks_b, info = raw_call(hip_engine, ta, tb, 0, [7], [7], 0)
                assert rc == 0 and info.tolist() == [0, 0, n, 0, n, 0] and chunks_a.tolist() == [n] and chunks_b.tolist() == [n]
                # without the flag the pairs of asset 7 with itself count too
                rc, _, _, _, info = raw_call(hip_engine, ta, tb, 0, [7], [7, 9], 0, flags=0)
                assert rc == -errno.ENOSPC and int(info[0]) == n * n + 2 * n
                rec, chunks_a, chunks_b, info = ta.join_overlaps_between(tb, 0, [7], [7, 9], 0, MANY, skip_same_asset=False)
                assert tuples(rec) == [(0, 0, n, 0, 0, n * n), (0, 1, n, 0, 0, 2 * n), (0, 0, n, 1, 0, n * n), (1, 0, 2, 1, 0, 2 * n)]
                assert info["chunk_pairs"] == n * n + 2 * n and info["records"] == 4
        check(hip_engine, ta, tb, (ka, wa, np.array([7], dtype=np.uint64)), (kb, wb, np.array([7, 9], dtype=np.uint64)), 0)


def test_every_pair_takes_a_slot(hip_engine):
    """
    Two tables of 300 identical rows, 300 listed assets of one chunk each on either side, no asset key in both: every candidate of the
    emit path takes a slot, 90 000 chunk pairs, so the count pass and the write pass have to agree on every one of them.
    """
    n = 300
    code = 0x0123456789ABCDEF
    listed_a, listed_b = np.arange(1, n + 1, dtype=np.uint64), np.arange(n + 1, 2 * n + 1, dtype=np.uint64)
    side_a = (chunk_keys(listed_a), np.full((n, 1), code, dtype=np.uint64), listed_a)
    side_b = (chunk_keys(listed_b), np.full((n, 1), code, dtype=np.uint64), listed_b)
    with dropping(sp_table(hip_engine, 8, *side_a[:2]), sp_table(hip_engine, 8, *side_b[:2])) as (ta, tb):
        rec, chunks_a, chunks_b, info = check(hip_engine, ta, tb, side_a, side_b, 0, skip=True)
        assert info["chunk_pairs"] == n * n == 90_000 and info["records"] == len(rec) == 2 * n * n == 180_000
        assert bool(np.all(rec["matched"] == 1)) and bool(np.all(rec["sum_hamming"] == 0)) and bool(np.all(rec["chunk_pairs"] == 1))
        assert chunks_a.tolist() == [1] * n and chunks_b.tolist() == [1] * n


def test_stop_chunks_per_table(hip_engine):
    """A chunk held by 50 assets of B and one of A: no pairs at max_doc_freq 49, 50 pairs at 50."""
    rng = np.random.default_rng(50)
    boiler = 0x5555AAAA3333CCCC
    assets, codes = [], []
    for a in range(1, 51):
        k = int(rng.integers(2, 6))
        assets += [a] * (k + 1)
        codes += rng.integers(0, 2**64, size=k, dtype=np.uint64).tolist() + [boiler]
    order = rng.permutation(len(assets))
    kb = chunk_keys(np.array(assets, dtype=np.uint64)[order], offsets=rng.permutation(len(assets)))
    wb = np.array(codes, dtype=np.uint64)[order][:, None]
    ka = chunk_keys(np.array([1000, 1000, 1001], dtype=np.uint64))
    wa = np.array([[boiler], [0x1111], [0x2222]], dtype=np.uint64)
    side_a, side_b = (ka, wa, np.array([1000, 1001], dtype=np.uint64)), (kb, wb, np.arange(1, 51, dtype=np.uint64))
    with dropping(sp_table(hip_engine, 8, ka, wa), sp_table(hip_engine, 8, kb, wb)) as (ta, tb):
        builds = hip_engine.stats()["freq_builds"]
        _, _, _, info = check(hip_engine, ta, tb, side_a, side_b, 0, max_doc_freq=0)
        assert info["chunk_pairs"] == 50 and info["records"] == 100 and info["stop_chunks_a"] == info["stop_chunks_b"] == 0
        assert hip_engine.stats()["freq_builds"] == builds, "max_doc_freq 0 built a frequency column"
        rec, _, chunks_b, info = check(hip_engine, ta, tb, side_a, side_b, 0, max_doc_freq=49)
        assert len(rec) == 0 and info["chunk_pairs"] == 0 and info["stop_chunks_a"] == 0 and info["stop_chunks_b"] == 50
        assert int(chunks_b.sum()) == len(kb)                                # stop chunks still count
        assert hip_engine.stats()["freq_builds"] == builds + 2, "one column per table, built once"
        _, _, _, info = check(hip_engine, ta, tb, side_a, side_b, 0, max_doc_freq=50)
        assert info["chunk_pairs"] == 50 and info["stop_chunks_b"] == 0
        assert hip_engine.stats()["freq_builds"] == builds + 2
        # the other way round: the chunk is frequent in the table that is now A
        _, _, _, info = check(hip_engine, tb, ta, side_b, side_a, 0, max_doc_freq=49)
        assert info["chunk_pairs"] == 0 and info["stop_chunks_a"] == 50 and info["stop_chunks_b"] == 0
        # a column counted over fewer rows: with dup_limit 20 the chunk has frequency 20
        _, _, _, info = check(hip_engine, ta, tb, side_a, side_b, 0, max_doc_freq=19, dup_limit=20)
        assert info["stop_chunks_b"] == 50
        _, _, _, info = check(hip_engine, ta, tb, side_a, side_b, 0, max_doc_freq=20, dup_limit=20)
        assert info["stop_chunks_b"] == 0 and info["chunk_pairs"] == 50


def test_the_smallest_distance(hip_engine):
    s = 0x00FF00FF0F0F3355
    flip = lambda *bits: s ^ sum(1 << b for b in bits)
    cands = [flip(1, 2, 3, 4, 5), flip(6, 7), flip(8, 9)]       # 5, 2, 2 bits off s
    tuples = lambda rec: [tuple(int(r[f]) for f in ("reserved", "src", "dst", "matched", "sum_hamming", "chunk_pairs")) for r in rec]
    side_a = (chunk_keys([1]), np.array([[s]], dtype=np.uint64), np.array([1], dtype=np.uint64))
    side_b = (chunk_keys([2, 2, 2]), np.array([[c] for c in cands], dtype=np.uint64), np.array([2], dtype=np.uint64))
    with dropping(sp_table(hip_engine, 8, *side_a[:2]), sp_table(hip_engine, 8, *side_b[:2])) as (ta, tb):
        rec, chunks_a, chunks_b, info = check(hip_engine, ta, tb, side_a, side_b, 5)
        assert tuples(rec) == [(0, 0, 0, 1, 2, 3), (1, 0, 0, 3, 9, 3)] and chunks_a.tolist() == [1] and chunks_b.tolist() == [3]
        rec, _, _, _ = check(hip_engine, tb, ta, side_b, side_a, 5)
        assert tuples(rec) == [(0, 0, 0, 3, 9, 3), (1, 0, 0, 1, 2, 3)]


def test_capacity_is_exact_on_both_kernels(hip_engine):
    rng = np.random.default_rng(9)
    side_a, side_b = two_tables(rng, 1500, 1100, 8, pool=30)
    (ka, wa, la), (kb, wb, lb) = side_a, side_b
    rc, *exp = model_overlaps_between(ka, wa, kb, wb, la, lb, 3)
    total = exp[3]["chunk_pairs"]
    assert total > 100
    assert model_overlaps_between(ka, wa, kb, wb, la, lb, 3, capacity=total - 1)[0] == ENOSPC
    with dropping(sp_table(hip_engine, 8, ka, wa), sp_table(hip_engine, 8, kb, wb)) as (ta, tb):
        for option in (forced, valu):
            with option(hip_engine):
                rc, _, _, _, info = raw_call(hip_engine, ta, tb, 3, la, lb, total - 1)
                assert rc == -errno.ENOSPC and int(info[0]) == total
                assert "capacity" in hip_engine._lib.isccsearch_last_error().decode()
                rc, _, _, _, info = raw_call(hip_engine, ta, tb, 3, la, lb, 0)
                assert rc == -errno.ENOSPC and int(info[0]) == total
                rc, rec, chunks_a, chunks_b, info = raw_call(hip_engine, ta, tb, 3, la, lb, total)
                assert rc == 0
                same_result((rec[: int(info[1])], chunks_a, chunks_b, dict(zip(INFO_NAMES, info.tolist()))), tuple(exp), "capacity == total")
        with pytest.raises(ValueError, match="exceed max_pairs"):
            ta.join_overlaps_between(tb, 3, la, lb, 0, total - 1)
        assert ta.join_overlaps_between(tb, 3, la, lb, 0, total)[3] == exp[3]


def test_rows_behind_a_segments_end(hip_engine):
    rng = np.random.default_rng(2)
    side_a, side_b = two_tables(rng, 3000, 2500, 8, pool=60)
    (ka, wa, la), (kb, wb, lb) = side_a, side_b
    with dropping(sp_table(hip_engine, 8, ka, wa), sp_table(hip_engine, 8, kb, wb)) as (ta, tb):
        gone_a = rng.choice(np.arange(1, 3000), size=700, replace=False)
        assert ta.remove(ka[gone_a]) == 700
        keep_a = np.setdiff1d(np.arange(3000), gone_a)
        _, _, _, info = check(hip_engine, ta, tb, (ka[keep_a], wa[keep_a], la), side_b, 4)
        assert info["chunk_pairs"] > 0 and info["live_rows_a"] <= len(keep_a)
        gone_b = rng.choice(np.arange(1, 2500), size=900, replace=False)       # now B is the smaller, streamed table
        assert tb.remove(kb[gone_b]) == 900
        keep_b = np.setdiff1d(np.arange(2500), gone_b)
        _, _, _, info = check(hip_engine, ta, tb, (ka[keep_a], wa[keep_a], la), (kb[keep_b], wb[keep_b], lb), 4)
        assert info["chunk_pairs"] > 0 and info["live_rows_b"] <= len(keep_b)
        ta.remove(ka[keep_a[1:]])                                              # one row: still a launch
        rec, chunks_a, _, info = check(hip_engine, ta, tb, (ka[:1], wa[:1], la), (kb[keep_b], wb[keep_b], lb), 64, skip=False)
        assert info["live_rows_a"] == 1 and info["chunk_pairs"] == info["live_rows_b"] and int(chunks_a.sum()) == 1
        ta.remove(ka[:1])                                                      # empty: nothing launched, chunks and info still filled
        empty = (ka[:0], wa[:0], la)
        rec, chunks_a, chunks_b, info = check(hip_engine, ta, tb, empty, (kb[keep_b], wb[keep_b], lb), 64, launches=False)
        assert len(rec) == 0 and info["chunk_pairs"] == 0 and info["live_rows_a"] == 0 and info["live_rows_b"] == int(chunks_b.sum()) > 0
        rec, _, _, info = check(hip_engine, tb, ta, (kb[keep_b], wb[keep_b], lb), empty, 64, max_doc_freq=5, launches=False)
        assert len(rec) == 0 and info["live_rows_a"] > 0 and info["live_rows_b"] == 0


def test_refused_arguments_leave_the_outputs_untouched(hip_engine):
    words = np.array([[5], [5], [6]], dtype=np.uint64)
    call = hip_engine._lib.isccsearch_join_overlaps_between
    last_error = lambda: hip_engine._lib.isccsearch_last_error().decode()
    with dropping(sp_table(hip_engine, 8, chunk_keys([1, 2, 3]), words), sp_table(hip_engine, 8, chunk_keys([4, 5, 6]), words),
                  hip_engine.open_table(_lib.METRIC_HAMMING, 1, 8), hip_engine.open_table(_lib.METRIC_NPHD, 1, 32),
                  hip_engine.open_table(_lib.METRIC_HAMMING, 2, 16)) as (ta, tb, t_kw1, t_nphd, t_wide):
        t_kw1.add(np.array([1, 2], dtype=np.uint64), words[:2])
        good_a, good_b = np.array([1, 2, 3], dtype=np.uint64), np.array([4, 5, 6], dtype=np.uint64)
        records = np.full(16, 0xEE, dtype=np.uint8).repeat(32).view(_lib.OVERLAP_DTYPE)
        chunks_a, chunks_b = np.full(3, 0xEEEEEEEE, dtype=np.uint32), np.full(3, 0xEEEEEEEE, dtype=np.uint32)
        info = np.full(6, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
        P = _lib.ptr
        base = dict(h=hip_engine.handle, table_a=ta.id, table_b=tb.id, max_hamming=0, max_doc_freq=0, dup_limit=1000, n_assets_a=3, asset_keys_a=P(good_a),
                    n_assets_b=3, asset_keys_b=P(good_b), flags=1, capacity=4, out_pairs=P(records), out_chunks_a=P(chunks_a), out_chunks_b=P(chunks_b),
                    out_info=P(info))
        unsorted, repeated = np.array([1, 3, 2], dtype=np.uint64), np.array([4, 5, 5], dtype=np.uint64)
        cases = [
            (dict(h=None), -errno.EINVAL, "handle"),
            (dict(asset_keys_a=None), -errno.EINVAL, "NULL"),
            (dict(asset_keys_b=None), -errno.EINVAL, "NULL"),
            (dict(out_chunks_a=None), -errno.EINVAL, "NULL"),
            (dict(out_chunks_b=None), -errno.EINVAL, "NULL"),
            (dict(out_info=None), -errno.EINVAL, "NULL"),
            (dict(out_pairs=None), -errno.EINVAL, "out_pairs"),
            (dict(table_b=ta.id), -errno.EINVAL, "isccsearch_join_overlaps joins a table with itself"),
            (dict(table_a=t_kw1.id), -errno.EINVAL, f"table {t_kw1.id} has"),
            (dict(table_b=t_kw1.id), -errno.EINVAL, "key_words"),
            (dict(table_b=t_nphd.id), -errno.EINVAL, "HAMMING"),
            (dict(table_b=t_wide.id), -errno.EINVAL, "max_bytes"),
            (dict(n_assets_a=0), -errno.EINVAL, "n_assets_a"),
            (dict(n_assets_a=1 << 31), -errno.EINVAL, "n_assets_a"),
            (dict(n_assets_b=0), -errno.EINVAL, "n_assets_b"),
            (dict(n_assets_b=1 << 31), -errno.EINVAL, "n_assets_b"),
            (dict(asset_keys_a=P(unsorted)), -errno.EINVAL, "asset_keys_a[2]"),
            (dict(asset_keys_b=P(repeated)), -errno.EINVAL, "asset_keys_b[2]"),
            (dict(max_hamming=-1), -errno.EINVAL, "max_hamming"),
            (dict(max_doc_freq=11, dup_limit=10), -errno.EINVAL, "dup_limit"),
            (dict(flags=3), -errno.EINVAL, "flags"),
            (dict(capacity=1 << 31), -errno.E2BIG, "32 bits"),
        ]
        before = counters(hip_engine), hip_engine.stats()["freq_builds"]
        for change, want, word in cases:
            args = dict(base, **change)
            rc = call(*args.values())
            assert rc == want and word in last_error(), (change, rc, last_error())
            untouched = all(bool(np.all(x.view(np.uint8) == 0xEE)) for x in (records, chunks_a, chunks_b, info))
            assert untouched, change
        assert (counters(hip_engine), hip_engine.stats()["freq_builds"]) == before
        with pytest.raises(ValueError, match="another engine"):
            ta.join_overlaps_between(object(), 0, good_a, good_b, 0, 10)
        # what is allowed: out_pairs NULL with capacity 0 (here -ENOSPC: codes 5, 5, 6 on either side give 5 chunk pairs), no flag,
        # max_doc_freq == dup_limit
        assert call(*dict(base, capacity=0, out_pairs=None).values()) == -errno.ENOSPC and int(info[0]) == 5
        assert call(*dict(base, capacity=8, flags=0, max_doc_freq=10, dup_limit=10).values()) == 0
        assert info.tolist() == [5, 10, 3, 0, 3, 0] and chunks_a.tolist() == [1, 1, 1] and chunks_b.tolist() == [1, 1, 1]


def test_default_dispatch_small_tables_stay_on_the_valu_kernel(hip_engine):
    rng = np.random.default_rng(22)
    side_a, side_b = two_tables(rng, 5000, 5000, 8, pool=100)
    (ka, wa, la), (kb, wb, lb) = side_a, side_b
    with dropping(sp_table(hip_engine, 8, ka, wa), sp_table(hip_engine, 8, kb, wb)) as (ta, tb):
        l0, m0 = counters(hip_engine)
        with hip_engine.options(mfma=1, join_mfma=1):
            got = ta.join_overlaps_between(tb, 5, la, lb, 0, MANY)
        l1, m1 = counters(hip_engine)
        assert m1 == m0 and l1 == l0 + 1
        rc, *exp = model_overlaps_between(ka, wa, kb, wb, la, lb, 5)
        same_result(got, tuple(exp), "default dispatch against the model")


def test_find_shared_matches_end_to_end(hip_engine):
    """Two libraries of about 300 assets and 3 000 chunks each, dealt alternately from one generated library, so that assets of A
    contain runs of B's chunks and the other way round.  The device result on both kernels equals the model-backed index's, and -- for 20
    assets of A -- what a simprint search of B's table by the asset's own chunks lists: ``search_raw`` asks for limit x oversampling
    > MAX_K neighbours, i.e. every row within the radius (B's table has fewer than 4 096 rows: no list fills the cap); under constant IDF
    its score of asset b is the mean over a's n chunks of the best similarity found in b -- ``coverage_a``, summed in another order:
    relative (n + 2) * 2^-52, the bound ``test_find_shared_content_end_to_end`` derives."""
    assets = library(np.random.default_rng(31), 600, chunks=(4, 14))
    assets_a, assets_b = assets[0::2], assets[1::2]
    cpu_engine = SharedOracleEngine()
    cpu_a, cpu_b = HipIndex(cpu_engine, HipOptions()), HipIndex(cpu_engine, HipOptions())
    cpu_a.add_assets(assets_a)
    cpu_b.add_assets(assets_b)
    exp = cpu_a.find_shared_matches(cpu_b, max_doc_freq=0)
    a, b = HipIndex(hip_engine, HipOptions()), HipIndex(hip_engine, HipOptions())
    try:
        a.add_assets(assets_a)
        b.add_assets(assets_b)
        table_b = b._sp_tables[CT]
        assert 2500 < a._sp_tables[CT].size < _lib.MAX_K and 2500 < table_b.size < _lib.MAX_K
        _, m0 = counters(hip_engine)
        with forced(hip_engine):
            got = a.find_shared_matches(b, max_doc_freq=0)
        _, m1 = counters(hip_engine)
        with valu(hip_engine):
            ref = a.find_shared_matches(b, max_doc_freq=0)
        assert m1 == m0 + 1 and counters(hip_engine)[1] == m1
        assert len(got) > 100 and got == exp and ref == exp
        kwargs = dict(min_chunks=2, min_coverage=0.2, max_doc_freq=5)
        assert b.find_shared_matches(a, **kwargs) == cpu_b.find_shared_matches(cpu_a, **kwargs)
        by_asset = {}
        for p in got:
            t = p.types[CT]
            by_asset.setdefault(p.iscc_id_a, {})[p.iscc_id_b] = (t.matched_a, t.coverage_a)
        threshold = b._opts.match_threshold_simprints
        checked = 0
        for iscc_id in sorted(by_asset)[:20]:
            body = codec.iscc_id_to_int(iscc_id).to_bytes(8, "big")
            simprints = [s for s, _ in a._sp_assets[CT][body]]
            n = len(simprints)
            found = table_b.search_raw(simprints, limit=300, threshold=threshold, total_assets=len(assets_b))
            others = {codec.iscc_id_from_int(int.from_bytes(r.iscc_id_body, "big"), b._realm_id or 0): r for r in found}
            assert set(others) == set(by_asset[iscc_id])
            for other, r in others.items():
                matched, coverage = by_asset[iscc_id][other]
                print(iscc_id, other, r.matches, matched, r.score, coverage)
                assert r.matches == matched
                assert abs(r.score - coverage) <= (n + 2) * 2.0**-52 * coverage, (iscc_id, other, r.score, coverage)
                checked += 1
        assert checked >= 20
    finally:
        a.close()
        b.close()
