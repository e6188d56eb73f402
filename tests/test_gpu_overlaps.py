"""
The device self-join of a simprint table into asset overlaps (``isccsearch_join_overlaps`` through ``HipTable.join_overlaps``) and
``find_shared_content`` on an MI355X.

Every case runs on both kernels -- ``forced(engine)`` (every launch on the matrix cores, ``mfma_join_kernel``) and ``valu(engine)``
(``join_scan_kernel``), the ``join_launches`` / ``join_mfma_launches`` counters saying which ran -- and compares records, chunks and
info for exact equality with the host model (``tests/overlap_model.py``) and with each other.  The shapes are those at which the two
emit paths change behaviour: 16 or 8 rows per block and 2 048 / 1 024 / 512-row slabs on the VALU kernel; 32-row groups, 64-row
steps, the 1 024-row chunk and the second block (``N_TWO_BLOCKS``) on the matrix cores.
"""

import ctypes
import errno

import numpy as np
import pytest

from iscc_search_amd import _lib
from iscc_search_amd.index import HipIndex, HipOptions
from overlap_model import ENOSPC, INFO_NAMES, chunk_keys, model_overlaps
from test_gpu_duplicates import planted, table_with
from test_gpu_join_mfma import N_TWO_BLOCKS, counters, dropping, forced, valu
from test_shared_content import CT, OverlapOracleEngine, library

pytestmark = pytest.mark.gpu

MANY = 10_000_000


def sp_table(engine, nbytes, keys, words):
    return table_with(engine, _lib.METRIC_HAMMING, 2, nbytes, keys, words, None)


def raw_call(engine, t, max_hamming, asset_keys, capacity, max_doc_freq=0, dup_limit=1000):
    """The C call itself: (rc, records, chunks, info array)."""
    asset_keys = np.ascontiguousarray(asset_keys, dtype=np.uint64)
    records = np.zeros(2 * capacity, dtype=_lib.OVERLAP_DTYPE)
    chunks = np.zeros(len(asset_keys), dtype=np.uint32)
    info = np.zeros(4, dtype=np.uint64)
    rc = engine._lib.isccsearch_join_overlaps(engine.handle, t.id, max_hamming, max_doc_freq, dup_limit, len(asset_keys), _lib.ptr(asset_keys),
                                              capacity, _lib.ptr(records) if capacity else None, _lib.ptr(chunks), _lib.ptr(info))
    return rc, records, chunks, info


def same_result(got, exp, what):
    (g_rec, g_chunks, g_info), (e_rec, e_chunks, e_info) = got, exp
    assert g_info == e_info, what
    assert g_rec.dtype == e_rec.dtype and g_rec.shape == e_rec.shape and g_rec.tobytes() == e_rec.tobytes(), what + ": records"
    assert np.array_equal(g_chunks, e_chunks), what + ": chunks"


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
        assert m1 > m0 and l1 - l0 == m1 - m0, "the forced call did not run on the matrix cores alone"
        assert m2 == m1 and l2 > l1, "the join_mfma=0 call did not run on the VALU kernel alone"
    else:
        assert (l2, m2) == (l0, m0), "a table without a pair of rows launched a join kernel"
    same_result(got, ref, "matrix cores against VALU")
    if exp is not None:
        same_result(got, exp, "matrix cores against the model")
    return got


def check(engine, t, keys, words, asset_keys, max_hamming, max_doc_freq=0, dup_limit=1000, launches=True):
    rc, rec, chunks, info = model_overlaps(keys, words, asset_keys, max_hamming, max_doc_freq, dup_limit)
    assert rc == 0
    return both_kernels(engine, lambda: t.join_overlaps(max_hamming, asset_keys, max_doc_freq, MANY, dup_limit), (rec, chunks, info), launches)


def chunked(rng, n, words):
    """n rows dealt to assets of 1-40 chunks in random row order, asset keys unrelated to the order; rows 0 and 1 (two assets) equal."""
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(int(rng.integers(1, 41)), n - sum(sizes), max(1, n // 2)))
    ids = rng.choice(np.arange(1, 10 * len(sizes) + 10, dtype=np.uint64), size=len(sizes), replace=False) * np.uint64(0x9E3779B97F4A7C15)
    assets = rng.permutation(np.repeat(ids, sizes))
    if assets[0] == assets[1]:
        other = int(np.nonzero(assets != assets[0])[0][0])
        assets[[1, other]] = assets[[other, 1]]
    words[1] = words[0]
    keys = chunk_keys(assets, offsets=rng.permutation(n))
    # most assets are listed, the planted pair's always; one listed asset has no rows
    listed = [a for i, a in enumerate(ids.tolist()) if len(ids) <= 4 or i % 7 != 3 or a in (int(assets[0]), int(assets[1]))]
    return keys, np.array(sorted(listed + [5]), dtype=np.uint64)


@pytest.mark.parametrize("n", [2, 17, 65, 1025, 2049, N_TWO_BLOCKS])
def test_simprints64(hip_engine, n):
    rng = np.random.default_rng(n)
    words = planted(rng, n, 8, pool=max(2, n // 30))
    keys, asset_keys = chunked(rng, n, words)
    with dropping(sp_table(hip_engine, 8, keys, words)) as (t,):
        for tau in (0, 5):
            _, _, info = check(hip_engine, t, keys, words[:, :1], asset_keys, tau)
            assert info["chunk_pairs"] >= 1 and info["records"] >= 2


@pytest.mark.parametrize("nbytes,tau", [(16, 7), (32, 9)])
def test_simprints128_and_256(hip_engine, nbytes, tau):
    rng = np.random.default_rng(nbytes)
    n = 3000
    words = planted(rng, n, nbytes, pool=100, flips=8)
    keys, asset_keys = chunked(rng, n, words)
    with dropping(sp_table(hip_engine, nbytes, keys, words)) as (t,):
        for max_hamming in (0, tau):
            _, _, info = check(hip_engine, t, keys, words[:, : nbytes // 8], asset_keys, max_hamming)
            assert info["chunk_pairs"] >= 1


def test_same_asset_pairs_take_no_slot(hip_engine):
    """1 025 identical rows of one asset: 524 800 row pairs within tau, none of them a chunk pair."""
    n = 1025
    words = np.full((n + 2, 1), 0x0123456789ABCDEF, dtype=np.uint64)
    words[n + 1] = 0xFEDCBA9876543210
    assets = np.array([7] * n + [9, 9], dtype=np.uint64)
    keys = chunk_keys(assets)
    with dropping(sp_table(hip_engine, 8, keys, words)) as (t,):
        for option in (forced, valu):
            with option(hip_engine):
                rc, rec, chunks, info = raw_call(hip_engine, t, 0, [7, 9], n)
                assert rc == 0 and info.tolist() == [n, 2, n + 2, 0] and chunks.tolist() == [n, 2]
                assert [tuple(int(v) for v in r) for r in rec[:2].tolist()] == [(0, 1, n, 0, 0, n), (1, 0, 1, 0, 0, n)]
                rc, rec, chunks, info = raw_call(hip_engine, t, 0, [7, 9], n - 1)
                assert rc == -errno.ENOSPC and int(info[0]) == n
                # without the second asset nothing takes a slot: capacity 0 is enough
                rc, rec, chunks, info = raw_call(hip_engine, t, 0, [7], 0)
                assert rc == 0 and info.tolist() == [0, 0, n, 0] and chunks.tolist() == [n]
        check(hip_engine, t, keys, words, np.array([7, 9], dtype=np.uint64), 0)


def test_every_pair_takes_a_slot(hip_engine):
    """
    300 identical rows of 300 listed assets, one chunk each: every candidate of the emit path takes a slot (the dense cases above are
    dense in pairs that take none).  The ring fills within a step and every lane takes many slots, so the count pass and the write
    pass have to agree on every one of the 44 850 chunk pairs.
    """
    n = 300
    words = np.full((n, 1), 0x0123456789ABCDEF, dtype=np.uint64)
    asset_keys = np.arange(1, n + 1, dtype=np.uint64)
    keys = chunk_keys(asset_keys)
    with dropping(sp_table(hip_engine, 8, keys, words)) as (t,):
        rec, chunks, info = check(hip_engine, t, keys, words, asset_keys, 0)
        assert info["chunk_pairs"] == n * (n - 1) // 2 == 44_850 and info["records"] == len(rec) == n * (n - 1) == 89_700
        assert bool(np.all(rec["matched"] == 1)) and bool(np.all(rec["sum_hamming"] == 0)) and bool(np.all(rec["chunk_pairs"] == 1))
        assert chunks.tolist() == [1] * n


def test_stop_chunks(hip_engine):
    rng = np.random.default_rng(50)
    boiler = np.uint64(0x5555AAAA3333CCCC)
    assets, codes = [], []
    for a in range(1, 61):                       # 60 assets of 5-12 ordinary chunks; the first 50 hold the boilerplate chunk too
        k = int(rng.integers(5, 13))
        assets += [a] * k
        codes += rng.integers(0, 2**64, size=k, dtype=np.uint64).tolist()
        if a <= 50:
            assets.append(a)
            codes.append(int(boiler))
    order = rng.permutation(len(assets))
    keys = chunk_keys(np.array(assets, dtype=np.uint64)[order], offsets=rng.permutation(len(assets)))
    words = np.array(codes, dtype=np.uint64)[order][:, None]
    # two ordinary chunks shared by assets 55 and 56, so that something pairs whatever the cut
    i55, i56 = int(np.nonzero(keys[:, 0] == 55)[0][0]), int(np.nonzero(keys[:, 0] == 56)[0][0])
    words[i56] = words[i55]
    asset_keys = np.arange(1, 61, dtype=np.uint64)
    with dropping(sp_table(hip_engine, 8, keys, words)) as (t,):
        builds = hip_engine.stats()["freq_builds"]
        _, _, info = check(hip_engine, t, keys, words, asset_keys, 0, max_doc_freq=0)
        assert info["records"] == 50 * 49 + 2 and info["stop_chunks"] == 0
        assert hip_engine.stats()["freq_builds"] == builds, "max_doc_freq 0 built the frequency column"
        _, _, info = check(hip_engine, t, keys, words, asset_keys, 0, max_doc_freq=49)
        assert info["records"] == 2 and info["chunk_pairs"] == 1 and info["stop_chunks"] == 50
        assert hip_engine.stats()["freq_builds"] == builds + 1
        rec, _, info = check(hip_engine, t, keys, words, asset_keys, 0, max_doc_freq=50)
        assert info["records"] == 50 * 49 + 2 and info["stop_chunks"] == 0 and info["chunk_pairs"] == 50 * 49 // 2 + 1
        # a column counted over fewer rows: with dup_limit 20 the boilerplate chunk has frequency 20
        _, _, info = check(hip_engine, t, keys, words, asset_keys, 0, max_doc_freq=19, dup_limit=20)
        assert info["stop_chunks"] == 50
        _, _, info = check(hip_engine, t, keys, words, asset_keys, 0, max_doc_freq=20, dup_limit=20)
        assert info["stop_chunks"] == 0


def test_the_smallest_distance(hip_engine):
    s = 0x00FF00FF0F0F3355
    flip = lambda *bits: s ^ sum(1 << b for b in bits)
    cands = [flip(1, 2, 3, 4, 5), flip(6, 7), flip(8, 9)]       # 5, 2, 2 bits off s
    tuples = lambda rec: [tuple(int(r[f]) for f in ("src", "dst", "matched", "sum_hamming", "chunk_pairs")) for r in rec]
    keys = chunk_keys([1, 2, 2, 2])
    words = np.array([[s]] + [[c] for c in cands], dtype=np.uint64)
    with dropping(sp_table(hip_engine, 8, keys, words)) as (t,):
        rec, chunks, info = check(hip_engine, t, keys, words, np.array([1, 2], dtype=np.uint64), 5)
        assert tuples(rec) == [(0, 1, 1, 2, 3), (1, 0, 3, 9, 3)] and chunks.tolist() == [1, 3]
    keys = chunk_keys([1, 2, 2, 3])
    with dropping(sp_table(hip_engine, 8, keys, words)) as (t,):
        rec, chunks, info = check(hip_engine, t, keys, words, np.array([1, 2, 3], dtype=np.uint64), 5)
        assert tuples(rec) == [(0, 1, 1, 2, 2), (0, 2, 1, 2, 1), (1, 0, 2, 7, 2), (1, 2, 1, 4, 1), (2, 0, 1, 2, 1), (2, 1, 1, 4, 1)]


def test_capacity_is_exact_on_both_kernels(hip_engine):
    rng = np.random.default_rng(9)
    n = 1500
    words = planted(rng, n, 8, pool=30)
    keys, asset_keys = chunked(rng, n, words)
    rc, exp_rec, exp_chunks, exp_info = model_overlaps(keys, words[:, :1], asset_keys, 3)
    total = exp_info["chunk_pairs"]
    assert total > 100
    assert model_overlaps(keys, words[:, :1], asset_keys, 3, capacity=total - 1)[0] == ENOSPC
    with dropping(sp_table(hip_engine, 8, keys, words)) as (t,):
        for option in (forced, valu):
            with option(hip_engine):
                rc, _, _, info = raw_call(hip_engine, t, 3, asset_keys, total - 1)
                assert rc == -errno.ENOSPC and int(info[0]) == total
                assert "capacity" in hip_engine._lib.isccsearch_last_error().decode()
                rc, _, _, info = raw_call(hip_engine, t, 3, asset_keys, 0)
                assert rc == -errno.ENOSPC and int(info[0]) == total
                rc, rec, chunks, info = raw_call(hip_engine, t, 3, asset_keys, total)
                assert rc == 0
                same_result((rec[: int(info[1])], chunks, dict(zip(INFO_NAMES, info.tolist()))), (exp_rec, exp_chunks, exp_info), "capacity == total")
        with pytest.raises(ValueError, match="exceed max_pairs"):
            t.join_overlaps(3, asset_keys, 0, total - 1)
        assert t.join_overlaps(3, asset_keys, 0, total)[2] == exp_info


def test_rows_behind_a_segments_end(hip_engine):
    rng = np.random.default_rng(2)
    n = 3000
    words = planted(rng, n, 8, pool=60)
    keys, asset_keys = chunked(rng, n, words)
    with dropping(sp_table(hip_engine, 8, keys, words)) as (t,):
        gone = rng.choice(np.arange(2, n), size=700, replace=False)
        assert t.remove(keys[gone]) == 700
        keep = np.setdiff1d(np.arange(n), gone)
        _, _, info = check(hip_engine, t, keys[keep], words[keep, :1], asset_keys, 4)
        assert info["chunk_pairs"] > 0 and info["live_rows"] <= len(keep)
        t.remove(keys[keep[1:]])
        rec, chunks, info = check(hip_engine, t, keys[:1], words[:1, :1], asset_keys, 64, launches=False)       # one row: nothing launched
        assert len(rec) == 0 and info == {"chunk_pairs": 0, "records": 0, "live_rows": 1, "stop_chunks": 0} and int(chunks.sum()) == 1
        t.remove(keys[:1])
        rec, chunks, info = check(hip_engine, t, keys[:0], words[:0, :1], asset_keys, 64, launches=False)       # empty
        assert len(rec) == 0 and info == {"chunk_pairs": 0, "records": 0, "live_rows": 0, "stop_chunks": 0} and int(chunks.sum()) == 0


def test_refused_arguments_leave_the_outputs_untouched(hip_engine):
    keys = chunk_keys([1, 2, 3])
    words = np.array([[5], [5], [6]], dtype=np.uint64)
    call = hip_engine._lib.isccsearch_join_overlaps
    last_error = lambda: hip_engine._lib.isccsearch_last_error().decode()
    with dropping(sp_table(hip_engine, 8, keys, words), hip_engine.open_table(_lib.METRIC_HAMMING, 1, 8),
                  hip_engine.open_table(_lib.METRIC_NPHD, 1, 32)) as (t, t_kw1, t_nphd):
        t_kw1.add(np.array([1, 2], dtype=np.uint64), words[:2])
        good = np.array([1, 2, 3], dtype=np.uint64)
        records = np.full(8, 0xEE, dtype=np.uint8).repeat(32).view(_lib.OVERLAP_DTYPE)
        chunks = np.full(3, 0xEEEEEEEE, dtype=np.uint32)
        info = np.full(4, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
        P = _lib.ptr
        h = hip_engine.handle
        base = dict(h=h, table=t.id, max_hamming=0, max_doc_freq=0, dup_limit=1000, n_assets=3, asset_keys=P(good), capacity=4,
                    out_pairs=P(records), out_chunks=P(chunks), out_info=P(info))
        unsorted, repeated = np.array([1, 3, 2], dtype=np.uint64), np.array([1, 2, 2], dtype=np.uint64)
        cases = [
            (dict(h=None), -errno.EINVAL, "handle"),
            (dict(asset_keys=None), -errno.EINVAL, "NULL"),
            (dict(out_chunks=None), -errno.EINVAL, "NULL"),
            (dict(out_info=None), -errno.EINVAL, "NULL"),
            (dict(out_pairs=None), -errno.EINVAL, "out_pairs"),
            (dict(table=t_kw1.id), -errno.EINVAL, "key_words"),
            (dict(table=t_nphd.id), -errno.EINVAL, "HAMMING"),
            (dict(n_assets=0), -errno.EINVAL, "n_assets"),
            (dict(n_assets=0xFFFFFFFF), -errno.EINVAL, "n_assets"),
            (dict(asset_keys=P(unsorted)), -errno.EINVAL, "asset_keys[2]"),
            (dict(asset_keys=P(repeated)), -errno.EINVAL, "asset_keys[2]"),
            (dict(max_hamming=-1), -errno.EINVAL, "max_hamming"),
            (dict(max_doc_freq=11, dup_limit=10), -errno.EINVAL, "dup_limit"),
            (dict(capacity=1 << 31), -errno.E2BIG, "32 bits"),
        ]
        before = counters(hip_engine)
        for change, want, word in cases:
            args = dict(base, **change)
            rc = call(*args.values())
            assert rc == want and word in last_error(), (change, rc, last_error())
            assert bool(np.all(records.view(np.uint8) == 0xEE)) and bool(np.all(chunks == 0xEEEEEEEE)) and bool(np.all(info == 0xEEEEEEEEEEEEEEEE)), change
        assert counters(hip_engine) == before
        with pytest.raises(ValueError, match="ascending"):
            t.join_overlaps(0, unsorted, 0, 10)
        # what is allowed: out_pairs NULL with capacity 0 (here -ENOSPC: one chunk pair), max_doc_freq == dup_limit
        assert call(*dict(base, capacity=0, out_pairs=None).values()) == -errno.ENOSPC and int(info[0]) == 1
        assert call(*dict(base, max_doc_freq=10, dup_limit=10).values()) == 0 and info.tolist() == [1, 2, 3, 0] and chunks.tolist() == [1, 1, 1]


def test_default_dispatch_small_table_stays_on_the_valu_kernel(hip_engine):
    rng = np.random.default_rng(22)
    n = 5000
    words = planted(rng, n, 8, pool=100)
    keys, asset_keys = chunked(rng, n, words)
    with dropping(sp_table(hip_engine, 8, keys, words)) as (t,):
        l0, m0 = counters(hip_engine)
        with hip_engine.options(mfma=1, join_mfma=1):
            got = t.join_overlaps(5, asset_keys, 0, MANY)
        l1, m1 = counters(hip_engine)
        assert m1 == m0 and l1 == l0 + 1
        rc, rec, chunks, info = model_overlaps(keys, words[:, :1], asset_keys, 5)
        same_result(got, (rec, chunks, info), "default dispatch against the model")


def test_find_shared_content_end_to_end(hip_engine):
    """About 300 assets and 3 000 chunks of one type: the device result equals the model-backed one, and -- for 20 assets -- what a
    simprint search by the asset's own chunks lists: ``search_raw`` asks for limit x oversampling = 6 000 > MAX_K neighbours, i.e. every
    row within the radius (the table has fewer than 4 096 rows: no list fills the cap); under constant IDF its score of asset B is the
    mean over A's n chunks of the best similarity found in B -- ``coverage_a``, summed in another order: relative (n + 2) * 2^-52."""
    assets = library(np.random.default_rng(31), 300, chunks=(4, 14))
    cpu = HipIndex(OverlapOracleEngine(), HipOptions())
    cpu.add_assets(assets)
    exp = cpu.find_shared_content(max_doc_freq=0)
    idx = HipIndex(hip_engine, HipOptions())
    try:
        idx.add_assets(assets)
        table = idx._sp_tables[CT]
        assert 2500 < table.size < _lib.MAX_K
        _, m0 = counters(hip_engine)
        with forced(hip_engine):
            got = idx.find_shared_content(max_doc_freq=0)
        _, m1 = counters(hip_engine)
        with valu(hip_engine):
            ref = idx.find_shared_content(max_doc_freq=0)
        assert m1 > m0 and counters(hip_engine)[1] == m1
        assert len(got) > 100 and got == exp and ref == exp
        assert idx.find_shared_content(min_chunks=2, min_coverage=0.2, max_doc_freq=5) == cpu.find_shared_content(min_chunks=2, min_coverage=0.2, max_doc_freq=5)
        by_asset = {}
        for p in got:
            t = p.types[CT]
            by_asset.setdefault(p.iscc_id_a, {})[p.iscc_id_b] = (t.matched_a, t.coverage_a)
            by_asset.setdefault(p.iscc_id_b, {})[p.iscc_id_a] = (t.matched_b, t.coverage_b)
        from iscc_search_amd import codec

        threshold = idx._opts.match_threshold_simprints
        checked = 0
        for iscc_id in sorted(by_asset)[:20]:
            body = codec.iscc_id_to_int(iscc_id).to_bytes(8, "big")
            simprints = [s for s, _ in idx._sp_assets[CT][body]]
            n = len(simprints)
            found = {r.iscc_id_body: r for r in table.search_raw(simprints, limit=300, threshold=threshold, total_assets=len(assets))}
            assert found.pop(body).matches == n                     # the asset itself
            others = {codec.iscc_id_from_int(int.from_bytes(b, "big"), idx._realm_id or 0): r for b, r in found.items()}
            assert set(others) == set(by_asset[iscc_id])
            for other, r in others.items():
                matched, coverage = by_asset[iscc_id][other]
                assert r.matches == matched
                assert abs(r.score - coverage) <= (n + 2) * 2.0**-52 * coverage, (iscc_id, other, r.score, coverage)
                checked += 1
        assert checked >= 20
    finally:
        idx.close()
