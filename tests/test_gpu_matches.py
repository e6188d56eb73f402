"""
The device cross join (``isccsearch_join_between`` through ``HipTable.join_between``) and ``find_matches`` on an MI355X.

Kernel results are compared for exact equality (keys and their sides, distances, prefix bits, order) with a numpy brute force
over all A x B row pairs; a 1 Mi-row table against the union of the existing range-limited scans; ``find_matches`` against
``search_assets`` per asset.
"""

import ctypes
import errno

import numpy as np
import pytest

from iscc_search_amd import _lib
from test_gpu_duplicates import mask_lengths, planted, prefix_masks, table_with
from test_matches import as_dict, definition, int_keys, split_pool

pytestmark = pytest.mark.gpu

TILE_W1 = 16     # rows of the SGPR side per block of the 64-bit kernel (join.hip.h JoinCfg<1>::TQ)
TILE_WN = 8      # ... of the kernels for longer codes (JoinCfg<W>::TQ, W > 1)
# rows per streamed slab: BLOCK * 2 * U (join.hip.h JoinCfg<W>::SLAB), BLOCK = 256 (scan_params.hip.h), U = 4, 2, 1, 1 for
# W = 1, 2, 3, 4 (valu_scan_kernel.hip.h TileCfg<W>::U)
SLAB_W1, SLAB_W2, SLAB_W3, SLAB_W4 = 2048, 1024, 512, 512


def sort_by_key(keys, words, nb):
    order = np.lexsort(keys.T[::-1]) if keys.ndim == 2 else np.argsort(keys)
    return keys[order], words[order], nb[order].astype(np.int64)


def np_join_between(side_a, side_b, mh):
    """All pairs (row of A, row of B) within mh[min(len_a, len_b)] bits over the common prefix: keys_a from A, sorted by (key_a, key_b)."""
    ka, wa, na = sort_by_key(*side_a)
    kb, wb, nb = sort_by_key(*side_b)
    mh = np.asarray(mh, dtype=np.int64)
    masks = prefix_masks()
    W = min(wa.shape[1], wb.shape[1])       # (words past the shorter table's width are never inside a common prefix)
    out_i, out_j, out_h, out_p = [], [], [], []
    for i0 in range(0, len(na), 128):
        i1 = min(i0 + 128, len(na))
        p = np.minimum(na[i0:i1, None], nb[None, :])
        h = np.zeros(p.shape, dtype=np.int64)
        for w in range(W):
            h += np.bitwise_count((wa[i0:i1, None, w] ^ wb[None, :, w]) & masks[p, w]).astype(np.int64)
        ii, jj = np.nonzero(h <= mh[p])     # row-major: already ordered by (i, j)
        out_i.append(ii + i0)
        out_j.append(jj)
        out_h.append(h[ii, jj])
        out_p.append(8 * p[ii, jj])
    if not out_i:
        return ka[:0], kb[:0], np.zeros(0, np.uint32), np.zeros(0, np.uint16)
    ii, jj = np.concatenate(out_i), np.concatenate(out_j)
    return ka[ii], kb[jj], np.concatenate(out_h).astype(np.uint32), np.concatenate(out_p).astype(np.uint16)


def check(table_a, table_b, side_a, side_b, mh):
    got = table_a.join_between(table_b, mh, 10_000_000)
    exp = np_join_between(side_a, side_b, mh)
    for g, e, name in zip(got, exp, ("keys_a", "keys_b", "hamming", "prefix_bits")):
        assert g.shape == e.shape and np.array_equal(g, e), name
    return len(exp[2])


def only(nbytes, tau):
    mh = np.full(33, -1, dtype=np.int16)
    mh[nbytes] = tau
    return mh


def two_sides(rng, n_a, n_b, nbytes, pool, flips=6):
    """Codes of both tables off ONE pool of base codes, so near-copies land on both sides."""
    words = planted(rng, n_a + n_b, nbytes, pool=pool, flips=flips)
    return words[:n_a], words[n_a:]


@pytest.mark.parametrize("n_a,n_b", [
    (1, 1), (TILE_W1 - 1, SLAB_W1 + 1), (SLAB_W1 + 1, TILE_W1 - 1), (TILE_W1, SLAB_W1), (SLAB_W1, TILE_W1),
    (TILE_W1 + 1, SLAB_W1 - 1), (SLAB_W1 + 1, SLAB_W1 + 1), (5000, 300),
])
def test_hamming64_against_numpy(hip_engine, n_a, n_b):
    """The larger table goes into SGPRs: table A is that side for n_a >= n_b and the streamed side otherwise."""
    rng = np.random.default_rng(1000 * n_a + n_b)
    wa, wb = two_sides(rng, n_a, n_b, 8, pool=max(2, (n_a + n_b) // 60))
    # keys in no row order; every third key of the smaller table also occurs in the other
    keys = rng.permutation(np.arange(1, n_a + n_b + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    ka, kb = keys[:n_a].copy(), keys[n_a:].copy()
    shared = np.arange(0, min(n_a, n_b), 3)
    kb[shared] = ka[shared]
    side_a = (ka, wa, np.full(n_a, 8, dtype=np.uint8))
    side_b = (kb, wb, np.full(n_b, 8, dtype=np.uint8))
    ta = table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, *side_a)
    tb = table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, *side_b)
    try:
        total = 0
        for tau in (0, 5, 64) if n_a * n_b <= 150_000 else (0, 5):      # (64: every pair, n_a * n_b of them)
            found = check(ta, tb, side_a, side_b, only(8, tau))
            assert tau != 64 or found == n_a * n_b
            total += found
        assert total > 0
        assert check(ta, tb, side_a, side_b, np.full(33, -1, dtype=np.int16)) == 0
    finally:
        ta.drop()
        tb.drop()


def test_hamming128_two_word_keys(hip_engine):
    rng = np.random.default_rng(5)
    n_a, n_b = 3003, 2001
    assert n_a % TILE_WN and n_b % SLAB_W2          # a partial last tile (of A, the larger side) and a partial last slab
    wa, wb = two_sides(rng, n_a, n_b, 16, pool=200)
    ka = np.stack([rng.integers(0, 4, size=n_a, dtype=np.uint64), rng.permutation(n_a).astype(np.uint64)], axis=1)
    # B's low words lie past A's, so the 50 keys taken over from A collide with no other key of B
    kb = np.stack([rng.integers(0, 4, size=n_b, dtype=np.uint64), rng.permutation(n_b).astype(np.uint64) + np.uint64(n_a)], axis=1)
    kb[:50] = ka[:50]
    assert len(np.unique(kb, axis=0)) == n_b
    side_a = (ka, wa, np.full(n_a, 16, dtype=np.uint8))
    side_b = (kb, wb, np.full(n_b, 16, dtype=np.uint8))
    ta = table_with(hip_engine, _lib.METRIC_HAMMING, 2, 16, *side_a)
    tb = table_with(hip_engine, _lib.METRIC_HAMMING, 2, 16, *side_b)
    try:
        assert check(ta, tb, side_a, side_b, only(16, 7)) > 0
        assert check(tb, ta, side_b, side_a, only(16, 7)) > 0
    finally:
        ta.drop()
        tb.drop()


def nphd_sides(rng, n_a, n_b):
    """Table A holds lengths {8, 12, 16, 32} (max 32 bytes), table B {8, 16, 24, 32}: la > lb, la < lb, a length that is no
    multiple of 8 and lengths only one side has."""
    wa, wb = two_sides(rng, n_a, n_b, 32, pool=150, flips=8)
    na = rng.choice([8, 12, 16, 32], size=n_a).astype(np.uint8)
    nb = rng.choice([8, 16, 24, 32], size=n_b).astype(np.uint8)
    ka = rng.permutation(n_a).astype(np.uint64) + np.uint64(10)
    kb = rng.permutation(n_b).astype(np.uint64) + np.uint64(10 + n_a // 2)         # half of B's keys occur in A
    return (ka, mask_lengths(wa, na), na), (kb, mask_lengths(wb, nb), nb)


@pytest.mark.parametrize("tau", [0, "p"])
def test_nphd_mixed_lengths_across_tables(hip_engine, tau):
    rng = np.random.default_rng(11)
    side_a, side_b = nphd_sides(rng, 4000, 3000)
    ta = table_with(hip_engine, _lib.METRIC_NPHD, 1, 32, *side_a)
    tb = table_with(hip_engine, _lib.METRIC_NPHD, 1, 32, *side_b)
    try:
        mh = np.full(33, -1, dtype=np.int16)
        for p in range(1, 33):
            mh[p] = 0 if tau == 0 else p
        assert check(ta, tb, side_a, side_b, mh) > 0
        if tau == "p":
            # pairs of every common prefix are among them: (12, 24) compares 12 bytes, (32, 8) compares 8
            assert {8 * 8, 8 * 12, 8 * 16, 8 * 32} <= set(ta.join_between(tb, mh, 10_000_000)[3].tolist())
    finally:
        ta.drop()
        tb.drop()


def test_nphd_every_pair_and_different_max_bytes(hip_engine):
    rng = np.random.default_rng(12)
    side_a, side_b = nphd_sides(rng, 300, 400)
    ta = table_with(hip_engine, _lib.METRIC_NPHD, 1, 32, *side_a)
    # NPHD tables of different max_bytes join: B's rows are cut to at most 24 bytes in a table that holds no more
    nb = np.minimum(side_b[2], 24).astype(np.uint8)
    side_b = (side_b[0], mask_lengths(side_b[1], nb), nb)
    tb = table_with(hip_engine, _lib.METRIC_NPHD, 1, 24, *side_b)
    try:
        mh = np.array([-1] + [8 * p for p in range(1, 33)], dtype=np.int16)
        assert check(ta, tb, side_a, side_b, mh) == 300 * 400
        assert check(tb, ta, side_b, side_a, mh) == 300 * 400
    finally:
        ta.drop()
        tb.drop()


def test_after_remove_and_empty_tables(hip_engine):
    rng = np.random.default_rng(2)
    n_a, n_b = 3000, 2500
    wa, wb = two_sides(rng, n_a, n_b, 8, pool=60)
    side_a = (np.arange(1, n_a + 1, dtype=np.uint64), wa, np.full(n_a, 8, dtype=np.uint8))
    side_b = (np.arange(1001, n_b + 1001, dtype=np.uint64), wb, np.full(n_b, 8, dtype=np.uint8))
    mh = only(8, 4)
    ta = table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, *side_a)
    tb = table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, *side_b)
    try:
        gone = rng.choice(n_a, size=700, replace=False)
        assert ta.remove(side_a[0][gone]) == 700
        keep = np.setdiff1d(np.arange(n_a), gone)
        side_a = tuple(x[keep] for x in side_a)
        assert check(ta, tb, side_a, side_b, mh) > 0
        gone = rng.choice(n_b, size=1900, replace=False)              # B becomes the smaller (streamed) side
        assert tb.remove(side_b[0][gone]) == 1900
        keep = np.setdiff1d(np.arange(n_b), gone)
        side_b = tuple(x[keep] for x in side_b)
        assert check(ta, tb, side_a, side_b, mh) > 0
        tb.remove(side_b[0])
        assert [len(a) for a in ta.join_between(tb, mh, 10)] == [0, 0, 0, 0]
        assert [len(a) for a in tb.join_between(ta, mh, 10)] == [0, 0, 0, 0]
    finally:
        ta.drop()
        tb.drop()


def test_capacity_retry(hip_engine):
    rng = np.random.default_rng(9)
    n_a, n_b = 2000, 1500
    wa, wb = two_sides(rng, n_a, n_b, 8, pool=20)
    ta = table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, np.arange(1, n_a + 1, dtype=np.uint64), wa, None)
    tb = table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, np.arange(1, n_b + 1, dtype=np.uint64), wb, None)
    try:
        mh = only(8, 3)
        full = ta.join_between(tb, mh, 10_000_000)
        total = len(full[2])
        assert total > 100
        call = hip_engine._lib.isccsearch_join_between
        cap = total // 3
        out = [np.empty(cap, np.uint64), np.empty(cap, np.uint64), np.empty(cap, np.uint32), np.empty(cap, np.uint16)]
        got_total = ctypes.c_uint64()
        rc = call(hip_engine.handle, ta.id, tb.id, _lib.ptr(mh), cap, *(_lib.ptr(a) for a in out), ctypes.byref(got_total))
        assert rc == -errno.ENOSPC and got_total.value == total
        out = [np.empty(total, np.uint64), np.empty(total, np.uint64), np.empty(total, np.uint32), np.empty(total, np.uint16)]
        rc = call(hip_engine.handle, ta.id, tb.id, _lib.ptr(mh), total, *(_lib.ptr(a) for a in out), ctypes.byref(got_total))
        assert rc == 0 and got_total.value == total
        for g, e in zip(out, full):
            assert np.array_equal(g, e)
        with pytest.raises(ValueError, match=f"{total} pairs exceed max_pairs"):
            ta.join_between(tb, mh, total - 1)
    finally:
        ta.drop()
        tb.drop()


def test_invalid_arguments(hip_engine):
    one = (np.array([1], dtype=np.uint64), np.zeros((1, 4), dtype=np.uint64))
    ham8 = table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, *one, None)
    ham16 = table_with(hip_engine, _lib.METRIC_HAMMING, 1, 16, *one, None)
    ham8_kw2 = table_with(hip_engine, _lib.METRIC_HAMMING, 2, 8, np.array([[0, 1]], dtype=np.uint64), one[1], None)
    nphd8 = table_with(hip_engine, _lib.METRIC_NPHD, 1, 8, *one, np.array([8], dtype=np.uint8))
    try:
        mh = only(8, 3)
        out = [np.empty(4, np.uint64), np.empty(4, np.uint64), np.empty(4, np.uint32), np.empty(4, np.uint16)]
        total = ctypes.c_uint64()

        def rc(a, b):
            return hip_engine._lib.isccsearch_join_between(hip_engine.handle, a.id, b.id, _lib.ptr(mh), 4, *(_lib.ptr(x) for x in out), ctypes.byref(total))

        assert rc(ham8, ham8) == -errno.EINVAL and "isccsearch_join_within" in _lib.last_error()
        assert rc(ham8, nphd8) == -errno.EINVAL and "metric" in _lib.last_error()
        assert rc(ham8, ham8_kw2) == -errno.EINVAL and "key_words" in _lib.last_error()
        assert rc(ham8, ham16) == -errno.EINVAL and "lengths" in _lib.last_error()
        with pytest.raises(ValueError, match="isccsearch_join_within"):
            ham8.join_between(ham8, mh, 10)
    finally:
        for t in (ham8, ham16, ham8_kw2, nphd8):
            t.drop()


def test_million_rows_against_range_scans(hip_engine):
    """2^20 synthetic 64-bit rows against 3 000 near-copies of some of them: the pairs are the union of search_within over the copies."""
    rng = np.random.default_rng(21)
    n, m, tau = 1 << 20, 3000, 3
    ta = hip_engine.open_table(_lib.METRIC_HAMMING, 1, 8)
    tb = hip_engine.open_table(_lib.METRIC_HAMMING, 1, 8)
    try:
        ta.add_synthetic(8, n, seed=77, first_row=0, key_base=1)
        _, cols = ta.export_rows(8, 0, n)
        copies = cols[0, rng.integers(0, n, size=m)].copy()
        for b in range(3):
            copies ^= np.left_shift(np.uint64(1), rng.integers(0, 64, size=m).astype(np.uint64)) * (rng.random(m) < 0.7)
        kb = rng.permutation(np.arange(1, 2 * m + 1, dtype=np.uint64))[:m]       # B's keys: no order, many of them keys of A too
        tb.add(kb, copies[:, None])
        mh = only(8, tau)
        qk, qh, _, qc = ta.search_within(copies[:, None], None, 64, tau)
        assert int(qc.max()) < 64                 # (no list was cut)
        exp = sorted((int(k), int(kb[i]), int(h)) for i in range(m) for k, h in zip(qk[i, : qc[i]].tolist(), qh[i, : qc[i]].tolist()))
        assert len(exp) >= m
        ka_, kb_, ham, pb = ta.join_between(tb, mh, 1_000_000)           # table A in SGPRs
        assert list(zip(ka_.tolist(), kb_.tolist(), ham.tolist())) == exp
        assert np.all(pb == 64)
        kb_, ka_, ham, pb = tb.join_between(ta, mh, 1_000_000)           # table A (here: tb) streamed
        assert sorted(zip(ka_.tolist(), kb_.tolist(), ham.tolist())) == exp
        assert list(zip(kb_.tolist(), ka_.tolist())) == sorted(zip(kb_.tolist(), ka_.tolist()))
    finally:
        ta.drop()
        tb.drop()


def test_find_matches_end_to_end(hip_engine):
    a, b, _ = split_pool(hip_engine, np.random.default_rng(17), 2000, 20)
    try:
        got = a.find_matches(b)
        assert len(got) > 100
        assert as_dict(got) == definition(a, b)
        assert sum(m.iscc_id_a == m.iscc_id_b for m in got) >= 20
        keys = int_keys(got)
        assert [(-m.score, k) for m, k in zip(got, keys)] == sorted((-m.score, k) for m, k in zip(got, keys))
        assert a.find_matches(b, min_score=0.95) == [m for m in got if m.score >= 0.95]
    finally:
        a.close()
        b.close()
