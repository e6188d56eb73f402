"""
The device self-join (``isccsearch_join_within`` through ``HipTable.join_within``) and ``find_duplicates`` on an MI355X.

Kernel results are compared for exact equality (keys, distances, prefix bits, order) with a numpy brute force over all row
pairs; a 1 M-row table against the union of the existing range-limited scans; ``find_duplicates`` against ``search_assets``
per asset.
"""

import ctypes
import errno

import numpy as np
import pytest

from iscc_search_amd import _lib, codec
from iscc_search_amd.index import HipIndex, HipOptions
from test_duplicates import build_assets, definition

pytestmark = pytest.mark.gpu

TILE_W1 = 16     # A rows per block of the 64-bit kernel (join.hip.h JoinCfg<1>::TQ)
SLAB_W1 = 2048   # rows per streamed slab of the 64-bit kernel


def prefix_masks():
    m = np.zeros((33, 4), dtype=np.uint64)
    for p in range(1, 33):
        for w in range(4):
            nbytes = min(max(p - 8 * w, 0), 8)
            m[p, w] = np.uint64(((1 << (8 * nbytes)) - 1) << (8 * (8 - nbytes))) if nbytes else np.uint64(0)
    return m


def np_join(keys, words, nb, mh):
    """All pairs (key_a < key_b) within mh[min(len_a, len_b)] bits over the common prefix, sorted by (key_a, key_b)."""
    n = len(nb)
    kw = 2 if keys.ndim == 2 else 1
    order = np.lexsort(keys.T[::-1]) if kw == 2 else np.argsort(keys)
    keys, words, nb = keys[order], words[order], nb[order].astype(np.int64)
    masks = prefix_masks()
    W = words.shape[1]
    out_i, out_j, out_h, out_p = [], [], [], []
    for i0 in range(0, n, 128):
        i1 = min(i0 + 128, n)
        p = np.minimum(nb[i0:i1, None], nb[None, :])
        h = np.zeros(p.shape, dtype=np.int64)
        for w in range(W):
            x = (words[i0:i1, None, w] ^ words[None, :, w]) & masks[p, w]
            h += np.bitwise_count(x).astype(np.int64)
        ii, jj = np.nonzero((h <= mh[p]) & (np.arange(n)[None, :] > np.arange(i0, i1)[:, None]))
        out_i.append(ii + i0)
        out_j.append(jj)
        out_h.append(h[ii, jj])
        out_p.append(8 * p[ii, jj])
    ii, jj = np.concatenate(out_i), np.concatenate(out_j)
    srt = np.lexsort((jj, ii))
    return keys[ii[srt]], keys[jj[srt]], np.concatenate(out_h)[srt].astype(np.uint32), np.concatenate(out_p)[srt].astype(np.uint16)


def planted(rng, n, nbytes, pool=None, flips=6):
    """Codes of nbytes bytes (words zero past the code), most of them a few bits off a small pool: many pairs at every distance."""
    W = (nbytes + 7) // 8
    pool = pool if pool is not None else max(8, n // 40)
    base = rng.integers(0, 2**64, size=(pool, 4), dtype=np.uint64)
    words = base[rng.integers(0, pool, size=n)].copy()
    for _ in range(flips):
        w = rng.integers(0, W, size=n)
        bit = rng.integers(0, 64, size=n).astype(np.uint64)
        words[np.arange(n), w] ^= np.left_shift(np.uint64(1), bit) * (rng.random(n) < 0.7)
    words[:, W:] = 0
    return words


def mask_lengths(words, nb):
    m = prefix_masks()
    return words & m[nb.astype(np.int64)]


def check(table, keys, words, nb, mh):
    got = table.join_within(mh, 10_000_000)
    exp = np_join(keys, words, nb, np.asarray(mh, dtype=np.int64))
    for g, e, name in zip(got, exp, ("keys_a", "keys_b", "hamming", "prefix_bits")):
        assert g.shape == e.shape and np.array_equal(g, e), name
    return len(exp[2])


def table_with(hip_engine, metric, kw, max_bytes, keys, words, nb):
    t = hip_engine.open_table(metric, kw, max_bytes)
    t.add(keys, words[:, : t.max_words], nb if metric == _lib.METRIC_NPHD else None)
    return t


@pytest.mark.parametrize("n", [TILE_W1 - 1, TILE_W1, TILE_W1 + 1, SLAB_W1 - 1, SLAB_W1, SLAB_W1 + 1, 5000])
def test_hamming64_against_numpy(hip_engine, n):
    rng = np.random.default_rng(n)
    words = planted(rng, n, 8, pool=max(2, n // 30))
    keys = rng.permutation(np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    nb = np.full(n, 8, dtype=np.uint8)
    t = table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, keys, words, nb)
    try:
        total = 0
        for tau in (0, 5, 64) if n <= SLAB_W1 + 1 else (0, 5):      # (64: every pair, n(n-1)/2 of them)
            mh = np.full(33, -1, dtype=np.int16)
            mh[8] = tau
            total += check(t, keys, words, nb, mh)
        assert total > 0
        assert check(t, keys, words, nb, np.full(33, -1, dtype=np.int16)) == 0
    finally:
        t.drop()


def test_hamming128_two_word_keys(hip_engine):
    rng = np.random.default_rng(5)
    n = 6000
    words = planted(rng, n, 16, pool=200)
    keys = np.stack([rng.integers(0, 4, size=n, dtype=np.uint64), rng.permutation(n).astype(np.uint64)], axis=1)
    nb = np.full(n, 16, dtype=np.uint8)
    t = table_with(hip_engine, _lib.METRIC_HAMMING, 2, 16, keys, words, nb)
    try:
        mh = np.full(33, -1, dtype=np.int16)
        mh[16] = 7
        assert check(t, keys, words, nb, mh) > 0
    finally:
        t.drop()


@pytest.mark.parametrize("tau", [0, "mid", "full"])
def test_nphd_mixed_lengths_across_segments(hip_engine, tau):
    rng = np.random.default_rng(11)
    n = 8000
    nb = rng.choice([8, 16, 24, 32, 12], size=n).astype(np.uint8)
    words = mask_lengths(planted(rng, n, 32, pool=150, flips=8), nb)
    keys = rng.permutation(n).astype(np.uint64) + np.uint64(10)
    t = table_with(hip_engine, _lib.METRIC_NPHD, 1, 32, keys, words, nb)
    try:
        mh = np.full(33, -1, dtype=np.int16)
        for p in range(1, 33):
            mh[p] = 0 if tau == 0 else (p if tau == "mid" else 8 * p)
        if tau == "full":             # every pair qualifies: a smaller table
            t.drop()
            sub = slice(0, 700)
            t = table_with(hip_engine, _lib.METRIC_NPHD, 1, 32, keys[sub], words[sub], nb[sub])
            assert check(t, keys[sub], words[sub], nb[sub], mh) == 700 * 699 // 2
        else:
            assert check(t, keys, words, nb, mh) > 0
    finally:
        t.drop()


def test_after_remove_empty_and_one_row(hip_engine):
    rng = np.random.default_rng(2)
    n = 3000
    words = planted(rng, n, 8, pool=60)
    keys = np.arange(1, n + 1, dtype=np.uint64)
    nb = np.full(n, 8, dtype=np.uint8)
    mh = np.full(33, -1, dtype=np.int16)
    mh[8] = 4
    t = table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, keys, words, nb)
    try:
        gone = rng.choice(n, size=700, replace=False)
        assert t.remove(keys[gone]) == 700
        keep = np.setdiff1d(np.arange(n), gone)
        assert check(t, keys[keep], words[keep], nb[keep], mh) > 0
        t.remove(keys[keep[1:]])
        assert check(t, keys[keep[:1]], words[keep[:1]], nb[keep[:1]], mh) == 0
        t.remove(keys[keep[:1]])
        assert [len(a) for a in t.join_within(mh, 10)] == [0, 0, 0, 0]
    finally:
        t.drop()


def test_capacity_retry(hip_engine):
    rng = np.random.default_rng(9)
    n = 2000
    words = planted(rng, n, 8, pool=20)
    keys = np.arange(1, n + 1, dtype=np.uint64)
    t = table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, keys, words, None)
    try:
        mh = np.full(33, -1, dtype=np.int16)
        mh[8] = 3
        full = t.join_within(mh, 10_000_000)
        total = len(full[2])
        assert total > 100
        cap = total // 3
        out = [np.empty(cap, np.uint64), np.empty(cap, np.uint64), np.empty(cap, np.uint32), np.empty(cap, np.uint16)]
        got_total = ctypes.c_uint64()
        rc = hip_engine._lib.isccsearch_join_within(hip_engine.handle, t.id, _lib.ptr(mh), cap, *(_lib.ptr(a) for a in out), ctypes.byref(got_total))
        assert rc == -errno.ENOSPC and got_total.value == total
        out = [np.empty(total, np.uint64), np.empty(total, np.uint64), np.empty(total, np.uint32), np.empty(total, np.uint16)]
        rc = hip_engine._lib.isccsearch_join_within(hip_engine.handle, t.id, _lib.ptr(mh), total, *(_lib.ptr(a) for a in out), ctypes.byref(got_total))
        assert rc == 0 and got_total.value == total
        for g, e in zip(out, full):
            assert np.array_equal(g, e)
        with pytest.raises(ValueError, match=f"{total} pairs exceed max_pairs"):
            t.join_within(mh, total - 1)
    finally:
        t.drop()


def test_million_rows_against_range_scans(hip_engine):
    """1 M synthetic 64-bit rows with planted near-copies: the join's pairs are the union of search_within over every planted row."""
    rng = np.random.default_rng(21)
    n, tau = 1 << 20, 3
    t = hip_engine.open_table(_lib.METRIC_HAMMING, 1, 8)
    try:
        t.add_synthetic(8, n, seed=77, first_row=0, key_base=1)
        # planted: 3 000 copies of random synthetic rows, up to 3 bits off, keys past the synthetic ones
        _, cols = t.export_rows(8, 0, n)
        src = rng.integers(0, n, size=3000)
        extra = cols[0, src].copy()
        for b in range(3):
            extra ^= np.left_shift(np.uint64(1), rng.integers(0, 64, size=3000).astype(np.uint64)) * (rng.random(3000) < 0.7)
        t.add(np.arange(n + 1, n + 3001, dtype=np.uint64), extra[:, None])
        mh = np.full(33, -1, dtype=np.int16)
        mh[8] = tau
        ka, kb, ham, pb = t.join_within(mh, 1_000_000)
        got = set(zip(ka.tolist(), kb.tolist(), ham.tolist()))
        # every pair has a planted row on at least one side (synthetic rows are random 64-bit words: no pair within 3 bits)
        keys_all, cols_all = t.export_rows(8, 0, t.size)
        q = np.concatenate([extra[:, None], cols[0, src][:, None]])
        qk, qh, _, qc = t.search_within(q, None, 64, tau)
        exp = set()
        qkeys = np.concatenate([np.arange(n + 1, n + 3001, dtype=np.uint64), keys_all[src]])
        for i in range(len(q)):
            for k, h in zip(qk[i, : qc[i]].tolist(), qh[i, : qc[i]].tolist()):
                if k != int(qkeys[i]):
                    exp.add((min(k, int(qkeys[i])), max(k, int(qkeys[i])), h))
        assert len(got) >= 3000 and got == exp
        assert np.all(pb == 64)
    finally:
        t.drop()


def test_find_duplicates_end_to_end(hip_engine):
    rng = np.random.default_rng(17)
    idx = HipIndex(hip_engine, HipOptions())
    try:
        idx.add_assets(build_assets(rng, 2000))
        got = idx.find_duplicates()
        exp = definition(idx)
        assert len(got) > 200
        assert {(p.iscc_id_a, p.iscc_id_b): (p.score, p.types) for p in got} == exp
        keys = [(codec.iscc_id_to_int(p.iscc_id_a), codec.iscc_id_to_int(p.iscc_id_b)) for p in got]
        assert [(-p.score, k) for p, k in zip(got, keys)] == sorted((-p.score, k) for p, k in zip(got, keys))
        assert idx.find_duplicates(min_score=0.95) == [p for p in got if p.score >= 0.95]
    finally:
        idx.close()
