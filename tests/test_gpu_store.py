"""
The column store (``csrc/store.hip.h``, ``csrc/table_kernels.hip.h``) against a plain host model
(``tests/store_model.py``): after EVERY mutating call the table's whole contents -- ``segments``, ``export_rows`` in windows, ``get``
and ``contains`` over every key and absent ones, ``size`` -- must equal the model's, bit for bit.  No tolerance anywhere.

  a  every writer of a row: the direct copy, ``split_rows_kernel``, the host staging loop, ``add_columns``, ``fill_kernel``; into an
     empty segment and behind rows; clean words and words with every bit past the code length set
  b  the second trip of every grid-stride loop of the table kernels (sizes from ``stats()["compute_units"]``)
  c  capacity growth in irregular batches with ``reserve`` interleaved
  d  swap-with-last removal: chains of moves inside one call, emptied segments, keys named twice, several segments per call
  e  the life cycle of the lazy key index, and batches it refuses
  f  export windows and every refusal of the store's entry points (all raised on the host before any launch)
  g  snapshots at table level
  h  rows left behind a segment's end by a removal, asked for through every scan family
  i  a fuzz over all of it

The bodies that need nothing but the table interface take any engine: ``tests/test_store_model.py`` runs them in the CPU tier on
the oracle-backed engine, so model and helper are themselves checked without a GPU.
"""

import os

import numpy as np
import pytest

from oracle import np_within, oracle_splitmix64_fill, oracle_topk
from store_model import StoreModel, assert_table_equals, dirty_words, key_tuples, mask_words

pytestmark = pytest.mark.gpu

HAMMING, NPHD = 0, 1


def is_hip(engine):
    return hasattr(engine, "stats")


def make_keys(rng, n, key_words, start):
    """n distinct keys; 128-bit keys share a handful of first words (assets), as simprint tables do."""
    lo = np.arange(start, start + n, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(2**61 - 1)
    return np.stack([rng.integers(0, 5, size=n).astype(np.uint64), lo], axis=1) if key_words == 2 else lo


def make_lens(rng, n, lengths):
    """Code lengths of a batch: one length, or every length but the last at random and the last exactly ONCE."""
    if len(lengths) == 1:
        return np.full(n, lengths[0], dtype=np.uint8)
    lens = rng.choice(lengths[:-1], size=n).astype(np.uint8)
    for i, b in enumerate(lengths[:-1]):      # (every length occurs, also in a batch of a few rows)
        lens[i % n] = b
    lens[int(rng.integers(len(lengths) - 1, n)) if n >= len(lengths) else n - 1] = lengths[-1]
    return lens


class Pair:
    """A table and its model, written together; every write is followed by the full comparison."""

    def __init__(self, engine, metric, key_words, max_bytes):
        self.engine, self.metric, self.key_words, self.max_bytes = engine, metric, key_words, max_bytes
        self.table = engine.open_table(metric, key_words, max_bytes)
        self.model = StoreModel(metric, key_words, max_bytes)
        self.checks = 0

    def check(self, by_key=True):
        self.checks += 1
        assert_table_equals(self.table, self.model, seed=self.checks, by_key=by_key)

    def add(self, keys, words, lens=None, trusted_unique=False, by_key=True):
        nb = lens if self.metric == NPHD else None
        self.table.add(keys, words, nb, trusted_unique=trusted_unique)
        self.model.add(keys, words, lens)
        self.check(by_key)

    def add_columns(self, nbytes, keys, cols, trusted_unique=False, by_key=True):
        self.table.add_columns(nbytes, keys, cols, trusted_unique=trusted_unique)
        self.model.add_columns(nbytes, keys, cols)
        self.check(by_key)

    def add_synthetic(self, nbytes, n, seed, first_row, key_base, by_key=True):
        """``fill_kernel`` against the host formula: word w of source row r is splitmix64(seed + 4 r + w), its key key_base + r."""
        self.table.add_synthetic(nbytes, n, seed, first_row, key_base)
        words = np.zeros((n, self.model.max_words), dtype=np.uint64)
        for w in range((nbytes + 7) // 8):
            words[:, w] = oracle_splitmix64_fill(n, seed, first=first_row, stride=4, lane=w)
        lo = np.uint64(key_base) + np.arange(first_row, first_row + n, dtype=np.uint64)
        keys = np.stack([np.zeros(n, dtype=np.uint64), lo], axis=1) if self.key_words == 2 else lo
        self.model.add(keys, words, np.full(n, nbytes))
        self.check(by_key)

    def remove(self, keys):
        got, want = self.table.remove(keys), self.model.remove(keys)
        assert got == want, f"remove returned {got}, the model removed {want}"
        self.check()
        return got

    def reserve(self, nbytes, rows):
        self.table.reserve(nbytes, rows)
        self.check()

    def unchanged_after(self, exc, match, call):
        with pytest.raises(exc, match=match):
            call()
        self.check()

    def search_equals_oracle(self, q, qlens, k):
        keys, words, lens = self.model.arrays()
        got = self.table.search(q, qlens if self.metric == NPHD else None, k)
        if self.metric == NPHD:
            exp = oracle_topk(NPHD, keys, words, lens, q, qlens, k)
        else:
            exp = oracle_topk(HAMMING, keys, words, None, q, None, k, fixed_nbytes=self.max_bytes)
        for g, e, name in zip(got, exp, ("keys", "hamming", "prefix_bits", "count")):
            np.testing.assert_array_equal(g, e, err_msg=f"search k={k}: {name}")
        return got

    def whole_table_search(self, rng, nq=3):
        """k = number of rows: the answer lists the whole table, so a row lost, doubled or changed by a move shows."""
        n = len(self.model)
        if not n:
            return
        keys, words, lens = self.model.arrays()
        pick = rng.integers(0, n, size=nq)
        q = words[pick].copy()
        q[:, 0] ^= np.uint64(1) << np.uint64(63)
        self.search_equals_oracle(q, lens[pick], min(n, 4096))

    def drop(self):
        self.table.drop()


def model_doc_freq(model, code, dup_limit):
    """Distinct first key words among the first ``dup_limit`` rows (ascending key) that hold ``code``."""
    code = tuple(int(x) for x in code)
    equal = sorted(k for k, (_, w) in model.rows.items() if w == code)[:dup_limit]
    return len({k[0] for k in equal})


def batch(rng, pair, n, lengths, start, dirty):
    """(keys, words, lens) of n new rows; ``dirty``: every bit past each code's length set, else zero."""
    keys = make_keys(rng, n, pair.key_words, start)
    lens = make_lens(rng, n, lengths)
    words = rng.integers(0, 2**64, size=(n, pair.model.max_words), dtype=np.uint64)
    words[::5] = words[0]                       # duplicates: equal codes once the padding is gone
    return keys, (dirty_words if dirty else mask_words)(words, lens), lens


# ---------------------------------------------------------------------------------------------------------------------
# a. ingest paths
# ---------------------------------------------------------------------------------------------------------------------
# (metric, key_words, max_bytes, lengths of a batch, writer).  isccsearch_add takes the direct copy for a batch of ONE length into a
# table of one-word codes, split_rows_kernel for one length and several words, the host staging loop for mixed lengths.
INGEST = {
    "direct-8": (HAMMING, 1, 8, [8], "add"),
    "direct-1": (HAMMING, 2, 1, [1], "add"),
    "direct-3": (HAMMING, 1, 3, [3], "add"),
    "direct-5": (HAMMING, 1, 5, [5], "add"),
    "direct-nphd-5-of-8": (NPHD, 1, 8, [5], "add"),
    "direct-nphd-3-of-6": (NPHD, 2, 6, [3], "add"),
    "split-16": (HAMMING, 1, 16, [16], "add"),
    "split-32": (HAMMING, 2, 32, [32], "add"),
    "split-13": (HAMMING, 2, 13, [13], "add"),
    "split-12-of-32": (NPHD, 1, 32, [12], "add"),
    "split-20-of-32": (NPHD, 2, 32, [20], "add"),
    "staged-4-lengths": (NPHD, 1, 32, [8, 12, 32, 5], "add"),
    "staged-one-word": (NPHD, 2, 8, [3, 8, 1], "add"),
    "columns-8": (HAMMING, 1, 8, [8], "columns"),
    "columns-13": (HAMMING, 2, 13, [13], "columns"),
    "columns-3-of-8": (NPHD, 1, 8, [3], "columns"),
    "columns-20-of-32": (NPHD, 1, 32, [20], "columns"),
}


@pytest.mark.parametrize("dirty", [False, True], ids=["clean", "dirty"])
@pytest.mark.parametrize("case", list(INGEST))
def test_ingest_paths(hip_engine, case, dirty):
    metric, key_words, max_bytes, lengths, writer = INGEST[case]
    rng = np.random.default_rng(sorted(INGEST).index(case) * 2 + dirty)
    pair = Pair(hip_engine, metric, key_words, max_bytes)
    try:
        start = 1
        for n in (300, 517):         # an empty segment, then behind its rows (dst_row != 0); more than one block each
            keys, words, lens = batch(rng, pair, n, lengths, start, dirty)
            start += n
            if writer == "columns":
                pair.add_columns(lengths[0], keys, np.ascontiguousarray(words[:, : (lengths[0] + 7) // 8].T))
            else:
                pair.add(keys, words, lens)
        mk, mw, ml = pair.model.arrays()
        some = np.concatenate([[0, 5, 10], rng.integers(0, len(mk), size=9)])
        # a lookup of the CLEAN code finds every row that was handed over with it, whatever its padding was
        got = pair.table.search_within(mw[some], ml[some] if metric == NPHD else None, 1000, 0)
        for i, r in enumerate(some):
            ek, eh, ep = np_within(mw, ml, mk, mw[r], int(ml[r]), 1000, 0)
            assert int(got[3][i]) == len(ek) and len(ek) >= 1, f"row {r}: {got[3][i]} rows found, {len(ek)} hold the code"
            np.testing.assert_array_equal(got[0][i, : len(ek)], ek, err_msg=f"row {r}: keys")
            np.testing.assert_array_equal(got[2][i, : len(ek)], ep, err_msg=f"row {r}: prefix bits")
            assert not got[1][i, : len(ek)].any()
        if metric == HAMMING:
            # the frequency column sorts and compares whole stored words, doc_freq scans under a mask: they agree only on clean rows
            for d in (1000, 3):
                want = np.array([model_doc_freq(pair.model, mw[r], d) for r in some], dtype=np.uint32)
                np.testing.assert_array_equal(pair.table.doc_freq(mw[some], None, d), want, err_msg=f"doc_freq, dup_limit {d}")
                np.testing.assert_array_equal(pair.table.get_freq(mk[some], d), want, err_msg=f"get_freq, dup_limit {d}")
    finally:
        pair.drop()


@pytest.mark.parametrize("metric,key_words,max_bytes,nbytes", [(HAMMING, 2, 13, 13), (NPHD, 1, 32, 20), (HAMMING, 1, 8, 8), (NPHD, 2, 8, 3)])
def test_synthetic_fill_against_the_host_formula(hip_engine, metric, key_words, max_bytes, nbytes):
    """``fill_kernel`` with first_row and key_base != 0, into an empty segment and behind rows, lengths that are no multiple of 8."""
    pair = Pair(hip_engine, metric, key_words, max_bytes)
    try:
        pair.add_synthetic(nbytes, 300, 0xC0FFEE, first_row=7, key_base=1 << 40, by_key=False)    # (get / contains would build the index)
        pair.add_synthetic(nbytes, 517, 0xC0FFEE, first_row=5000, key_base=1 << 40)
        mk, mw, ml = pair.model.arrays()
        pair.search_equals_oracle(mw[[3, 400]] ^ np.uint64(1 << 63), ml[[3, 400]], 10)
    finally:
        pair.drop()


# ---------------------------------------------------------------------------------------------------------------------
# b. grid-stride loops: the smallest sizes at which each table kernel's loop takes a second trip
# ---------------------------------------------------------------------------------------------------------------------
def _by_key(keys, *arrays):
    order = np.lexsort((keys[:, 1], keys[:, 0])) if keys.ndim == 2 else np.argsort(keys, kind="stable")
    return (keys[order],) + tuple(a[order] for a in arrays)


def test_split_rows_second_trip(hip_engine):
    n = hip_engine.stats()["compute_units"] * 8 * 256 + 3
    rng = np.random.default_rng(41)
    keys = rng.permutation(n).astype(np.uint64) + np.uint64(1)
    words = rng.integers(0, 2**64, size=(n, 2), dtype=np.uint64)
    t = hip_engine.open_table(HAMMING, 1, 16)
    try:
        t.add(keys, words, trusted_unique=True)
        assert t.segments() == {16: n}
        gk, gc = t.export_rows(16, 0, n)
        gk, gw = _by_key(gk, np.ascontiguousarray(gc.T))
        ek, ew = _by_key(keys, words)
        np.testing.assert_array_equal(gk, ek)
        np.testing.assert_array_equal(gw, ew)
    finally:
        t.drop()


def test_add_columns_mask_second_trip(hip_engine):
    """``add_columns`` of a length that is no multiple of 8 masks its last column in one launch of at most compute units x 8 blocks."""
    n = hip_engine.stats()["compute_units"] * 8 * 256 + 3
    rng = np.random.default_rng(43)
    keys = rng.permutation(n).astype(np.uint64) + np.uint64(1)
    words = rng.integers(0, 2**64, size=(n, 2), dtype=np.uint64)
    t = hip_engine.open_table(HAMMING, 1, 12)
    try:
        t.add_synthetic(12, 5, 1, 0, 1 << 40)             # (behind rows: the launch starts at row 5 of the column)
        t.add_columns(12, keys, np.ascontiguousarray(dirty_words(words, 12).T), trusted_unique=True)
        gk, gc = t.export_rows(12, 5, n)
        gk, gw = _by_key(gk, np.ascontiguousarray(gc.T))
        ek, ew = _by_key(keys, mask_words(words, 12))
        np.testing.assert_array_equal(gk, ek)
        np.testing.assert_array_equal(gw, ew)
    finally:
        t.drop()


def test_gathers_second_trip(hip_engine):
    """``get`` (gather_rows_kernel) and ``get_freq`` (gather_u32_kernel) launch at most 1 024 blocks of 256."""
    m = 1024 * 256 + 3
    rng = np.random.default_rng(42)
    n = m + 1000
    keys = rng.permutation(n).astype(np.uint64) + np.uint64(1)
    klass = rng.integers(0, n // 2, size=n)              # class sizes 0, 1, 2, 3 ...: the frequencies differ from row to row
    words = (np.uint64(0x9E3779B97F4A7C15) * (klass.astype(np.uint64) + np.uint64(1))).reshape(n, 1)
    t = hip_engine.open_table(HAMMING, 1, 8)
    try:
        t.add(keys, words, trusted_unique=True)
        asked = rng.permutation(n)[:m]
        gw, gb = t.get(keys[asked])
        np.testing.assert_array_equal(gb, np.full(m, 8, dtype=np.uint8))
        np.testing.assert_array_equal(gw, words[asked])
        np.testing.assert_array_equal(t.get_freq(keys[asked], 1000), np.bincount(klass)[klass[asked]].astype(np.uint32))
    finally:
        t.drop()


def test_fill_second_trip(hip_engine):
    n = hip_engine.stats()["compute_units"] * 16 * 256 + 3
    seed, first, base = 0xFEED, 11, 1 << 33
    t = hip_engine.open_table(HAMMING, 2, 12)
    try:
        t.add_synthetic(12, n, seed, first, base)
        gk, gc = t.export_rows(12, 0, n)
        gk, gw = _by_key(gk, np.ascontiguousarray(gc.T))
        np.testing.assert_array_equal(gk[:, 0], np.zeros(n, dtype=np.uint64))
        np.testing.assert_array_equal(gk[:, 1], np.uint64(base + first) + np.arange(n, dtype=np.uint64))
        np.testing.assert_array_equal(gw[:, 0], oracle_splitmix64_fill(n, seed, first=first, stride=4, lane=0))
        np.testing.assert_array_equal(gw[:, 1], oracle_splitmix64_fill(n, seed, first=first, stride=4, lane=1) & np.uint64(0xFFFFFFFF00000000))
    finally:
        t.drop()


# ---------------------------------------------------------------------------------------------------------------------
# c. growth
# ---------------------------------------------------------------------------------------------------------------------
GROWTH_SIZES = [1, 2047, 2048, 2049] + [1 + (i * 37) % 131 for i in range(33)] + [2047, 1, 2049, 2, 300]    # 42 batches


@pytest.mark.parametrize("max_bytes,key_words", [(8, 1), (32, 2)])
def test_growth_in_irregular_batches(hip_engine, max_bytes, key_words):
    """Capacities are multiples of 2 048 rows and at least double: 2 048 -> 4 096 -> 8 192 -> 16 384, and where ``reserve`` puts them."""
    rng = np.random.default_rng(max_bytes)
    pair = Pair(hip_engine, HAMMING, key_words, max_bytes)
    try:
        start = 1
        for i, n in enumerate(GROWTH_SIZES):
            keys, words, lens = batch(rng, pair, n, [max_bytes], start, dirty=bool(i % 2))
            start += n
            pair.add(keys, words, lens, trusted_unique=bool(i % 3 == 0))
            rows = len(pair.model)
            if i % 4 == 1:
                pair.table.reserve(max_bytes, rows // 2)    # below the row count: nothing to do (the next batch's comparison shows it)
            elif i % 4 == 2:
                pair.table.reserve(max_bytes, rows)         # at it
            elif i % 8 == 3:
                pair.reserve(max_bytes, rows + 1 + 700 * (i % 5))       # above it: a growth copy of its own when the capacity is passed
        assert len(pair.model) == sum(GROWTH_SIZES) > 8192
        pair.whole_table_search(rng)
    finally:
        pair.drop()


# ---------------------------------------------------------------------------------------------------------------------
# d. removal
# ---------------------------------------------------------------------------------------------------------------------
def row_order(pair, nbytes):
    """The keys of a segment in ROW order, to build removals whose moves chain (the expected contents come from the model alone)."""
    n = pair.table.segments().get(nbytes, 0)
    return pair.table.export_rows(nbytes, 0, n)[0]


REMOVAL = {
    "w1-k1": (HAMMING, 1, 8, [8]), "w1-k2": (HAMMING, 2, 5, [5]), "w2-k1": (HAMMING, 1, 16, [16]), "w2-k2": (HAMMING, 2, 13, [13]),
    "w4-k1": (HAMMING, 1, 32, [32]), "w4-k2": (HAMMING, 2, 32, [32]),         # 4 + 2 = 6 lanes of move_rows_kernel
    "nphd-k1": (NPHD, 1, 32, [8, 20, 32]), "nphd-k2": (NPHD, 2, 32, [3, 16, 29]),
}


@pytest.mark.parametrize("case", list(REMOVAL))
def test_removal_by_swap_with_last(hip_engine, case):
    metric, key_words, max_bytes, lengths = REMOVAL[case]
    rng = np.random.default_rng(sorted(REMOVAL).index(case))
    pair = Pair(hip_engine, metric, key_words, max_bytes)
    try:
        n = 3000
        keys = make_keys(rng, n, key_words, 1)
        lens = rng.choice(lengths, size=n).astype(np.uint8)
        words = rng.integers(0, 2**64, size=(n, pair.model.max_words), dtype=np.uint64)
        pair.add(keys, words, lens)

        def removed(victims, count=None):
            got = pair.remove(victims)
            assert count is None or got == count
            pair.whole_table_search(rng)

        b0 = lengths[0]
        order = row_order(pair, b0)
        removed(order[-1:], 1)                                                  # the last row: no move
        removed(order[:1], 1)                                                   # the first row: one move
        order = row_order(pair, b0)
        # a chain: row 0's key, then the keys that were last and last but one -- each was moved into row 0 by the removal before it
        removed(np.concatenate([order[:1], order[-1:], order[-2:-1]]), 3)
        order = row_order(pair, b0)
        # longer chains through several rows: every key of rows 3, 9, 27 is followed by the key that will have been moved into that row
        m = len(order)
        chain = [order[3], order[m - 1], order[9], order[m - 3], order[m - 2], order[m - 4], order[27], order[m - 5], order[m - 6], order[m - 7]]
        removed(np.array(chain, dtype=np.uint64), len(chain))
        order = row_order(pair, b0)
        m = len(order)
        # ... and one that walks DOWN the tail first, so that later moves read rows that earlier moves of the call wrote
        chain = [order[m - 2], order[1], order[m - 1], order[2], order[m - 3], order[0], order[m - 4]]
        removed(np.array(chain, dtype=np.uint64), len(chain))
        # a key named twice and absent keys mixed in
        order = row_order(pair, b0)
        absent = pair.model.absent_keys(rng, 3)
        removed(np.concatenate([order[4:5], absent[:1], order[4:5], order[-1:], absent[1:], order[-1:]]), 2)
        # one call that touches every segment, chains in each
        victims = []
        for b in lengths:
            o = row_order(pair, b)
            victims += [o[0], o[-1], o[len(o) // 2], o[-2], o[1]]
        removed(np.array(victims, dtype=np.uint64), len(victims))
        # a third of the table at random, in one call
        live = pair.model.keys_in_order()
        removed(live[rng.permutation(len(live))[: len(live) // 3]], len(live) // 3)
        # removed keys come back with other codes and lengths
        back = keys[np.array([k not in pair.model.rows for k in key_tuples(keys)])][:500]
        pair.add(back, rng.integers(0, 2**64, size=(len(back), pair.model.max_words), dtype=np.uint64), rng.choice(lengths, size=len(back)).astype(np.uint8))
        pair.whole_table_search(rng)
        # one segment emptied while the others stay (NPHD), then every row: ascending insertion order
        if len(lengths) > 1:
            removed(pair.model.keys_in_order(lengths[1]))
            assert lengths[1] not in pair.table.segments()
        live = pair.model.keys_in_order()
        removed(live, len(live))
        assert pair.table.size == 0 and pair.table.segments() == {}
        # ... and, refilled, in descending insertion order (every removal takes the last row: no move at all)
        pair.add(keys, words, lens)
        removed(pair.model.keys_in_order()[::-1].copy(), n)
        # the only row of a segment
        pair.add(keys[:1], words[:1], lens[:1])
        removed(keys[:1], 1)
        pair.add(keys[:2], words[:2], lens[:2])
    finally:
        pair.drop()


def test_removal_of_20000_keys_out_of_30000(hip_engine):
    rng = np.random.default_rng(2030)
    pair = Pair(hip_engine, HAMMING, 2, 16)
    try:
        keys = make_keys(rng, 30_000, 2, 1)
        pair.add(keys, rng.integers(0, 2**64, size=(30_000, 2), dtype=np.uint64))
        assert pair.remove(keys[rng.permutation(30_000)[:20_000]]) == 20_000
        pair.whole_table_search(rng)
    finally:
        pair.drop()


# ---------------------------------------------------------------------------------------------------------------------
# e. key index life cycle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trusted_unique", [False, True], ids=["checked", "trusted"])
@pytest.mark.parametrize("metric,key_words,max_bytes,lengths", [(HAMMING, 1, 8, [8]), (NPHD, 2, 32, [8, 13, 32])])
def test_key_index_life_cycle(hip_engine, metric, key_words, max_bytes, lengths, trusted_unique):
    rng = np.random.default_rng(50 + key_words)
    pair = Pair(hip_engine, metric, key_words, max_bytes)
    mw = pair.model.max_words
    try:
        k1, w1, l1 = batch(rng, pair, 700, lengths, 1, dirty=False)
        pair.add(k1, w1, l1, trusted_unique=trusted_unique, by_key=False)          # trusted rows: no index yet
        if is_hip(hip_engine) and trusted_unique:
            pair.add_synthetic(lengths[0], 40, 77, first_row=3, key_base=1 << 50, by_key=False)      # ... which only a table without index takes
        assert pair.table.contains(k1[:5]).all()                                     # builds the index from the device's keys
        pair.check()
        k2, w2, l2 = batch(rng, pair, 300, lengths, 701, dirty=True)
        pair.add(k2, w2, l2, trusted_unique=trusted_unique)                          # the indexed commit
        pair.remove(np.concatenate([k1[::7], k2[-3:]]))
        k3, w3, _ = batch(rng, pair, 200, lengths[-1:], 1001, dirty=False)
        pair.add_columns(lengths[-1], k3, np.ascontiguousarray(w3[:, : (lengths[-1] + 7) // 8].T), trusted_unique=trusted_unique)
        if is_hip(hip_engine):
            pair.unchanged_after(ValueError, "synthetic rows cannot be added to a table whose key index is built", lambda: pair.table.add_synthetic(lengths[0], 10, 1, 0, 1 << 51))
        # refused batches leave the table as it was: a key that is present, a key repeated inside the batch
        k4, w4, l4 = batch(rng, pair, 50, lengths, 2001, dirty=False)
        nb4 = l4 if metric == NPHD else None
        present = k4.copy()
        present[31] = k2[10]
        pair.unchanged_after(KeyError, "already present", lambda: pair.table.add(present, w4, nb4))
        twice = k4.copy()
        twice[49] = k4[2]
        pair.unchanged_after(KeyError, "already present", lambda: pair.table.add(twice, w4, nb4))
        cols = np.ascontiguousarray(w4[:, : (lengths[-1] + 7) // 8].T)
        pair.unchanged_after(KeyError, "already present", lambda: pair.table.add_columns(lengths[-1], present, cols))
        pair.unchanged_after(KeyError, "already present", lambda: pair.table.add_columns(lengths[-1], twice, cols))
        pair.add(k4, w4, l4)                                                         # the same rows, clean, are taken
        pair.whole_table_search(rng)
    finally:
        pair.drop()


# ---------------------------------------------------------------------------------------------------------------------
# f. export windows and refusals.  Every refusal below is raised before anything is launched: by HipTable's argument checks, by
#    check_nbytes, by the window test of isccsearch_export or by the length loop of isccsearch_add (store.hip.h).
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,key_words,max_bytes,nbytes", [(HAMMING, 1, 13, 13), (NPHD, 2, 32, 20)])
def test_export_windows_and_refusals(hip_engine, metric, key_words, max_bytes, nbytes):
    rng = np.random.default_rng(60)
    pair = Pair(hip_engine, metric, key_words, max_bytes)
    t, W, n = pair.table, (nbytes + 7) // 8, 333
    try:
        keys, words, lens = batch(rng, pair, n, [nbytes], 1, dirty=False)
        pair.add(keys, words, lens)
        whole_keys, whole_cols = t.export_rows(nbytes, 0, n)
        assert whole_keys.shape[0] == n and whole_cols.shape == (W, n)
        for first, count in ((0, 0), (n, 0), (n - 1, 1), (0, n)):
            k, c = t.export_rows(nbytes, first, count)
            np.testing.assert_array_equal(k, whole_keys[first : first + count])
            np.testing.assert_array_equal(c, whole_cols[:, first : first + count])
        refused = [
            (rf"rows \[{n}, \+1\) outside the segment's {n} rows", lambda: t.export_rows(nbytes, n, 1)),
            (rf"rows \[0, \+{n + 1}\) outside the segment's {n} rows", lambda: t.export_rows(nbytes, 0, n + 1)),
            (rf"nbytes 0 outside 1\.\.{max_bytes}", lambda: t.export_rows(0, 0, 1)),
            (rf"nbytes {max_bytes + 1} outside 1\.\.{max_bytes}", lambda: t.export_rows(max_bytes + 1, 0, 1)),
            (rf"nbytes {max_bytes + 1} outside 1\.\.{max_bytes}", lambda: t.reserve(max_bytes + 1, 10)),
            (rf"nbytes 0 outside 1\.\.{max_bytes}", lambda: t.reserve(0, 10)),
            (rf"nbytes 0 outside 1\.\.{max_bytes}", lambda: t.add_columns(0, keys[:2] + np.uint64(10**6), np.zeros((0, 2), dtype=np.uint64))),
            (rf"nbytes {max_bytes + 1} outside 1\.\.{max_bytes}", lambda: t.add_columns(max_bytes + 1, keys[:2] + np.uint64(10**6), np.zeros(((max_bytes + 8) // 8, 2), dtype=np.uint64))),
            (rf"cols must be shaped \[{W}, 2\]", lambda: t.add_columns(nbytes, keys[:2] + np.uint64(10**6), np.zeros((W + 1, 2), dtype=np.uint64))),
            (rf"cols must be shaped \[{W}, 2\]", lambda: t.add_columns(nbytes, keys[:2] + np.uint64(10**6), np.zeros((W, 3), dtype=np.uint64))),
        ]
        if metric == HAMMING:
            refused += [
                (rf"Hamming tables hold {max_bytes}-byte codes only", lambda: t.add_columns(8, keys[:2] + np.uint64(10**6), np.zeros((1, 2), dtype=np.uint64))),
                (rf"Hamming tables hold {max_bytes}-byte codes only", lambda: t.reserve(max_bytes - 1, 10)),
            ]
        else:
            bad = np.array([nbytes, max_bytes + 1], dtype=np.uint8)
            refused += [
                (rf"row 1: code length {max_bytes + 1} outside 1\.\.{max_bytes} bytes", lambda: t.add(keys[:2] + np.uint64(10**6), words[:2], bad)),
                (r"row 0: code length 0 outside", lambda: t.add(keys[:2] + np.uint64(10**6), words[:2], np.zeros(2, dtype=np.uint8))),
            ]
        for match, call in refused:
            pair.unchanged_after(ValueError, match, call)
    finally:
        pair.drop()


# ---------------------------------------------------------------------------------------------------------------------
# g. snapshots at table level
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,key_words,max_bytes,lengths", [(HAMMING, 2, 13, [13]), (NPHD, 1, 32, [5, 12, 32])], ids=["hamming13-k2", "nphd-k1"])
def test_snapshots_at_table_level(hip_engine, tmp_path, metric, key_words, max_bytes, lengths):
    rng = np.random.default_rng(70 + metric)
    pair = Pair(hip_engine, metric, key_words, max_bytes)
    others = []
    try:
        keys, words, lens = batch(rng, pair, 211, lengths, 1, dirty=True)
        pair.add(keys, words, lens)
        for i, (save_chunk, load_chunk) in enumerate([(1, 97), (97, 1), (10**6, 10**6)]):      # chunks of 1 row, a prime, more than a segment
            path = str(tmp_path / f"snap{i}")
            pair.table.save(path, chunk_rows=save_chunk)
            fresh = Pair(hip_engine, metric, key_words, max_bytes)
            others.append(fresh)
            fresh.table.load(path, chunk_rows=load_chunk)
            fresh.model.rows = dict(pair.model.rows)
            fresh.check()
        # load APPENDS: behind the rows a table already holds
        behind = Pair(hip_engine, metric, key_words, max_bytes)
        others.append(behind)
        k2, w2, l2 = batch(rng, behind, 100, lengths, 5000, dirty=True)
        behind.add(k2, w2, l2)
        behind.table.load(path, chunk_rows=64)
        behind.model.rows.update(pair.model.rows)
        behind.check()
        # the reloaded table takes removals and rows like any other
        fresh.remove(keys[::3])
        fresh.add(k2, w2, l2)
        fresh.whole_table_search(rng)
        # a truncated column file is refused before a row is taken (the first segment's: nothing of the snapshot was loaded yet)
        first = min(pair.model.segments())
        name = os.path.join(path, f"seg{first:02d}.w0.u64")
        with open(name, "r+b") as f:
            f.truncate(os.path.getsize(name) - 8)
        empty = Pair(hip_engine, metric, key_words, max_bytes)
        others.append(empty)
        empty.unchanged_after(ValueError, f"segment {first} is truncated", lambda: empty.table.load(path))
    finally:
        pair.drop()
        for p in others:
            p.drop()


# ---------------------------------------------------------------------------------------------------------------------
# h. stale rows behind the end.  A removal leaves codes and keys in place behind a segment's row count: asked for exactly, through
#    every scan family, they must not come back -- while the surviving duplicates planted beside them must.
# ---------------------------------------------------------------------------------------------------------------------
def _launches(engine, fn):
    before = engine.stats()
    out = fn()
    after = engine.stats()
    return out, {name: after[name] - before[name] for name in ("scan_launches", "mfma_launches", "mfma_pack_launches")}


def _stale_pair(engine, nbytes, r, middle):
    """3 x 2 048 rows, r of them removed: the last r (their rows stay behind the end), or r from the middle (the tail holds copies of live rows)."""
    rng = np.random.default_rng(800 + r + nbytes)
    n = 3 * 2048
    pair = Pair(engine, HAMMING, 1, nbytes)
    keys = make_keys(rng, n, 1, 1)
    words = rng.integers(1, 2**64, size=(n, pair.model.max_words), dtype=np.uint64)
    tail = np.arange(n - r, n)
    gone = np.arange(n // 2, n // 2 + r) if middle else tail
    # exact duplicates of the tail's codes among the rows that stay (of every third, and of the first and the last), and inside the tail
    dup_of = np.unique(np.concatenate([tail[::3], tail[:1], tail[-1:]]))
    words[100 : 100 + len(dup_of)] = words[dup_of]
    words[1000 : 1000 + len(dup_of[::2])] = words[dup_of[::2]]
    if r > 1:
        words[tail[1]] = words[tail[0]]
    pair.table.add(keys, words, trusted_unique=True)
    pair.model.add(keys, words)
    # (the last rows from the back: each is the last row when its turn comes, so nothing moves and every one stays where it was)
    assert pair.remove(keys[gone] if middle else keys[gone][::-1].copy()) == r
    return pair, keys, words, gone


def _ask(pair, codes, nq):
    return np.resize(codes, (nq, codes.shape[1]))


def _no_key_twice(got):
    for i in range(got[0].shape[0]):
        listed = got[0][i, : int(got[3][i])]
        assert len(np.unique(listed)) == len(listed), f"query {i}: a key is listed twice"


@pytest.mark.parametrize("middle", [False, True], ids=["last-rows", "swapped"])
@pytest.mark.parametrize("r", [1, 63, 64, 65, 127, 2047])
def test_stale_rows_64_bit(hip_engine, r, middle):
    pair, keys, words, gone = _stale_pair(hip_engine, 8, r, middle)
    eng = hip_engine
    n = len(pair.model)
    try:
        # swapped: the rows moved into the gap came from the tail, where their copies still lie
        codes = words[-r:] if middle else words[gone]
        for k in (10, min(n, 4096)):
            with eng.options(tiny_rows=16384, mfma_min_rows=65536, mfma_min_queries=17):
                got, ran = _launches(eng, lambda: pair.search_equals_oracle(_ask(pair, codes, 12), None, k))      # tiny_search_kernel
                assert ran["scan_launches"] >= 1 and ran["mfma_launches"] == 0, ran
                _no_key_twice(got)
            with eng.options(tiny_rows=0, mfma_min_rows=65536, mfma_min_queries=17):
                got, ran = _launches(eng, lambda: pair.search_equals_oracle(_ask(pair, codes, 12), None, k))      # scan_kernel
                assert ran["scan_launches"] >= 1 and ran["mfma_launches"] == 0, ran
                _no_key_twice(got)
            with eng.options(mfma=1, mfma_pack=1, mfma_pack3=1, mfma_min_queries=1, mfma_min_rows=1):
                for nq in (12, 40, 160):                             # mfma_pack_kernel; 160 queries = 5 groups in a chunk: mfma_pack3_kernel
                    got, ran = _launches(eng, lambda: pair.search_equals_oracle(_ask(pair, codes, nq), None, k))
                    assert ran["mfma_pack_launches"] >= 1, (nq, ran)
                    _no_key_twice(got)
        mk, mw, ml = pair.model.arrays()
        q = _ask(pair, codes, 24)
        expected = [np_within(mw, 8, mk, q[i], 8, 64, 0) for i in range(len(q))]
        for opts in (dict(tiny_rows=16384), dict(tiny_rows=0), dict(tiny_rows=0, mfma=1, mfma_min_queries=1, mfma_min_rows=1)):
            with eng.options(**opts):
                got = pair.table.search_within(q, None, 64, 0)
                for i, (ek, eh, _) in enumerate(expected):
                    assert int(got[3][i]) == len(ek), f"{opts} query {i}: {got[3][i]} rows at distance 0, the model holds {len(ek)}"
                    np.testing.assert_array_equal(got[0][i, : len(ek)], ek, err_msg=f"{opts} query {i}")
                want = np.array([len(ek) for ek, _, _ in expected], dtype=np.uint32)
                np.testing.assert_array_equal(pair.table.doc_freq(q, None, 1000), want, err_msg=f"doc_freq {opts}")
        assert max(len(ek) for ek, _, _ in expected) >= 2, "no surviving duplicate was asked for"
        # build_freq_column over the rows that are left
        some = np.concatenate([np.arange(100, 100 + min(r, 30)), [0, 1000, len(keys) // 3]])
        some = some[[key in pair.model.rows for key in key_tuples(keys[some])]]
        want = np.array([model_doc_freq(pair.model, words[i].tolist(), 1000) for i in some], dtype=np.uint32)
        np.testing.assert_array_equal(pair.table.get_freq(keys[some], 1000), want, err_msg="get_freq")
        # join_scan_kernel at radius 0: the pairs of equal codes among the rows that are left
        mh = np.full(33, -1, dtype=np.int16)
        mh[8] = 0
        ka, kb, ham, pbits = pair.table.join_within(mh, 1_000_000)
        by_code = {}
        for key, code in zip(mk.tolist(), mw[:, 0].tolist()):
            by_code.setdefault(code, []).append(key)
        pairs = sorted((a, b) for ks in by_code.values() for a in ks for b in ks if a < b)
        assert list(zip(ka.tolist(), kb.tolist())) == pairs and len(pairs) >= 1
        assert not ham.any() and (pbits == 64).all()
    finally:
        pair.drop()


@pytest.mark.parametrize("middle", [False, True], ids=["last-rows", "swapped"])
@pytest.mark.parametrize("r", [1, 63, 64, 65, 127, 2047])
def test_stale_rows_128_bit(hip_engine, r, middle):
    """The same through ``mfma_scan_kernel`` (two-word codes), and through the XOR + popcount kernels for comparison."""
    pair, keys, words, gone = _stale_pair(hip_engine, 16, r, middle)
    eng = hip_engine
    n = len(pair.model)
    try:
        codes = words[-r:] if middle else words[gone]
        for k in (10, min(n, 4096)):
            with eng.options(mfma=1, mfma_min_queries=1, mfma_min_rows=1):
                for nq in (12, 40):
                    got, ran = _launches(eng, lambda: pair.search_equals_oracle(_ask(pair, codes, nq), None, k))
                    assert ran["mfma_launches"] >= 1 and ran["mfma_pack_launches"] == 0, (nq, ran)
                    _no_key_twice(got)
            with eng.options(tiny_rows=0, mfma_min_rows=65536, mfma_min_queries=17):
                _no_key_twice(pair.search_equals_oracle(_ask(pair, codes, 12), None, k))
            with eng.options(tiny_rows=16384, mfma_min_rows=65536, mfma_min_queries=17):
                _no_key_twice(pair.search_equals_oracle(_ask(pair, codes, 12), None, k))
    finally:
        pair.drop()


# ---------------------------------------------------------------------------------------------------------------------
# i. a store fuzz
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_store_fuzz(hip_engine, tmp_path, seed):
    rng = np.random.default_rng(9000 + seed)
    metric = int(rng.integers(0, 2))
    key_words = int(rng.integers(1, 3))
    max_bytes = int(rng.choice([1, 3, 8, 12, 16, 21, 32]))
    lengths = [max_bytes] if metric == HAMMING else sorted({max_bytes, max(1, max_bytes // 2), max(1, max_bytes - 3), 1})
    pair = Pair(hip_engine, metric, key_words, max_bytes)
    retired = []
    next_key = 1
    try:
        for step in range(25):
            op = str(rng.choice(["add", "add", "add", "remove", "remove", "reserve", "contains", "snapshot"]))
            rows = len(pair.model)
            if step == 0 and is_hip(hip_engine) and seed % 3 == 0:
                pair.add_synthetic(int(rng.choice(lengths)), int(rng.choice([1, 300, 2049])), seed, first_row=int(rng.integers(0, 1000)), key_base=1 << 62, by_key=False)
            elif op == "add" or rows == 0:
                n = int(rng.choice([1, 2, 7, 300, 2047, 2049]))
                if rows + n > 6000:
                    continue
                path = str(rng.choice(["one-length", "mixed", "columns"]))
                keys, words, lens = batch(rng, pair, n, lengths if path == "mixed" else [int(rng.choice(lengths))], next_key, dirty=bool(rng.integers(0, 2)))
                next_key += n
                trusted = bool(rng.integers(0, 2))
                if path == "columns":
                    pair.add_columns(int(lens[0]), keys, np.ascontiguousarray(words[:, : (int(lens[0]) + 7) // 8].T), trusted_unique=trusted)
                else:
                    pair.add(keys, words, lens, trusted_unique=trusted)
            elif op == "remove":
                live = pair.model.keys_in_order()
                m = min(rows, int(rng.choice([1, 2, 50, 1500])))
                victims = np.concatenate([live[rng.permutation(rows)[:m]], pair.model.absent_keys(rng, 2), live[-1:], live[:1]])
                pair.remove(victims[rng.permutation(len(victims))])
            elif op == "reserve":
                b = int(rng.choice(lengths))
                pair.reserve(b, int(rng.choice([0, rows // 2, pair.model.segments().get(b, 0), rows + 1, rows + 2049])))
            elif op == "contains":
                asked = np.concatenate([pair.model.keys_in_order()[:: max(1, rows // 40)], pair.model.absent_keys(rng, 5)])
                np.testing.assert_array_equal(pair.table.contains(asked), np.array([k in pair.model.rows for k in key_tuples(asked)]))
                pair.check()
            else:
                path = str(tmp_path / f"step{step}")
                pair.table.save(path, chunk_rows=int(rng.choice([97, 1000, 10**6])))
                fresh = Pair(hip_engine, metric, key_words, max_bytes)
                retired.append(pair)
                fresh.model.rows, fresh.checks = dict(pair.model.rows), pair.checks
                fresh.table.load(path, chunk_rows=int(rng.choice([211, 10**6])))
                pair = fresh                        # ... and the sequence goes on with the reloaded table
                pair.check()
        pair.whole_table_search(rng)
    finally:
        pair.drop()
        for p in retired:
            p.drop()
