"""
A plain host model of one table of the column store -- TEST INFRASTRUCTURE.

The model is a dict: key -> (code length in bytes, code words).  What it states about a table:

  * a row's last kept word is masked to the code length and the words past it are zero, whichever entry point wrote it
    and whatever the caller left in the bits past the length;
  * per code length there is one segment that holds exactly the model's (key, words) pairs of that length, every key once;
  * nothing about row order inside a segment (swap-with-last removal moves rows): the only order claims are that
    ``export_rows`` windows tile a segment without gap or overlap and that ``segments()`` gives the model's counts.

``assert_table_equals(table, model)`` compares a ``HipTable`` -- or the oracle-backed ``OracleTable`` of the CPU tier -- with
the model through every read entry point of the store: ``segments``, ``export_rows``, ``get``, ``contains``, ``size``.
"""

import numpy as np

FULL = 0xFFFFFFFFFFFFFFFF


def word_mask(nbytes, w):
    # type: (int, int) -> int
    """Mask of word ``w`` of a code of ``nbytes`` bytes: codes are packed big-endian, so the kept bytes are the word's top ones."""
    inside = min(8, max(0, nbytes - 8 * w))
    return (FULL << (8 * (8 - inside))) & FULL


def mask_words(words, nbytes):
    # type: (np.ndarray, np.ndarray | int) -> np.ndarray
    """``words`` [n, max_words] with every bit past each row's code length cleared."""
    words = np.array(words, dtype=np.uint64, ndmin=2)
    lens = np.broadcast_to(np.asarray(nbytes, dtype=np.int64), (words.shape[0],))
    for b in np.unique(lens).tolist():
        sel = lens == b
        for w in range(words.shape[1]):
            words[sel, w] &= np.uint64(word_mask(b, w))
    return words


def dirty_words(words, nbytes):
    # type: (np.ndarray, np.ndarray | int) -> np.ndarray
    """The same codes with EVERY bit past each row's code length set: what a careless caller of the C-ABI may hand over."""
    clean = mask_words(words, nbytes)
    return clean | ~mask_words(np.full(clean.shape, FULL, dtype=np.uint64), nbytes)


def key_tuples(keys):
    # type: (np.ndarray) -> list[tuple]
    keys = np.asarray(keys, dtype=np.uint64)
    return [tuple(k) for k in keys.tolist()] if keys.ndim == 2 else [(k,) for k in keys.tolist()]


class StoreModel:
    """What a table must hold after a sequence of adds and removes."""

    def __init__(self, metric, key_words, max_bytes):
        # type: (int, int, int) -> None
        self.metric, self.key_words, self.max_bytes = metric, key_words, max_bytes
        self.max_words = (max_bytes + 7) // 8
        self.rows = {}      # key tuple -> (nbytes, words tuple [max_words]); dicts keep insertion order

    def __len__(self):
        return len(self.rows)

    def add(self, keys, words, nbytes=None):
        # type: (np.ndarray, np.ndarray, np.ndarray | None) -> None
        """Rows as ``HipTable.add`` takes them; a key already present or repeated in the batch raises KeyError and changes nothing."""
        kts = key_tuples(keys)
        if len(set(kts)) != len(kts) or any(k in self.rows for k in kts):
            raise KeyError("key already present")
        lens = np.full(len(kts), self.max_bytes, dtype=np.int64) if nbytes is None else np.asarray(nbytes, dtype=np.int64)
        assert lens.min(initial=1) >= 1 and lens.max(initial=1) <= self.max_bytes
        assert self.metric == 1 or (lens == self.max_bytes).all()
        stored = mask_words(np.asarray(words, dtype=np.uint64).reshape(len(kts), self.max_words), lens)
        for k, b, w in zip(kts, lens.tolist(), stored.tolist()):
            self.rows[k] = (b, tuple(w))

    def add_columns(self, nbytes, keys, cols):
        # type: (int, np.ndarray, np.ndarray) -> None
        """Rows of one length as ``HipTable.add_columns`` takes them: ``cols`` [W, n] word-major."""
        cols = np.asarray(cols, dtype=np.uint64)
        words = np.zeros((cols.shape[1], self.max_words), dtype=np.uint64)
        words[:, : cols.shape[0]] = cols.T
        self.add(keys, words, np.full(cols.shape[1], nbytes))

    def remove(self, keys):
        # type: (np.ndarray) -> int
        """Rows removed: a key that is absent, or named a second time, counts for nothing."""
        return sum(self.rows.pop(k, None) is not None for k in key_tuples(keys))

    def segments(self):
        # type: () -> dict[int, int]
        out = {}
        for b, _ in self.rows.values():
            out[b] = out.get(b, 0) + 1
        return dict(sorted(out.items()))

    def segment_set(self, nbytes):
        # type: (int) -> set
        """{(key tuple, words tuple [W])} of one segment."""
        W = (nbytes + 7) // 8
        return {(k, w[:W]) for k, (b, w) in self.rows.items() if b == nbytes}

    def keys_in_order(self, nbytes=None):
        # type: (int | None) -> np.ndarray
        """The live keys in insertion order (of one segment, or of the whole table) as ``HipTable`` takes keys."""
        return self._key_array([k for k, (b, _) in self.rows.items() if nbytes is None or b == nbytes])

    def _key_array(self, kts):
        arr = np.array(kts, dtype=np.uint64).reshape(len(kts), self.key_words)
        return arr if self.key_words == 2 else arr[:, 0]

    def arrays(self):
        # type: () -> tuple
        """(keys, words [n, max_words], nbytes [n]) for ``oracle.oracle_topk``."""
        words = np.array([w for _, w in self.rows.values()], dtype=np.uint64).reshape(len(self.rows), self.max_words)
        return self.keys_in_order(), words, np.array([b for b, _ in self.rows.values()], dtype=np.uint8)

    def absent_keys(self, rng, n):
        # type: (np.random.Generator, int) -> np.ndarray
        """``n`` keys the model does not hold: neighbours of live keys (the likeliest wrong hits) and random ones."""
        out = {}
        live = list(self.rows)
        while len(out) < n:
            if live and rng.random() < 0.5:
                base = live[int(rng.integers(0, len(live)))]
                k = base[:-1] + ((base[-1] + int(rng.integers(1, 3))) & FULL,)
            else:
                k = tuple(int(x) for x in rng.integers(0, 2**64, size=self.key_words, dtype=np.uint64))
            if k not in self.rows:
                out[k] = None
        return self._key_array(list(out))


def export_segment(table, nbytes, n, cuts):
    # type: (object, int, int, list[int]) -> tuple
    """Rows [0, n) of a segment read through consecutive ``export_rows`` windows that end at ``cuts`` and at n."""
    edges = sorted({0, n, *[c for c in cuts if 0 <= c <= n]})
    if len(edges) < 3:
        edges = [0] + edges if n else [0, 0, 0]       # still two windows: an empty one in front
    parts = [table.export_rows(nbytes, a, b - a) for a, b in zip(edges[:-1], edges[1:])]
    for (k, c), a, b in zip(parts, edges[:-1], edges[1:]):
        assert k.shape[0] == b - a and c.shape == ((nbytes + 7) // 8, b - a), f"segment {nbytes}: window [{a}, {b}) came back shaped {k.shape} / {c.shape}"
    return np.concatenate([k for k, _ in parts]), np.concatenate([c for _, c in parts], axis=1)


def assert_table_equals(table, model, seed=0, by_key=True):
    # type: (object, StoreModel, int, bool) -> None
    """
    The table holds exactly the model's rows.  ``by_key=False`` leaves out ``get`` and ``contains``: they build the table's key
    index, which a caller that tests the paths of an unindexed table must not do yet.
    """
    rng = np.random.default_rng(seed)
    assert table.segments() == model.segments(), f"segments(): {table.segments()} != {model.segments()}"
    assert table.size == len(model), f"size: {table.size} != {len(model)}"
    for nbytes, n in model.segments().items():
        W = (nbytes + 7) // 8
        keys, cols = export_segment(table, nbytes, n, [int(rng.integers(0, n + 1)), n // 2])
        kts = key_tuples(keys)
        assert len(set(kts)) == n, f"segment {nbytes}: {n - len(set(kts))} keys exported twice"
        past = cols[W - 1] & np.uint64(FULL ^ word_mask(nbytes, W - 1))
        assert not past.any(), f"segment {nbytes}: {int(np.count_nonzero(past))} rows with bits set past the code length, first {int(past[np.nonzero(past)[0][0]]):#x}"
        got = set(zip(kts, (tuple(w) for w in cols.T.tolist())))
        want = model.segment_set(nbytes)
        if got != want:
            missing, extra = sorted(want - got)[:3], sorted(got - want)[:3]
            raise AssertionError(f"segment {nbytes}: {len(want - got)} rows missing or changed (first {missing}), {len(got - want)} not in the model (first {extra})")
    if not by_key:
        return
    live = model.keys_in_order()
    absent = model.absent_keys(rng, 7 + min(len(model) // 8, 250))
    asked = np.concatenate([live, absent]) if len(live) else absent
    asked = asked[rng.permutation(len(asked))]
    words, lens = table.get(asked)
    found = table.contains(asked)
    assert words.shape == (len(asked), model.max_words) and lens.shape == (len(asked),) and found.shape == (len(asked),)
    exp = [model.rows.get(k, (0, (0,) * model.max_words)) for k in key_tuples(asked)]
    np.testing.assert_array_equal(lens, np.array([b for b, _ in exp], dtype=np.uint8), err_msg="get: code lengths (0 = absent)")
    np.testing.assert_array_equal(words, np.array([w for _, w in exp], dtype=np.uint64).reshape(words.shape), err_msg="get: code words")
    np.testing.assert_array_equal(found, np.array([b != 0 for b, _ in exp]), err_msg="contains")
