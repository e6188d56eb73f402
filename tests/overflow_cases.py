"""
Tables and batches that FORCE a candidate list past its buffer (numpy only; nothing of the engine is imported here).

Every search keeps ``cap`` candidates per query (``Batch::reserve``, csrc/batch.hip.h); a list that outgrows it is answered again by
the retry with levels, by ``Batch::fix_query`` or -- device-resident lists -- marked ``COUNT_OVERFLOW``.  The cases below plant, per
"hot" query, a class of rows whose size alone decides whether that happens:

    near    rows at distances 1 .. d - 1 of the hot query, fewer than any k the tests ask for
    tie     rows at EXACTLY distance d (d > 0: pairwise distinct codes, the flipped bits spread over every compared word and, in a
            masked last word, over its live bits only; d = 0: equal codes)
    others  random rows, each checked to lie beyond d of every hot query

With fewer than k rows nearer than d, the k-th distance of a hot query is d, every valid threshold admits the ``near + tie`` rows
within d, and the list overflows exactly when ``near + tie > cap``.  tests/test_overflow_cases.py proves these counts from the rows;
tests/test_gpu_overflow.py runs the engine over them.  Keys come in the patterns that walk the key radixes through bytes they never
see otherwise (``make_keys``).
"""

import functools

import numpy as np

import threshold_model as tm

METRIC_HAMMING, METRIC_NPHD = 0, 1
ALL_ONES = 0xFFFFFFFFFFFFFFFF
HIGH = 0xFFFFFFFFFF000000          # the top five key bytes 0xFF (and with them the top bit)
TOP_BIT_ASSET = 0x8000000000000001
U64 = np.uint64


def cap_of(candidate_cap, k, single_pass):
    # type: (int, int, bool) -> int
    """
    Entries of the per-query candidate buffer.  Mirrors the first two statements of ``Batch::reserve`` (csrc/batch.hip.h):
    ``cap = max(candidate_cap, 16 * k)``, raised to ``max(cap, 64 * k)`` when ``self_tighten`` and ``mfma`` are on and the search has
    neither a radius nor a radius ratio -- ``single_pass`` says that all of these hold.  (The raise does not look at whether the batch
    really takes the single pass: its retry with levels keeps the same buffer.)
    """
    cap = max(int(candidate_cap), 16 * k)
    return max(cap, 64 * k) if single_pass else cap


def make_keys(rng, n, key_words, pattern, hi=None):
    # type: (np.random.Generator, int, int, str, int | None) -> np.ndarray
    """
    ``n`` unique keys, uint64 [n] or [n, 2] (hi, lo), in table order (not key order):

        small       perm + 7                                                  (two words: hi = 1 + perm % 299)
        high        0xFFFFFFFFFF000000 | i: five 0xFF bytes, top bit set      (two words: hi = HIGH | i >> 8, lo = HIGH | i)
        spread      top byte from {0x00, 0x7F, 0x80, 0xFF}, i + 1 below it    (two words: that byte tops hi, lo = i + 1)
        one_asset   (two words) hi = ``hi`` for every row, lo = HIGH | i: a radix meets its first cut in the LOW word, byte 13
        few_assets  (two words) hi from {0, 1, 0xFF..FE, 0xFF..FF} -- the first two rare --, lo contiguous
    """
    if n >= 1 << 24:
        raise ValueError("the patterns keep 24 bits for the row")
    i = rng.permutation(n).astype(U64)
    top = rng.choice(np.array([0x00, 0x7F, 0x80, 0xFF], dtype=U64), size=n) << U64(56)
    if key_words == 1:
        if pattern == "small":
            keys = i + U64(7)
        elif pattern == "high":
            keys = U64(HIGH) | i
        elif pattern == "spread":
            keys = top | (i + U64(1))
        else:
            raise ValueError(f"no one-word key pattern '{pattern}'")
        assert len(np.unique(keys)) == n
        return keys
    if pattern == "small":
        his, lo = U64(1) + i % U64(299), rng.permutation(n).astype(U64) + U64(7)
    elif pattern == "high":
        his, lo = U64(HIGH) | (i >> U64(8)), U64(HIGH) | i
    elif pattern == "spread":
        his, lo = top, i + U64(1)
    elif pattern == "one_asset":
        his, lo = np.full(n, hi, dtype=U64), U64(HIGH) | i
    elif pattern == "few_assets":
        his = rng.choice(np.array([0, 1, ALL_ONES - 1, ALL_ONES], dtype=U64), size=n, p=[0.02, 0.02, 0.48, 0.48])
        lo = i + U64(1000)
    else:
        raise ValueError(f"no two-word key pattern '{pattern}'")
    keys = np.stack([his, lo], axis=1)
    assert len(np.unique(keys, axis=0)) == n
    return keys


def _flips(rng, count, nb, pbytes, max_words):
    # type: (np.random.Generator, int, int, int, int) -> np.ndarray
    """
    uint64 [count, max_words]: pairwise distinct XOR patterns of exactly ``nb`` bits inside the first ``pbytes`` bytes (big-endian
    packed: bit 0 is the top of word 0).  With ``nb`` at least the number of compared words every word gets one of them -- the
    last word among its live bits, which are the only ones ever drawn.
    """
    out = np.zeros((count, max_words), dtype=U64)
    if nb == 0 or count == 0:
        return out
    bits = 8 * pbytes
    words = (pbytes + 7) // 8
    have = np.zeros((0, max_words), dtype=U64)
    while len(have) < count:
        m = count - len(have) + 16
        r = rng.random((m, bits), dtype=np.float32)
        if nb >= words:
            for w in range(words):
                live = min(64, bits - 64 * w)
                r[np.arange(m), 64 * w + rng.integers(0, live, size=m)] = -1.0
        pos = np.argsort(r, axis=1, kind="stable")[:, :nb]
        x = np.zeros((m, max_words), dtype=U64)
        for j in range(nb):
            x[np.arange(m), pos[:, j] // 64] ^= U64(1) << (63 - pos[:, j] % 64).astype(U64)
        both = np.concatenate([have, x])
        _, first = np.unique(both, axis=0, return_index=True)
        have = both[np.sort(first)]
    return have[:count]


def flip_bytes(rng, count, nb, nbytes):
    # type: (np.random.Generator, int, int, int) -> np.ndarray
    """``_flips`` over whole codes of ``nbytes`` bytes, as bytes: uint8 [count, nbytes] XOR patterns of ``nb`` bits, pairwise distinct."""
    W = (nbytes + 7) // 8
    return _flips(rng, count, nb, nbytes, W).astype(">u8").view(np.uint8).reshape(count, 8 * W)[:, :nbytes]


class Case:
    """
    One planted table.  ``keys`` / ``words`` / ``lens`` (None: fixed length) as ``HipTable.add`` takes them; ``hot`` [h, W] and
    ``hot_bytes`` [h] the hot queries; ``classes`` the planted classes, each with the ``rows`` it owns (``near_rows``, ``tie_rows``).
    """

    def __init__(self, metric, max_bytes, key_words, keys, words, lens, hot, hot_bytes, classes):
        self.metric, self.max_bytes, self.key_words = metric, max_bytes, key_words
        self.max_words = (max_bytes + 7) // 8
        self.keys, self.words, self.lens, self.hot, self.hot_bytes, self.classes = keys, words, lens, hot, hot_bytes, classes
        for a in (keys, words, hot, hot_bytes) + ((lens,) if lens is not None else ()):
            a.setflags(write=False)

    @property
    def n(self):
        return len(self.words)

    def row_bytes(self):
        return np.full(self.n, self.max_bytes, dtype=np.int64) if self.lens is None else self.lens.astype(np.int64)

    def segments(self):
        return sorted(set(self.row_bytes().tolist()))

    def qlen(self, qbytes):
        return self.max_bytes if self.metric == METRIC_HAMMING else int(qbytes)

    def dist(self, q_words, qbytes):
        # type: (np.ndarray, int) -> np.ndarray
        """Hamming distance of ONE query to every row over the compared prefix, min(query length, row length) bytes: int64 [n]."""
        return _prefix_distances(self.words, self.row_bytes(), q_words, self.qlen(qbytes))

    def class_of(self, hot, seg=None):
        found = [c for c in self.classes if c["hot"] == hot and (seg is None or c["seg"] == seg)]
        assert len(found) == 1
        return found[0]

    def size_of(self, hot, seg=None):
        c = self.class_of(hot, seg)
        return c["near"] + c["tie"]

    def hot_query(self, hot):
        return self.hot[hot], int(self.hot_bytes[hot])

    def listed(self, q_words, qbytes, k):
        # type: (np.ndarray, int, int) -> dict
        """Per segment, the rows within the query's k-th distance OVER THAT SEGMENT: what the tightest valid threshold lists for its job."""
        d, rb, out = self.dist(q_words, qbytes), self.row_bytes(), {}
        for b in self.segments():
            ds = np.sort(d[rb == b])
            out[b] = int((ds <= ds[min(k, len(ds)) - 1]).sum())
        return out


def _with_defaults(classes, max_bytes):
    # type: (list[dict], int) -> tuple
    """Copies of the class dicts with ``hot``, ``seg`` and ``qbytes`` filled in, and the byte length of every hot query: uint8 [hot queries]."""
    classes = [dict(c) for c in classes]
    for i, c in enumerate(classes):
        c.setdefault("hot", i)
        c.setdefault("seg", max_bytes)
        c.setdefault("qbytes", max_bytes)
        if c["near"] and c["d"] < 2:
            raise ValueError("no distance strictly between 0 and d for the near rows")
    hot_bytes = np.zeros(1 + max((c["hot"] for c in classes), default=-1), dtype=np.uint8)
    for c in classes:
        assert hot_bytes[c["hot"]] in (0, c["qbytes"]), "classes of one hot query name one query length"
        hot_bytes[c["hot"]] = c["qbytes"]
    return classes, hot_bytes


def _class_rows(rng, c, hot_query, W):
    # type: (np.random.Generator, dict, np.ndarray, int) -> np.ndarray
    """The ``near`` rows, then the ``tie`` rows of one class: the hot query's prefix with bits flipped, random behind the prefix both share."""
    m = c["near"] + c["tie"]
    p = min(c["seg"], c["qbytes"])
    rows = rng.integers(0, 2**64, size=(m, W), dtype=U64) & tm.prefix_masks(c["seg"], W)
    pm = tm.prefix_masks(p, W)
    rows = (rows & ~pm) | (hot_query & pm)
    for j in range(c["near"]):
        dj = 1 + ((j + 1) * (c["d"] - 1)) // (c["near"] + 1)
        assert 1 <= dj < c["d"]
        rows[j] ^= _flips(rng, 1, dj, p, W)[0]
    rows[c["near"]:] ^= _flips(rng, c["tie"], c["d"], p, W)
    return rows


def _random_rows(rng, lens, W):
    # type: (np.random.Generator, np.ndarray, int) -> np.ndarray
    """One random code per entry of ``lens``, zero past its byte length."""
    masks = np.stack([tm.prefix_masks(int(b), W) for b in lens]) if len(lens) else np.zeros((0, W), dtype=U64)
    return rng.integers(0, 2**64, size=(len(lens), W), dtype=U64) & masks


def _prefix_distances(words, lens, query, qbytes):
    # type: (np.ndarray, np.ndarray, np.ndarray, int) -> np.ndarray
    """Hamming distance of one query to rows of the byte lengths ``lens``, each over min(row length, query length) bytes: int64 [rows]."""
    out = np.zeros(len(words), dtype=np.int64)
    for b in set(lens.tolist()):
        sel = lens == b
        out[sel] = tm.distances(words[sel], np.asarray(query, dtype=U64).reshape(1, -1), min(int(b), int(qbytes)))[0]
    return out


def _beyond(classes, h, lens):
    # type: (list[dict], int, np.ndarray) -> np.ndarray
    """Per row length in ``lens``, the distance a row OUTSIDE hot query h's classes must exceed: the d of h's class in that segment, else h's largest d."""
    mine = {c["seg"]: c["d"] for c in classes if c["hot"] == h}
    return np.array([mine.get(int(b), max(mine.values())) for b in lens], dtype=np.int64)


def _push_random_rows_beyond(rng, words, lens, first, classes, hot, hot_bytes):
    """Rows ``first ..`` are the random ones: draw those again that lie within a planted distance of a hot query, until none does."""
    W = words.shape[1]
    for _ in range(64):
        bad = np.zeros(len(words) - first, dtype=bool)
        for h in range(len(hot)):
            bad |= _prefix_distances(words[first:], lens[first:], hot[h], hot_bytes[h]) <= _beyond(classes, h, lens[first:])
        if not bad.any():
            return
        redo = first + np.nonzero(bad)[0]
        words[redo] = _random_rows(rng, lens[redo], W)
    raise RuntimeError("random rows keep falling within a planted distance")


def planted(rng, n, nbytes, key_words, keys, classes):
    # type: (np.random.Generator, int, int | tuple, int, str | dict, list[dict]) -> Case
    """
    A table of ``n`` rows, random except for the planted classes.

    :param nbytes: the code length of a Hamming table, or the row lengths of an NPHD table (its rows cycle through them)
    :param keys: a pattern of ``make_keys``, or ``{"pattern": .., "hi": ..}``
    :param classes: one dict per class: ``d``, ``near``, ``tie``; ``hot`` (index of its hot query; default: its own position --
                    classes that name one index share the query); NPHD also ``seg`` (row length of the class) and ``qbytes`` (length
                    of its hot query): the class is planted within the prefix of min(seg, qbytes) bytes both share
    """
    nphd = not np.isscalar(nbytes)
    lengths = tuple(nbytes) if nphd else (int(nbytes),)
    max_bytes = max(lengths)
    W = (max_bytes + 7) // 8
    classes, hot_bytes = _with_defaults(classes, max_bytes)
    hot = rng.integers(0, 2**64, size=(len(hot_bytes), W), dtype=U64)
    for h in range(len(hot)):
        hot[h] &= tm.prefix_masks(int(hot_bytes[h]), W)

    # the classes in front, one after the other, the random rows behind them
    words = np.zeros((n, W), dtype=U64)
    lens = np.zeros(n, dtype=np.int64)
    spans, at = [], 0
    for c in classes:
        rows = _class_rows(rng, c, hot[c["hot"]], W)
        if at + len(rows) > n:
            raise ValueError(f"the planted rows do not fit {n}")
        words[at : at + len(rows)], lens[at : at + len(rows)] = rows, c["seg"]
        spans.append((at, at + len(rows)))
        at += len(rows)
    lens[at:] = np.array(lengths, dtype=np.int64)[np.arange(n - at) % len(lengths)]
    words[at:] = _random_rows(rng, lens[at:], W)
    _push_random_rows_beyond(rng, words, lens, at, classes, hot, hot_bytes)
    # (the rows of another query's class are planted, not drawn again: they must lie beyond too)
    for h in range(len(hot)):
        for c, (a, b) in zip(classes, spans):
            if c["hot"] != h:
                assert (_prefix_distances(words[a:b], lens[a:b], hot[h], hot_bytes[h]) > _beyond(classes, h, lens[a:b])).all(), \
                    "two planted classes overlap: take another seed"

    spec = keys if isinstance(keys, dict) else {"pattern": keys}
    key_arr = make_keys(rng, n, key_words, spec["pattern"], spec.get("hi"))
    # planted rows all over the table, not in front of it: row i of the table is row order[i] of the layout above
    order = rng.permutation(n)
    where = np.empty(n, dtype=np.int64)
    where[order] = np.arange(n)
    for c, (a, b) in zip(classes, spans):
        c["near_rows"] = np.sort(where[a : a + c["near"]])
        c["tie_rows"] = np.sort(where[a + c["near"] : b])
    return Case(METRIC_NPHD if nphd else METRIC_HAMMING, max_bytes, key_words, key_arr, words[order], lens[order].astype(np.uint8) if nphd else None,
                hot, hot_bytes, classes)


# ---------------------------------------------------------------------------------------------------------------------------------
# the tables of tests/test_gpu_overflow.py, each made once per process
# ---------------------------------------------------------------------------------------------------------------------------------
CANDIDATE_CAP = 64                      # what the GPU tests lower option candidate_cap to, unless stated
KS = (4, 10)
NEAR = 3                                # rows nearer than d per hot query with d > 0: fewer than the smallest k


def _cls(size, d, **kw):
    near = NEAR if d else 0
    return dict(d=d, near=near, tie=size - near, **kw)


# (a) per path and k: cap 64 / 160 with levels, 256 / 640 in the single pass.  Each class is one more than one of these or about five
# times one (321 = 5 x 64 + 1; 3 201 = 5 x 640 + 1 = 20 x 160 + 1 = 12.5 x 256 + 1): every (path, k) finds its ``cap + 1`` and a multiple
SCAN_SIZES = [(65, 9), (161, 0), (257, 9), (321, 0), (641, 9), (3201, 9)]
SCAN_SIZES_NPHD = [(65, 9), (161, 0), (257, 9), (641, 9), (3201, 9)]      # all in the 16-byte segment, which holds a third of the other rows
SCAN_FORMS = {
    # name: (code bytes, key words, keys)
    "b8k1": (8, 1, "small"),
    "b8k2": (8, 2, "few_assets"),
    "b13k1": (13, 1, "spread"),
    "b16k2": (16, 2, {"pattern": "one_asset", "hi": TOP_BIT_ASSET}),
    "b24k1": (24, 1, "high"),
    "b32k2": (32, 2, {"pattern": "one_asset", "hi": ALL_ONES}),
    "nphd": ((8, 16, 32), 1, "small"),
}
SCAN_BATCHES = [
    # queries, k, an all-zero query among them
    (3, 4, False),
    (8, 10, False),
    (9, 4, False),          # 64-bit codes: mfma_pack_kernel
    (130, 10, False),       # 64-bit codes: mfma_pack3_kernel
    (9, 10, True),          # 64-bit codes: the unpacked kernel
]
# the paths of tests/test_gpu_thresholds.py::PATHS -> whether Batch::reserve raises the buffer to 64 k for their top-k searches
SINGLE_PASS = {"xor8": False, "xor16": False, "mfma_levels": False, "mfma_single": True}
SCAN_ROWS = 5003                        # no multiple of 64, 128 or 192
RADIX_ROWS = 70_001                     # above fix_query's floor of 65 536 collected rows
RADIX_TABLES = {
    "radix_high": (1, "high"),
    "radix_asset": (2, {"pattern": "one_asset", "hi": TOP_BIT_ASSET}),
    "radix_ones": (2, {"pattern": "one_asset", "hi": ALL_ONES}),
}
SELECT_TABLES = {
    # (d): name: (code bytes, key words, keys)
    "sel_b8k2_high": (8, 2, "high"),
    "sel_b8k2_few": (8, 2, "few_assets"),
    "sel_b32k2_spread": (32, 2, "spread"),
    "sel_b32k2_few": (32, 2, "few_assets"),
    "sel_b13k1_high": (13, 1, "high"),
    "sel_b13k1_spread": (13, 1, "spread"),
}
BOUNDARY_K, BOUNDARY_WIDE_K = 4, 65
BOUNDARY_WIDE_CAP = 16 * BOUNDARY_WIDE_K        # 1 040: option candidate_cap of the second boundary pair, so that 16 k does not move cap
DOCFREQ_TABLES = {
    # (g): name: (rows, class size, keys); dup_limit 25 -> cap 400 < 450, dup_limit 1 000 -> cap 16 000 < 17 000
    "df_few_450": (5003, 450, "few_assets"),
    "df_ones_450": (5003, 450, {"pattern": "one_asset", "hi": ALL_ONES}),
    "df_few_17000": (20_003, 17_000, "few_assets"),
    "df_ones_17000": (20_003, 17_000, {"pattern": "one_asset", "hi": ALL_ONES}),
}
DOCFREQ_LIMIT = {"df_few_450": 25, "df_ones_450": 25, "df_few_17000": 1000, "df_ones_17000": 1000}


def _seed(name):
    return [ord(c) for c in name]


@functools.lru_cache(maxsize=None)
def case(name):
    # type: (str) -> Case
    rng = np.random.default_rng(_seed(name))
    if name.startswith("scan_"):
        nbytes, key_words, keys = SCAN_FORMS[name[5:]]
        if name == "scan_nphd":
            return planted(rng, SCAN_ROWS, nbytes, key_words, keys, [_cls(s, d, seg=16, qbytes=16) for s, d in SCAN_SIZES_NPHD])
        return planted(rng, SCAN_ROWS, nbytes, key_words, keys, [_cls(s, d) for s, d in SCAN_SIZES])
    if name == "boundary":
        # (b) radius 9 admits exactly cap and cap + 1 rows: 64 | 65 under candidate_cap 64 with k = 4, 1 040 | 1 041 under candidate_cap 1 040 with k = 65
        return planted(rng, SCAN_ROWS, 16, 1, "spread", [_cls(s, 9) for s in (CANDIDATE_CAP, CANDIDATE_CAP + 1, BOUNDARY_WIDE_CAP, BOUNDARY_WIDE_CAP + 1)])
    if name in RADIX_TABLES:
        key_words, keys = RADIX_TABLES[name]
        return planted(rng, RADIX_ROWS, 16, key_words, keys, [dict(d=9, near=0, tie=RADIX_ROWS)])
    if name in SELECT_TABLES:
        nbytes, key_words, keys = SELECT_TABLES[name]
        return planted(rng, SCAN_ROWS, nbytes, key_words, keys, [_cls(3003, 9)])
    if name == "nphd_one":
        # (e) three hot queries of 8, 16 and 32 bytes, each with ONE class, in the 16-byte segment
        return planted(rng, SCAN_ROWS, (8, 16, 32), 1, "spread", [_cls(300, 9, seg=16, qbytes=8), _cls(300, 0, seg=16, qbytes=16), _cls(300, 9, seg=16, qbytes=32)])
    if name == "nphd_two":
        # ... and each with TWO: in the 16-byte and in the 32-byte segment
        return planted(rng, SCAN_ROWS, (8, 16, 32), 1, "high",
                       [_cls(300, 9, seg=16, qbytes=32, hot=0), _cls(300, 9, seg=32, qbytes=32, hot=0),
                        _cls(300, 9, seg=16, qbytes=16, hot=1), _cls(300, 0, seg=32, qbytes=16, hot=1),
                        _cls(300, 9, seg=16, qbytes=8, hot=2), _cls(300, 9, seg=32, qbytes=8, hot=2)])
    if name == "healthy":
        return planted(rng, 2003, 8, 1, "small", [])
    if name in DOCFREQ_TABLES:
        n, size, keys = DOCFREQ_TABLES[name]
        return planted(rng, n, 16, 2, keys, [_cls(size, 0)])
    raise KeyError(name)


def halves(c):
    # type: (Case) -> tuple
    """The rows of a fixed-length case as two tables of alternate rows: ((keys, words), (keys, words))."""
    return (c.keys[0::2], c.words[0::2]), (c.keys[1::2], c.words[1::2])


def async_flagged(c, k, cap):
    # type: (Case, int, int) -> set
    """Hot queries of a fixed-length case for which one of ``halves(c)`` holds more than ``cap`` rows within the query's k-th distance over that half."""
    out = set()
    for h in range(len(c.hot)):
        d = c.dist(*c.hot_query(h))
        for half in (d[0::2], d[1::2]):
            ds = np.sort(half)
            if int((ds <= ds[min(k, len(ds)) - 1]).sum()) > cap:
                out.add(h)
    return out


def overflowing(c, cap):
    # type: (Case, int) -> list[int]
    """Hot queries of a case whose every class outgrows ``cap``: the one-past-the-buffer class first, then the largest, then the rest."""
    hots = sorted({cl["hot"] for cl in c.classes if all(x["near"] + x["tie"] > cap for x in c.classes if x["hot"] == cl["hot"])},
                  key=lambda h: min(x["near"] + x["tie"] for x in c.classes if x["hot"] == h))
    return hots[:1] + hots[-1:] + hots[1:-1] if len(hots) > 2 else hots


def hot_positions(nq):
    # type: (int) -> list[int]
    """Where a batch of ``nq`` queries holds its hot ones: first, last, and either side of the edges of the 8-, 16-, 32- and 128-query groups."""
    return sorted({0, nq - 1} | {p for p in (7, 8, 15, 16, 31, 32, 127, 128) if p < nq})


def quiet_queries(c, rng, count, lengths, ks=KS, cap=CANDIDATE_CAP):
    # type: (Case, np.random.Generator, int, tuple, tuple, int) -> tuple
    """
    ``count`` random queries (words [count, W], bytes [count]) that no search over this case flags: for every k in ``ks`` and every
    segment, the rows within the query's own k-th distance fit ``cap``, the smallest buffer -- redrawn until they do.
    """
    W = c.max_words
    out_w, out_b = np.zeros((count, W), dtype=U64), np.zeros(count, dtype=np.uint8)
    for i in range(count):
        qb = int(lengths[i % len(lengths)])
        for _ in range(256):
            q = rng.integers(0, 2**64, size=W, dtype=U64) & tm.prefix_masks(qb, W)
            if q.any() and all(max(c.listed(q, qb, k).values()) <= cap for k in ks):
                break
        else:
            raise RuntimeError("no quiet query found")
        out_w[i], out_b[i] = q, qb
    return out_w, out_b


class Batch:
    """Queries of one call: ``q`` [nq, W], ``qn`` (None: fixed length), the positions of the hot ones and which hot query each holds."""

    def __init__(self, c, q, qb, hot_at):
        self.q, self.qb, self.hot_at = q, qb, hot_at
        self.qn = qb.copy() if c.metric == METRIC_NPHD else None
        self.nq = len(q)
        for a in (self.q, self.qb):
            a.setflags(write=False)

    def quiet(self):
        return [i for i in range(self.nq) if i not in self.hot_at]


@functools.lru_cache(maxsize=None)
def scan_batch(name, nq, cap, zero=False):
    # type: (str, int, int, bool) -> Batch
    """
    (a) ``nq`` queries over case ``name``: at ``hot_positions(nq)`` the hot queries whose class outgrows ``cap``, in turn; everywhere else
    quiet random queries.  ``zero``: one quiet query is all zeros instead (64-bit batches then stay off the packed kernels).
    """
    c = case(name)
    rng = np.random.default_rng(_seed(name) + [nq, cap, int(zero)])
    hots = overflowing(c, cap)
    assert hots, "no class of this case outgrows the buffer"
    lengths = (16,) if c.metric == METRIC_NPHD else (c.max_bytes,)
    q, qb = quiet_queries(c, rng, nq, lengths)
    hot_at = {}
    for j, p in enumerate(hot_positions(nq)):
        h = hots[j % len(hots)]
        q[p], qb[p] = c.hot_query(h)
        hot_at[p] = h
    if zero:
        p = next(i for i in range(nq) if i not in hot_at)
        q[p] = 0
    return Batch(c, q, qb, hot_at)


@functools.lru_cache(maxsize=None)
def mixed_batch(name, nq):
    # type: (str, int) -> Batch
    """(c) - (g): the hot queries of case ``name`` spread evenly over ``nq`` queries (first and last among them), quiet ones of every row length between."""
    c = case(name)
    rng = np.random.default_rng(_seed(name) + [nq, 77])
    n_hot = len(c.hot)
    assert nq >= n_hot
    lengths = tuple(c.segments()) if c.metric == METRIC_NPHD else (c.max_bytes,)
    q, qb = quiet_queries(c, rng, nq, lengths, cap=CANDIDATE_CAP if c.n < RADIX_ROWS else 1 << 30)
    hot_at = {}
    for h in range(n_hot):
        p = 0 if n_hot == 1 else (h * (nq - 1)) // (n_hot - 1)
        q[p], qb[p] = c.hot_query(h)
        hot_at[p] = h
    return Batch(c, q, qb, hot_at)


# ---------------------------------------------------------------------------------------------------------------------------------
# expected results, from the oracle alone
# ---------------------------------------------------------------------------------------------------------------------------------
def expect_topk(keys, words, lens, metric, max_bytes, q, qn, k):
    from oracle import oracle_topk

    return oracle_topk(metric, keys, words, lens, q, qn, k, fixed_nbytes=0 if metric == METRIC_NPHD else max_bytes)


def expect_within(keys, words, lens, metric, max_bytes, q, qn, k, radius):
    """``HipTable.search_within``'s four arrays by ``oracle.np_within``, zeros past every count."""
    from oracle import np_within

    nq = len(q)
    kshape = (nq, k, 2) if keys.ndim == 2 else (nq, k)
    out = (np.zeros(kshape, np.uint64), np.zeros((nq, k), np.uint32), np.zeros((nq, k), np.uint16), np.zeros(nq, np.uint32))
    for i in range(nq):
        kk, h, p = np_within(words, max_bytes if lens is None else lens, keys, q[i], max_bytes if metric == METRIC_HAMMING else int(qn[i]), k, radius)
        cnt = len(h)
        out[0][i, :cnt], out[1][i, :cnt], out[2][i, :cnt], out[3][i] = kk, h, p, cnt
    return out


def expect(c, b, k, radius=None):
    # type: (Case, Batch, int, int | None) -> tuple
    if radius is None:
        return expect_topk(c.keys, c.words, c.lens, c.metric, c.max_bytes, b.q, b.qn, k)
    return expect_within(c.keys, c.words, c.lens, c.metric, c.max_bytes, b.q, b.qn, k, radius)


def doc_freq_of(c, q_words, dup_limit):
    # type: (Case, np.ndarray, int) -> tuple
    """(distinct first key words, rows) among the first ``dup_limit`` rows EQUAL to one code of a fixed-length case, by ascending key."""
    equal = np.nonzero((c.words == np.asarray(q_words, dtype=U64)).all(axis=1))[0]
    kk = c.keys[equal]
    order = np.lexsort((kk[:, 1], kk[:, 0])) if kk.ndim == 2 else np.argsort(kk)
    first = kk[order][:dup_limit]
    assets = first[:, 0] if kk.ndim == 2 else first
    return len(np.unique(assets)), len(first)


# ---------------------------------------------------------------------------------------------------------------------------------
# (h) simprint corpora: chunks (16-byte key = asset | offset | size, big-endian; one simprint each) with "hot" simprints stored thousands of times
# ---------------------------------------------------------------------------------------------------------------------------------
SIMPRINT_LIMIT, SIMPRINT_THRESHOLD, SIMPRINT_OVERSAMPLING = 20, 0.9, 2
SIMPRINT_COUNT = SIMPRINT_LIMIT * SIMPRINT_OVERSAMPLING       # neighbours asked per query simprint: 40
SIMPRINT_DUP_LIMIT = 1000               # rows the document-frequency scan of a scoring request looks at (the product's DOC_FREQ_DUP_LIMIT)
LOOKUPS_PER_BATCH = 1024                # queries one batch of the search pipeline takes
HOT_FLIPS = 5                           # the distance of a hot simprint's chunks that do not equal it
# kind: (bits, per hot simprint (chunks equal to it, chunks at distance 5), assets that hold each, ordinary chunks, ordinary simprints)
SIMPRINT_CORPORA = {
    64: (64, [(2_700, 300), (30, 2_970)], 600, 2_003, 1_200),
    128: (128, [(2_700, 300), (30, 2_970)], 600, 2_003, 1_200),
    256: (256, [(2_700, 300), (30, 2_970)], 600, 2_003, 1_200),
    # one simprint in 17 003 equal chunks, five per asset: more than the 16 000 rows the collision scan of dup_limit 1 000 buffers
    "big": (64, [(17_003, 0)], 3_400, 2_000, 500),
}


def _flip_first_bits(data, n):
    out = bytearray(data)
    for b in range(n):
        out[b // 8] ^= 1 << (7 - b % 8)
    return bytes(out)


class SimprintCorpus:
    """``keys`` (16 bytes each) and ``vecs`` uint8 [chunks, bytes] as ``HipSimprintIndex.add_raw`` takes them; ``hot`` and ``pool`` simprints as bytes."""

    def __init__(self, kind):
        import struct

        ndim, hot_plan, assets_per_hot, ordinary, pool_size = SIMPRINT_CORPORA[kind]
        rng = np.random.default_rng(_seed(f"simprints {kind}"))
        nb = ndim // 8
        self.kind, self.ndim, self.nb, self.hot_plan = kind, ndim, nb, hot_plan
        hot = [rng.integers(0, 256, size=nb, dtype=np.uint8) for _ in hot_plan]
        self.pool = [bytes(r) for r in np.unique(rng.integers(0, 256, size=(pool_size, nb), dtype=np.uint8), axis=0)]
        ids = [0, ALL_ONES] + list(range(1, assets_per_hot - 1))        # the asset ids 0 and all ones among them
        pointer = lambda asset, offset, size: asset.to_bytes(8, "big") + struct.pack("!II", offset, size)
        self.keys, vecs = [], []
        for which, (code, (equal, away)) in enumerate(zip(hot, hot_plan)):
            flips = iter(flip_bytes(rng, away, HOT_FLIPS, nb))
            at_zero = set(rng.choice(equal + away, size=equal, replace=False).tolist())
            for slot in range(equal + away):
                asset, c = ids[slot % assets_per_hot], slot // assets_per_hot
                self.keys.append(pointer(asset, which * 1_000_000 + c * 10, 10 + c))
                vecs.append(code if slot in at_zero else code ^ next(flips))
        for i in range(ordinary):
            self.keys.append(pointer(10_000 + i % 400, 5_000_000 + i, 7))
            vecs.append(np.frombuffer(_flip_first_bits(self.pool[i % len(self.pool)], i % 3 if i >= len(self.pool) else 0), dtype=np.uint8))
        self.vecs = np.stack(vecs)
        self.vecs.setflags(write=False)
        self.hot = [bytes(h) for h in hot]
        self.total_assets = assets_per_hot + 400
        assert len(set(self.keys)) == len(self.keys)

    def dist(self, simprint):
        # type: (bytes) -> np.ndarray
        """Hamming distance of one simprint to the simprint of every chunk: int64 [chunks]."""
        return np.unpackbits(self.vecs ^ np.frombuffer(simprint, dtype=np.uint8), axis=1).sum(axis=1, dtype=np.int64)

    def h_max(self):
        """The largest distance whose score 1 - d / bits passes the match threshold."""
        return max(d for d in range(self.ndim + 1) if 1.0 - d / self.ndim >= SIMPRINT_THRESHOLD)

    def ordinary(self, n):
        """``n`` query simprints 0 - 2 bits away from ordinary stored ones."""
        return [_flip_first_bits(self.pool[i], i % 3) for i in range(n)]

    def raw_requests(self):
        """The hot simprints first, last, and in the middle of 30 ordinary ones (the big corpus: its one hot simprint among 10)."""
        if self.kind == "big":
            return [self.ordinary(5) + self.hot + self.ordinary(10)[5:]]
        (a, b), plain = self.hot, self.ordinary(30)
        return [[a, b] + plain, plain + [b, a], plain[:15] + [a] + plain[15:] + [b]]

    def many_requests(self):
        """Hot and ordinary requests that fit one round of a many-request call."""
        (a, b), plain = self.hot, self.ordinary(30)
        return [[a] + plain[:10], plain[10:22], [b, a], plain[:3]]

    def exact_given(self, form):
        """Simprints as given to a hard-boundary search, hot ones repeated: ``one batch`` of distinct lookups, or ``two batches``."""
        absent = bytes(range(1, self.nb + 1))
        if self.kind == "big":
            assert form == "one batch"
            return self.hot + self.pool[:130] + self.hot
        a, b = self.hot
        return [a] + self.pool[:140] + [b, absent, a] if form == "one batch" else [a, b] + self.pool[:1100] + [a]


@functools.lru_cache(maxsize=None)
def simprint_corpus(kind):
    return SimprintCorpus(kind)
