"""
Constructed mixed-length NPHD tables and an exact host model of the search over them (numpy + ``fractions`` only; nothing of the
engine or of ``oracle/`` is imported here).

On uniformly random codes the shortest compared prefix always wins a top-k list, so the rank table, the merge of the
per-segment lists and the ratio speculation never meet an input that decides them.  The tables built here do:

    sweep table       one row for every byte length p in 1..32 and every h in 0..4p, at distance exactly h from a query Q over its
                      first 8p bits (and 8p - h from ~Q): every fraction of the rank table, and tie classes that span all 32 lengths
    clustered table   rows of 3 / 8 / 13 / 16 / 24 / 32 bytes around seeded centres, h / (8p) spread alike at every length, so
                      that the lists of a query interleave the lengths
    hint scenarios    the clustered table plus planted rows that put a batch's worst k-th NPHD exactly where the verdict of the
                      ratio speculation changes (``MHintModel``)

``model_topk`` is brute force over every row: p = min(row bytes, query bytes), h = popcount over the first 8p bits, order by
(Fraction(h, 8p), key).  The fractions are compared through ``model_rank``, their dense rank among ALL fractions h' / (8p'),
which is computed with ``Fraction`` here and is what the engine's 33 x 257 ``dist_rank`` table must hold.
tests/test_nphd_cases.py holds this file to the oracle, tests/test_gpu_nphd_mixed.py holds the engine to this file.
"""

import functools
from fractions import Fraction

import numpy as np

MAX_BYTES = 32
SWEEP_ROWS = sum(4 * p + 1 for p in range(1, MAX_BYTES + 1))     # 2 144
CLUSTER_LENGTHS = (3, 8, 13, 16, 24, 32)
CLUSTER_QUERY_LENGTHS = (4, 8, 13, 16, 24, 32)
MARGIN = Fraction(1, 32)        # the speculation's margin above the hint
DECAY = Fraction(1, 256)        # what a hit takes off the hint at most

_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# codes as bytes: uint8 [n, 32], zero beyond each row's length; bit i of a code is bit 7 - i % 8 of byte i // 8
# ---------------------------------------------------------------------------------------------------------------------
def to_words(code_bytes):
    # type: (np.ndarray) -> np.ndarray
    """uint8 [n, 32] -> uint64 [n, 4], big-endian packed (the C-ABI layout)."""
    b = np.ascontiguousarray(code_bytes, dtype=np.uint8).reshape(-1, 4, 8)
    return b.view(">u8").reshape(-1, 4).astype(np.uint64)


def to_bytes(words):
    # type: (np.ndarray) -> np.ndarray
    """uint64 [n, 4] -> uint8 [n, 32]."""
    w = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, 4)
    return w.astype(">u8").view(np.uint8).reshape(-1, 32)


def flipped(code, positions):
    # type: (np.ndarray, np.ndarray | list) -> np.ndarray
    """A copy of the 32-byte code with the given bit positions flipped."""
    out = np.array(code, dtype=np.uint8)
    for i in positions:
        out[int(i) // 8] ^= np.uint8(0x80 >> (int(i) % 8))
    return out


def truncated(code, nbytes):
    # type: (np.ndarray, int) -> np.ndarray
    out = np.array(code, dtype=np.uint8)
    out[nbytes:] = 0
    return out


def keys_as_ints(keys):
    # type: (np.ndarray) -> list
    """uint64 [n] or [n, 2] (hi, lo) -> Python ints."""
    keys = np.asarray(keys, dtype=np.uint64)
    if keys.ndim == 2:
        return [(int(hi) << 64) | int(lo) for hi, lo in keys]
    return [int(x) for x in keys]


# ---------------------------------------------------------------------------------------------------------------------
# the exact model
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rank_fractions():
    """Every distinct fraction h / (8p), ascending: position = dense rank."""
    return tuple(sorted({Fraction(h, 8 * p) for p in range(1, MAX_BYTES + 1) for h in range(8 * p + 1)}))


@functools.lru_cache(maxsize=None)
def _rank_table():
    index = {f: i for i, f in enumerate(_rank_fractions())}
    table = np.full((MAX_BYTES + 1, 8 * MAX_BYTES + 1), len(index), dtype=np.int64)
    for p in range(1, MAX_BYTES + 1):
        for h in range(8 * p + 1):
            table[p, h] = index[Fraction(h, 8 * p)]
    table.setflags(write=False)
    return table


def model_rank(p, h):
    # type: (int, int) -> int
    """Dense rank of h / (8p) among all fractions h' / (8p') with p' in 1..32 and 0 <= h' <= 8p'."""
    if not (1 <= p <= MAX_BYTES and 0 <= h <= 8 * p):
        raise ValueError(f"no fraction {h} / (8 * {p})")
    return int(_rank_table()[p, h])


def batch_distances(rows, lens, q_bytes, qlen):
    # type: (np.ndarray, np.ndarray, np.ndarray, int) -> tuple
    """
    (h int64 [nq, n], p int64 [n]) of queries of ONE byte length against rows given as bytes (uint8 [n, 32]):
    p = min(row bytes, query bytes), h the popcount over the first 8p bits.
    """
    p = np.minimum(np.asarray(lens, dtype=np.int64), int(qlen))
    q_bytes = np.asarray(q_bytes, dtype=np.uint8).reshape(-1, 32)
    h = np.empty((q_bytes.shape[0], rows.shape[0]), dtype=np.int64)
    for i in range(0, q_bytes.shape[0], 16):
        cum = np.cumsum(_POP8[rows[None, :, :] ^ q_bytes[i : i + 16, None, :]].astype(np.int16), axis=2, dtype=np.int16)
        h[i : i + 16] = np.take_along_axis(cum, np.broadcast_to((p - 1)[None, :, None], (cum.shape[0], cum.shape[1], 1)), axis=2)[:, :, 0]
    return h, p


def prefix_distances(words, lens, q_bytes, qlen):
    # type: (np.ndarray, np.ndarray, np.ndarray, int) -> tuple
    """(h [n], p [n]) of one query (a 32-byte code as uint8) against packed rows."""
    h, p = batch_distances(to_bytes(words), lens, q_bytes, qlen)
    return h[0], p


def model_topk(keys, words, lens, q, qlen, k, radius=None):
    # type: (np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray | int, int, int | None) -> tuple
    """
    Exact top-k of every query, brute force: (keys [nq, k(, 2)], hamming uint32 [nq, k], prefix_bits uint16 [nq, k], count uint32 [nq]),
    zeros beyond a query's count.  ``radius``: only rows whose Hamming distance over the compared prefix is <= radius bits
    (the absolute count, whatever the prefix length) are eligible.
    """
    keys = np.asarray(keys, dtype=np.uint64)
    q = np.ascontiguousarray(q, dtype=np.uint64).reshape(-1, 4)
    qlens = np.broadcast_to(np.asarray(qlen, dtype=np.int64), (q.shape[0],))
    # (a batch that repeats queries is answered once per distinct (query, length))
    distinct, inverse = np.unique(np.concatenate([q, qlens[:, None].astype(np.uint64)], axis=1), axis=0, return_inverse=True)
    if len(distinct) < q.shape[0]:
        return tuple(a[inverse.reshape(-1)] for a in model_topk(keys, words, lens, distinct[:, :4], distinct[:, 4].astype(np.int64), k, radius))
    rows, q_bytes = to_bytes(words), to_bytes(q)
    nq, n = q_bytes.shape[0], rows.shape[0]
    two = keys.ndim == 2
    out_k = np.zeros((nq, k, 2) if two else (nq, k), dtype=np.uint64)
    out_h = np.zeros((nq, k), dtype=np.uint32)
    out_p = np.zeros((nq, k), dtype=np.uint16)
    out_c = np.zeros(nq, dtype=np.uint32)
    table = _rank_table()
    beyond = len(_rank_fractions())         # the rank of a row that is not eligible
    for length in np.unique(qlens):
        which = np.nonzero(qlens == length)[0]
        h_all, p = batch_distances(rows, lens, q_bytes[which], int(length))
        for i, h in zip(which, h_all):
            rank = table[p, h]
            if radius is not None:
                rank = np.where(h <= radius, rank, beyond)
            # every row at or under the k-th smallest rank, then the exact order (rank, key) among those
            cut = np.partition(rank, k - 1)[k - 1] if k < n else beyond
            cand = np.nonzero((rank <= cut) & (rank < beyond))[0]
            ck = keys[cand]
            order = cand[np.lexsort((ck[:, 1], ck[:, 0], rank[cand])) if two else np.lexsort((ck, rank[cand]))][:k]
            c = len(order)
            out_k[i, :c], out_h[i, :c], out_p[i, :c], out_c[i] = keys[order], h[order], 8 * p[order], c
    return out_k, out_h, out_p, out_c


def kth_ratios(result, k):
    # type: (tuple, int) -> list
    """Per query the NPHD of its k-th row as a Fraction, None where the list holds fewer than k rows."""
    _, ham, pbits, cnt = result
    return [Fraction(int(ham[i, k - 1]), int(pbits[i, k - 1])) if cnt[i] >= k else None for i in range(len(cnt))]


# ---------------------------------------------------------------------------------------------------------------------
# keys unrelated to the rows they name
# ---------------------------------------------------------------------------------------------------------------------
def scattered_keys(rng, n, key_words):
    # type: (np.random.Generator, int, int) -> np.ndarray
    """
    n distinct keys in seeded random order.  One word: 0, 2^64 - 1, values around 2^63 and small ones.  Two words: the same values
    as ``lo`` under a ``hi`` word that many rows share (0, 1, 2^63, 2^64 - 1), so that the order within a ``hi`` is decided by ``lo``.
    """
    top = np.uint64(1) << np.uint64(63)
    third = n // 3
    lo = np.concatenate([np.arange(third, dtype=np.uint64), top - np.uint64(third // 2) + np.arange(third, dtype=np.uint64),
                         np.uint64(0xFFFFFFFFFFFFFFFF) - np.arange(n - 2 * third, dtype=np.uint64)])
    assert len(np.unique(lo)) == n and lo.min() == 0 and lo.max() == np.uint64(0xFFFFFFFFFFFFFFFF) and (lo >= top).sum() > n // 3
    lo = rng.permutation(lo)
    if key_words == 1:
        return lo
    hi = rng.choice(np.array([0, 1, 1 << 63, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64), size=n)
    return np.stack([hi, lo], axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# the sweep table
# ---------------------------------------------------------------------------------------------------------------------
class Sweep:
    """keys, words [n, 4], lens [n], the query code ``Q`` (uint8 [32]) and per row its (p, h)."""

    def __init__(self, keys, words, lens, Q, p, h):
        self.keys, self.words, self.lens, self.Q, self.p, self.h = keys, words, lens, Q, p, h
        for a in (keys, words, lens, Q, p, h):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def sweep_table(key_words=1, seed=20240):
    # type: (int, int) -> Sweep
    """
    For every p in 1..32 and h in 0..4p one row: Q's first p bytes with exactly h seeded bit positions among the first 8p flipped,
    zero beyond.  Rows in seeded random order, keys unrelated to (p, h).
    """
    rng = np.random.default_rng(seed)
    Q = rng.integers(0, 256, size=32, dtype=np.uint8)
    rows, ps, hs = [], [], []
    for p in range(1, MAX_BYTES + 1):
        for h in range(4 * p + 1):
            rows.append(truncated(flipped(Q, rng.choice(8 * p, size=h, replace=False)), p))
            ps.append(p)
            hs.append(h)
    order = rng.permutation(len(rows))
    rows, ps, hs = np.array(rows, dtype=np.uint8)[order], np.array(ps, dtype=np.int64)[order], np.array(hs, dtype=np.int64)[order]
    assert len(rows) == SWEEP_ROWS
    return Sweep(scattered_keys(rng, len(rows), key_words), to_words(rows), ps.astype(np.uint8), Q, ps, hs)


def sweep_queries(Q, seed=7):
    # type: (np.ndarray, int) -> tuple
    """(words [9, 4], lens [9]): Q, ~Q, Q cut to 4 / 8 / 13 / 16 / 24 bytes, Q with 3 and ~Q with 5 seeded bits flipped."""
    rng = np.random.default_rng(seed)
    codes = [(Q, 32), (~Q, 32)] + [(truncated(Q, b), b) for b in (4, 8, 13, 16, 24)]
    codes += [(flipped(Q, rng.choice(256, size=3, replace=False)), 32), (flipped(~Q, rng.choice(256, size=5, replace=False)), 32)]
    return to_words(np.array([c for c, _ in codes], dtype=np.uint8)), np.array([b for _, b in codes], dtype=np.uint8)


def sweep_queries_many(Q, nq, nbytes, seed=11):
    # type: (np.ndarray, int, int, int) -> tuple
    """``nq`` queries of ONE length: Q and ~Q cut to ``nbytes``, then each of them with 1..6 seeded bits inside the length flipped."""
    rng = np.random.default_rng(seed + nbytes)
    codes = [truncated(Q, nbytes), truncated(~Q, nbytes)]
    while len(codes) < nq:
        base = codes[len(codes) % 2]
        codes.append(flipped(base, rng.choice(8 * nbytes, size=int(rng.integers(1, 7)), replace=False)))
    return to_words(np.array(codes, dtype=np.uint8)), np.full(nq, nbytes, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# the clustered table
# ---------------------------------------------------------------------------------------------------------------------
class Clustered:
    """keys, words [n, 4], lens [n] and the centres (uint8 [C, 32])."""

    def __init__(self, keys, words, lens, centres):
        self.keys, self.words, self.lens, self.centres = keys, words, lens, centres
        for a in (keys, words, lens, centres):
            a.setflags(write=False)


def _cluster_rows(rng, centres, per_centre, random_rows):
    rows, lens = [], []
    for p in CLUSTER_LENGTHS:
        bits = 8 * p
        for c in centres:
            # stratified over [0, 0.3]: the same spread of h / (8p) at every length, and every length holds the centre's own prefix
            for j in range(per_centre):
                h = int(round(0.3 * bits * (j + rng.random()) / per_centre)) if j else 0
                rows.append(truncated(flipped(c, rng.choice(bits, size=h, replace=False)), p))
                lens.append(p)
        rnd = rng.integers(0, 256, size=(random_rows, 32), dtype=np.uint8)
        rnd[:, p:] = 0
        rows.extend(rnd)
        lens.extend([p] * random_rows)
    return np.array(rows, dtype=np.uint8), np.array(lens, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def clustered_table(key_words=1, seed=31337, n_centres=40, per_centre=50, random_rows=500):
    # type: (int, int, int, int, int) -> Clustered
    """Six segments of n_centres x per_centre + random_rows (2 500) rows each, in seeded random order."""
    rng = np.random.default_rng(seed)
    centres = rng.integers(0, 256, size=(n_centres, 32), dtype=np.uint8)
    rows, lens = _cluster_rows(rng, centres, per_centre, random_rows)
    order = rng.permutation(len(rows))
    return Clustered(scattered_keys(rng, len(rows), key_words), to_words(rows[order]), lens[order], centres)


def clustered_queries(table, nq, seed=5, lengths=None):
    # type: (Clustered, int, int, tuple | None) -> tuple
    """
    (words [nq, 4], lens [nq]): centres with 0..3 seeded bits flipped, cut to the lengths of ``lengths`` in turn (default: of twelve
    queries six of 32 bytes, two of 24 and one each of 16, 13, 8 and 4 -- a query shorter than, equal to and longer than every row
    length).  The flipped bits lie where only the query's LONGEST compared prefix sees them (a 24-byte query: bits 128..191), so
    that the shorter prefixes tie at the centre's own rows and the longest one is set back by a few steps of its finer grid.  A
    16-byte query meets exactly four compared prefixes (24 / 64 / 104 / 128 bits); for its ten nearest rows to hold all four it
    carries at most one flipped bit.
    """
    rng = np.random.default_rng(seed)
    lengths = lengths or (32, 16, 24, 32, 4, 32, 8, 32, 13, 32, 24, 32)
    codes, lens = [], []
    for i in range(nq):
        b = lengths[i % len(lengths)]
        c = table.centres[int(rng.integers(0, len(table.centres)))]
        below = 8 * max([x for x in CLUSTER_LENGTHS if x < b], default=0)       # bits that a shorter compared prefix sees too
        flips = below + rng.choice(8 * b - below, size=int(rng.integers(0, 2 if b == 16 else 4)), replace=False)
        codes.append(truncated(flipped(c, flips), b))
        lens.append(b)
    return to_words(np.array(codes, dtype=np.uint8)), np.array(lens, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# the hint of a table of several code lengths
# ---------------------------------------------------------------------------------------------------------------------
def size_class(m):
    # type: (int) -> int
    """Batches of 1 | 2-3 | 4-7 | ... queries keep a hint each."""
    return int(m).bit_length()


def length_class(nbytes):
    # type: (int) -> int
    """... and so do the query lengths 8 / 16 / 24 / 32 bytes; every other length shares one."""
    return nbytes // 8 if nbytes % 8 == 0 and 8 <= nbytes <= 32 else 0


class MHintModel:
    """
    The multi-segment (ratio) speculation as its comments state it, in exact arithmetic.

    One hint per (size class, length class).  A batch that finds no usable hint (none yet, another k, or backed off) takes the
    ordinary path and SEEDS the hint with its worst k-th NPHD.  Otherwise every segment lists, per query, its rows within
    floor((ratio + 1/32) x compared bits + 1e-9) bits, each list is cut to its k best, the lists are merged, and the step STANDS iff
    no list overflowed, every query has k rows and the worst k-th NPHD is <= ratio + 1/32.  A hit leaves
    ratio = max(worst, ratio - 1/256); a miss answers the batch by the ordinary path, re-seeds the hint with the true worst and backs
    off: after the n-th miss in a row the next 2^n - 2 batches of the class (at most 14) do not speculate.

    ``step`` returns the verdict as the (spec_hits, spec_misses) delta the batch must show.
    """

    def __init__(self, keys, words, lens, list_cap=16384):
        self.keys, self.words, self.lens, self.list_cap = keys, words, np.asarray(lens, dtype=np.int64), list_cap
        self.rows = to_bytes(words)
        self.hints = {}

    class Hint:
        def __init__(self):
            self.k, self.ratio, self.skip, self.penalty = 0, Fraction(0), 0, 0

    def hint(self, m, qlen):
        return self.hints.setdefault((size_class(m), length_class(qlen)), MHintModel.Hint())

    def radius_bits(self, bound, bits):
        # type: (Fraction, int) -> int
        return min(bits, int(bound * bits + Fraction(1, 10**9)))      # (floor: the operand is positive)

    def speculative_lists(self, q, qlen, k, bound):
        """(stands, worst k-th NPHD or None): the merged radius-limited lists of the batch under ``bound``."""
        h, p = batch_distances(self.rows, self.lens, np.unique(to_bytes(q), axis=0), qlen)
        radius = np.array([0] + [self.radius_bits(bound, 8 * b) for b in range(1, MAX_BYTES + 1)], dtype=np.int64)
        listed = h <= radius[p][None, :]
        for length in np.unique(self.lens):
            if (listed[:, self.lens == length].sum(axis=1) > self.list_cap).any():
                return False, None
        if (listed.sum(axis=1) < k).any():
            return False, None
        # (each segment's list is cut to its k best before the merge: the merged top k is the top k of the union either way)
        rank = np.where(listed, _rank_table()[p[None, :], h], len(_rank_fractions()))
        worst = _rank_fractions()[int(np.partition(rank, k - 1, axis=1)[:, k - 1].max())]
        return worst <= bound, worst

    def step(self, q, qlen, k, speculate=True):
        # type: (np.ndarray, int, int, bool) -> tuple
        m = np.asarray(q).reshape(-1, 4).shape[0]
        hint = self.hint(m, qlen)
        true_worst = max(kth_ratios(model_topk(self.keys, self.words, self.lens, q, qlen, k), k))     # (k <= rows: every list is full)
        ready = False
        if speculate and hint.k == k:
            if hint.skip:
                hint.skip -= 1
            else:
                ready = True
        if not ready:
            hint.k, hint.ratio = k, true_worst
            return (0, 0)
        stands, worst = self.speculative_lists(q, qlen, k, hint.ratio + MARGIN)
        if stands:
            assert worst == true_worst
            hint.penalty, hint.ratio = 0, max(worst, hint.ratio - DECAY)
            return (1, 0)
        hint.penalty = min(2 * hint.penalty + 1, 15)
        hint.skip = hint.penalty - 1
        hint.k, hint.ratio = k, true_worst
        return (0, 1)


# ---------------------------------------------------------------------------------------------------------------------
# hint scenarios: the clustered table + planted probes whose k-th row lies where the verdict changes
# ---------------------------------------------------------------------------------------------------------------------
PROBE_CLEAR_RATIO = Fraction(1, 5)      # no row that is not planted for a probe lies within this NPHD of it (5 / 24 is the nearest)


class Scenario:
    """keys, words, lens of the table; ``steps``: [(label, probe code or None, k, expected verdict)]; the centres for filler queries."""

    def __init__(self, keys, words, lens, steps, centres, qlen):
        self.keys, self.words, self.lens, self.steps, self.centres, self.qlen = keys, words, lens, steps, centres, qlen


# per query length: (label, k, bytes of the planted k-th row, its distance over the compared prefix, the verdict the rule gives)
# -- the arithmetic behind every line is spelled out in tests/test_nphd_cases.py::test_hint_scenarios_are_what_they_claim
SCENARIO_STEPS = {
    32: [
        ("seed 12/256", 10, 32, 12, (0, 0)),
        ("hit: 16/256 <= 12/256 + 8/256", 10, 32, 16, (1, 0)),
        ("boundary hit in the 256-bit segment: 24/256 == 16/256 + 8/256", 10, 32, 24, (1, 0)),
        ("boundary hit in the 64-bit segment: 8/64 == 24/256 + 8/256", 10, 8, 8, (1, 0)),
        ("miss one bit further out: 41/256 > 32/256 + 8/256", 10, 32, 41, (0, 1)),
        ("decay: a batch that ends far inside leaves 41/256 - 1/256", 10, None, None, (1, 0)),
        ("miss under the decayed hint only: 49/256 > 40/256 + 8/256", 10, 32, 49, (0, 1)),
        ("another k seeds anew: 11/192", 11, 24, 11, (0, 0)),
        ("boundary hit in the 192-bit segment: 17/192 == 11/192 + 6/192", 11, 24, 17, (1, 0)),
        ("miss: 24/192 > 17/192 + 6/192", 11, 24, 24, (0, 1)),
        ("another k seeds anew: 16/256", 12, 32, 16, (0, 0)),
        ("fractional radius, 24 bits: floor(24/256 x 24) = 2, the k-th at 2/24", 12, 3, 2, (1, 0)),
        ("one bit beyond floor((2/24 + 1/32) x 24) = 2: the k-th at 3/24", 12, 3, 3, (0, 1)),
    ],
    13: [
        ("seed 4/64", 10, 8, 4, (0, 0)),
        ("boundary hit in the 64-bit segment: 6/64 == 4/64 + 2/64", 10, 8, 6, (1, 0)),
        ("miss one bit further out: 9/64 > 6/64 + 2/64", 10, 8, 9, (0, 1)),
        ("decay: a batch that ends far inside leaves 9/64 - 1/256", 10, None, None, (1, 0)),
        ("miss under the decayed hint only: 11/64 > 35/256 + 8/256", 10, 8, 11, (0, 1)),
        ("another k seeds anew: 8/104", 11, 13, 8, (0, 0)),
        ("fractional radius, 104 bits: floor((8/104 + 1/32) x 104) = 11, the k-th at 11/104", 11, 13, 11, (1, 0)),
        ("one bit beyond floor((11/104 + 1/32) x 104) = 14: the k-th at 15/104 in a 16-byte row", 11, 16, 15, (0, 1)),
        ("another k seeds anew: 4/64", 12, 8, 4, (0, 0)),
        ("fractional radius, 24 bits: floor((4/64 + 1/32) x 24) = 2, the k-th at 2/24", 12, 3, 2, (1, 0)),
        ("one bit beyond floor((2/24 + 1/32) x 24) = 2: the k-th at 3/24", 12, 3, 3, (0, 1)),
    ],
}


@functools.lru_cache(maxsize=None)
def _clear_limits():
    """Per compared prefix p (bytes) the largest h with h / (8p) < PROBE_CLEAR_RATIO."""
    return np.array([0] + [max(h for h in range(8 * p + 1) if Fraction(h, 8 * p) < PROBE_CLEAR_RATIO) for p in range(1, MAX_BYTES + 1)])


def _clear_of(words, lens, code, qlen):
    """No row within PROBE_CLEAR_RATIO of ``code`` cut to the query length."""
    h, p = prefix_distances(words, lens, truncated(code, qlen), qlen)
    return not (h <= _clear_limits()[p]).any()


@functools.lru_cache(maxsize=None)
def hint_scenario(qlen, seed=909):
    # type: (int, int) -> Scenario
    """
    The clustered table plus, for every step of SCENARIO_STEPS[qlen] that plants one, a probe: a seeded code P far from every row, k - 1
    copies of its prefixes (rows of 8 / 16 / 24 / 32 bytes, distance 0) and ONE row of the step's byte length at the step's distance
    over the compared prefix, so that the probe's k-th NPHD is exactly that fraction: nothing else lies between the copies and
    PROBE_CLEAR_RATIO, so whatever key the planted row has it is the k-th row if its segment lists it -- and were that segment's
    radius one bit short, the probe would hold k - 1 rows.
    """
    base = clustered_table(1)
    rng = np.random.default_rng(seed + qlen)
    rows, lens, probes = [to_bytes(base.words)], [np.asarray(base.lens)], []
    planted_rows, planted_lens = [], []
    for label, k, row_bytes, h, verdict in SCENARIO_STEPS[qlen]:
        if row_bytes is None:
            probes.append(None)
            continue
        have_w = to_words(np.concatenate(rows + ([np.array(planted_rows, dtype=np.uint8)] if planted_rows else [])))
        have_l = np.concatenate(lens + [np.array(planted_lens, dtype=np.uint8)])
        while True:
            P = rng.integers(0, 256, size=32, dtype=np.uint8)
            if _clear_of(have_w, have_l, P, qlen):
                break
        for j in range(k - 1):
            b = (8, 16, 24, 32)[j % 4]
            planted_rows.append(truncated(P, b))
            planted_lens.append(b)
        compared = 8 * min(row_bytes, qlen)
        planted_rows.append(truncated(flipped(P, rng.choice(compared, size=h, replace=False)), row_bytes))
        planted_lens.append(row_bytes)
        probes.append(truncated(P, qlen))
    all_rows = np.concatenate(rows + [np.array(planted_rows, dtype=np.uint8)])
    all_lens = np.concatenate(lens + [np.array(planted_lens, dtype=np.uint8)])
    n_base, n_new = len(base.lens), len(planted_lens)
    # keys of the planted rows: outside the base table's (small, around 2^63, top) values and far from 0 and 2^64 - 1
    new_keys = np.uint64(1 << 40) + rng.permutation(n_new).astype(np.uint64)
    keys = np.concatenate([np.asarray(base.keys), new_keys])
    assert len(np.unique(keys)) == n_base + n_new
    steps = [(label, probe, k, verdict) for (label, k, _, _, verdict), probe in zip(SCENARIO_STEPS[qlen], probes)]
    return Scenario(keys, to_words(all_rows), all_lens, steps, base.centres, qlen)


def scenario_batch(sc, step_index, m, seed=77):
    # type: (Scenario, int, int, int) -> np.ndarray
    """Words [m, 4] of a step's batch: its probe (if it has one) LAST, in front of it exact centres cut to the query length."""
    rng = np.random.default_rng(seed + 1000 * step_index + m)
    probe = sc.steps[step_index][1]
    fill = m if probe is None else m - 1
    codes = [truncated(sc.centres[int(c)], sc.qlen) for c in rng.integers(0, len(sc.centres), size=fill)]
    if probe is not None:
        codes.append(probe)
    return to_words(np.array(codes, dtype=np.uint8))
