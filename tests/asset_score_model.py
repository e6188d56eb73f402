"""
Plain host model of ``HipEngine.match_assets`` (TEST INFRASTRUCTURE): the arguments of that call in, its six outputs out.

Independent of the HIP library and of ``iscc_search_amd.unit_match``: the neighbour lists are brute force over the rows the
test itself added (``ModelTable``), ordered by exact integer arithmetic; the scoring is Python dicts in insertion order and
Python floats, as ``iscc_search/indexes/usearch/index.py:786-839`` runs it for one query.  Nothing here is fast; the lists are
NumPy, only the aggregation loops in Python.
"""

import math
import sys

import numpy as np

MAX_BYTES = 32
TAB_H = 257
LCM_BYTES = math.lcm(*range(1, MAX_BYTES + 1))       # h / 8p compared as h * (LCM_BYTES / p): exact, below 2^56
UNIT_DTYPE = np.dtype([("table", "<u4"), ("type", "<u4"), ("max_hamming", "<i4"), ("nbytes", "<u4"), ("words", "<u8", (4,))])
_BLOCK = 1 << 24      # bytes compared per NumPy step


def words_to_bytes(words):
    """uint64 words [n, W] packed big-endian (the C-ABI layout) as code bytes uint8 [n, 32]."""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    out = np.zeros((words.shape[0], MAX_BYTES), dtype=np.uint8)
    out[:, : 8 * words.shape[1]] = words.astype(">u8").view(np.uint8).reshape(words.shape[0], -1)
    return out


def score_tables(exponent):
    """
    The two tables a caller hands to ``match_assets``, [prefix bytes 0..32][hamming 0..256] flattened: the unit score
    ``max(0, 1 - float64(float32(h) / float32(8 p)))`` and ``score ** exponent`` by Python's own ``**``.
    """
    score = np.zeros((MAX_BYTES + 1, TAB_H), dtype=np.float64)
    for p in range(1, MAX_BYTES + 1):
        for h in range(TAB_H):
            score[p, h] = max(0.0, 1.0 - float(np.float32(h) / np.float32(8 * p)))
    flat = score.ravel()
    return flat, np.array([s**exponent for s in flat.tolist()], dtype=np.float64)


class ModelTable:
    """The rows of one NPHD table with 64-bit keys, kept in ascending key order."""

    def __init__(self):
        self.keys = np.zeros(0, dtype=np.uint64)
        self.codes = np.zeros((0, MAX_BYTES), dtype=np.uint8)
        self.nbytes = np.zeros(0, dtype=np.int64)

    def add(self, keys, words, nbytes):
        keys = np.concatenate([self.keys, np.asarray(keys, dtype=np.uint64)])
        codes = np.concatenate([self.codes, words_to_bytes(words)])
        nb = np.concatenate([self.nbytes, np.asarray(nbytes, dtype=np.int64)])
        order = np.argsort(keys, kind="stable")
        self.keys, self.codes, self.nbytes = keys[order], codes[order], nb[order]
        assert len(np.unique(self.keys)) == len(self.keys)

    def _hamming(self, q_codes, q_nbytes):
        """(hamming [m, n], prefix bytes [n]) of m query codes of ONE length against every row, over the common prefix."""
        m, n = len(q_codes), len(self.keys)
        pb = np.minimum(self.nbytes, q_nbytes)
        ham = np.zeros((m, n), dtype=np.int64)
        for length in np.unique(self.nbytes).tolist():
            rows = np.nonzero(self.nbytes == length)[0]
            p = min(length, q_nbytes)
            step = max(1, _BLOCK // max(1, len(rows) * p))
            for at in range(0, m, step):
                diff = self.codes[rows][None, :, :p] ^ q_codes[at : at + step, None, :p]
                ham[at : at + step, rows] = np.bitwise_count(diff).sum(axis=2, dtype=np.int64)
        return ham, pb

    def lists(self, q_codes, q_nbytes, k, instance):
        """
        Per query code its neighbour list [(key, prefix bytes * 257 + hamming)], at most k long.  Similarity: every row, ascending
        exact (h / 8p, key).  INSTANCE: the rows with no differing bit over the common prefix, ascending key.
        """
        q_codes = np.asarray(q_codes, dtype=np.uint8).reshape(-1, MAX_BYTES)
        if len(self.keys) == 0:
            return [([], []) for _ in range(len(q_codes))]
        ham, pb = self._hamming(q_codes, q_nbytes)
        out = []
        if instance:
            for row in ham:
                hit = np.nonzero(row == 0)[0][:k]
                out.append((self.keys[hit].tolist(), (pb[hit] * TAB_H).tolist()))
            return out
        rank = ham * (LCM_BYTES // pb)[None, :]
        order = np.argsort(rank, axis=1, kind="stable")[:, :k]            # rows stand in key order: ties ascend by key
        for row, o in zip(ham, order):
            out.append((self.keys[o].tolist(), (pb[o] * TAB_H + row[o]).tolist()))
        return out


def float_sum(values, compensated):
    """CPython's ``sum()`` of floats: sequential additions up to 3.11, Neumaier's compensated form from 3.12 (``bltinmodule.c``)."""
    if bool(compensated) == (sys.version_info >= (3, 12)):
        return sum(values)
    if not compensated:
        s = 0.0
        for x in values:
            s = s + x
        return s
    s, c = 0.0, 0.0
    for x in values:
        t = s + x
        if abs(s) >= abs(x):
            c += (s - t) + x
        else:
            c += (x - t) + s
        s = t
    return s + c if c and math.isfinite(c) else s


def score_lists(unit_lists, unit_types, exclude, score_table, pow_table, threshold, compensated, limit):
    """
    One query: ``unit_lists`` [(keys, table indices)] in unit order, ``unit_types`` their type indices, ``exclude`` a key or None.
    Returns [(key, total, {type: score})], ranked and cut.
    """
    merged = {}           # key -> {type: [score, table index of that score]}, both dicts in first-appearance order
    for (keys, idxs), t in zip(unit_lists, unit_types):
        for key, i in zip(keys, idxs):
            types = merged.setdefault(key, {})
            s = score_table[i]
            held = types.get(t)
            if held is None:
                types[t] = [s, i]
            elif s > held[0]:
                held[0], held[1] = s, i
    scored = []
    for key, types in merged.items():
        confident, powers = [], []
        for s, i in types.values():
            if s >= threshold:
                confident.append(s)
                powers.append(pow_table[i])
        if not confident or key == exclude:
            continue
        weight = float_sum(confident, compensated)
        total = float_sum(powers, compensated) / weight if weight > 0.0 else 0.0
        scored.append((key, total, types))
    scored.sort(key=lambda r: r[1], reverse=True)
    return [(key, total, {t: s for t, (s, _) in types.items()}) for key, total, types in scored[:limit]]


def unit_lists(tables, units, instance_first_k, instance_max_k, limit):
    """Every unit's final neighbour list, one brute-force pass per (table, code length, kind): [(keys, table indices)]."""
    units = np.asarray(units, dtype=UNIT_DTYPE)
    codes = words_to_bytes(units["words"]) if len(units) else np.zeros((0, MAX_BYTES), dtype=np.uint8)
    out = [None] * len(units)
    groups = {}
    for u in range(len(units)):
        groups.setdefault((int(units["table"][u]), int(units["nbytes"][u]), int(units["max_hamming"][u]) >= 0), []).append(u)
    for (tid, nbytes, instance), members in groups.items():
        table = tables[tid]
        got = table.lists(codes[members], nbytes, instance_first_k if instance else limit, instance)
        if instance and instance_max_k > instance_first_k:
            full = [j for j, (keys, _) in enumerate(got) if len(keys) >= instance_first_k]
            if full:
                for j, again in zip(full, table.lists(codes[members][full], nbytes, instance_max_k, True)):
                    got[j] = again
        for u, lst in zip(members, got):
            out[u] = lst
    return out


def match_assets(tables, units, offsets, limit, instance_first_k, instance_max_k, exclude, has_exclude, score_table, pow_table,
                 threshold, compensated, n_types, lists=None):
    """
    ``HipEngine.match_assets`` over ``tables`` = {table id: ModelTable}: (keys u64 [nq, limit], scores f64 [nq, limit], counts u32
    [nq], types u8 [nq, limit, n_types] 255 past the last, type scores f64 [nq, limit, n_types], unit counts u32 [units]).
    ``lists``: the units' neighbour lists from elsewhere (``unit_lists``' shape) instead of the brute force.
    """
    units = np.asarray(units, dtype=UNIT_DTYPE)
    offsets = [int(o) for o in offsets]
    nq = len(offsets) - 1
    score_table = np.asarray(score_table, dtype=np.float64).tolist()
    pow_table = np.asarray(pow_table, dtype=np.float64).tolist()
    if lists is None:
        lists = unit_lists(tables, units, instance_first_k, instance_max_k, limit)
    keys = np.zeros((nq, limit), dtype=np.uint64)
    scores = np.zeros((nq, limit), dtype=np.float64)
    counts = np.zeros(nq, dtype=np.uint32)
    types = np.full((nq, limit, n_types), 255, dtype=np.uint8)
    type_scores = np.zeros((nq, limit, n_types), dtype=np.float64)
    unit_counts = np.array([len(k) for k, _ in lists], dtype=np.uint32)
    unit_type = units["type"].tolist()
    for q in range(nq):
        a, b = offsets[q], offsets[q + 1]
        ranked = score_lists(lists[a:b], unit_type[a:b], int(exclude[q]) if has_exclude[q] else None, score_table, pow_table,
                             float(threshold), compensated, limit)
        c = counts[q] = len(ranked)
        if c:
            keys[q, :c] = np.array([key for key, _, _ in ranked], dtype=np.uint64)
            scores[q, :c] = [min(1.0, total) for _, total, _ in ranked]
            types[q, :c] = [list(per_type) + [255] * (n_types - len(per_type)) for _, _, per_type in ranked]
            type_scores[q, :c] = [list(per_type.values()) + [0.0] * (n_types - len(per_type)) for _, _, per_type in ranked]
    return keys, scores, counts, types, type_scores, unit_counts
