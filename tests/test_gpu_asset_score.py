"""
On-device asset scoring (isccsearch_match_assets, csrc/assets_api.hip.h and csrc/asset_score.hip) against the plain host model of
``tests/asset_score_model.py``: ``HipEngine.match_assets`` called directly on small NPHD tables, all six outputs compared with
``==`` (scores bit for bit).  The shapes are the smallest that reach each branch: the record counts around the sort's sizes, blocks
that walk several queries on the scratch path, tie order, threshold and clamp edges, both summation rules, self-exclusion,
the key that equals the sort's padding, the second round over a query list, the overflow redo, and the refusals.
"""

import contextlib
import os

import numpy as np
import pytest

import asset_score_model as model
from helpers import flip_bits
from iscc_search_amd import _lib
from iscc_search_amd.engine import pack_bytes

pytestmark = pytest.mark.gpu

LDS_ITEMS = 2048                      # asset_score.h: items per sort array held in LDS
SIZE = (_lib.MAX_BYTES + 1) * 257
REAL = model.score_tables(2)          # the tables HipIndex hands over at its default exponent
OUTPUTS = ("keys", "scores", "counts", "types", "type_scores", "unit_counts")
DEFAULT_OPTS = not os.environ.get("ISCC_HIP_OPTS")
KEY_MAX = 2**64 - 1


class World:
    """The tables of one test, each twice: on the device and as the model's rows."""

    def __init__(self, engine):
        self.engine = engine
        self.rows = {}        # table id -> ModelTable
        self.hip = []

    def table(self, keys=None, codes=None):
        """A 64-bit-key NPHD table; ``codes`` a list of byte strings or a uint8 array [n, nbytes]."""
        t = self.engine.open_table(_lib.METRIC_NPHD, 1, 32)
        self.hip.append(t)
        self.rows[t.id] = model.ModelTable()
        if keys is not None:
            self.add(t, keys, codes)
        return t

    def add(self, t, keys, codes):
        keys = np.asarray(keys, dtype=np.uint64)
        words, nb = pack_bytes(codes, t.max_words)
        t.add(keys, words, nb)
        self.rows[t.id].add(keys, words, nb)

    def match(self, queries, limit, tabs=REAL, threshold=0.0, n_types=1, first_k=64, max_k=4096, exclude=None, compensated=(False, True)):
        """
        One call per summation rule, every output equal to the model's.  ``queries``: per query [(table, type, code bytes,
        instance)]; ``exclude``: per query a key or None.  Returns the outputs of the last call.
        """
        units, offsets = make_units(queries)
        nq = len(queries)
        ex = np.array([0 if e is None else e for e in (exclude or [None] * nq)], dtype=np.uint64)
        has_ex = np.array([e is not None for e in (exclude or [None] * nq)], dtype=np.uint8)
        for comp in compensated:
            args = (units, offsets, limit, first_k, max_k, ex, has_ex, tabs[0], tabs[1], threshold, comp, n_types)
            got = self.engine.match_assets(*args)
            want = model.match_assets(self.rows, *args)
            assert_equal(got, want)
        return got

    def drop(self):
        for t in self.hip:
            t.drop()


def assert_equal(got, want):
    for name, g, w in zip(OUTPUTS, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, name
        assert np.array_equal(g, w), f"{name} differ at {np.argwhere(g != w)[:5].tolist()}"


@contextlib.contextmanager
def world(engine):
    w = World(engine)
    try:
        yield w
    finally:
        w.drop()


def make_units(queries):
    n = sum(len(q) for q in queries)
    units = np.zeros(n, dtype=_lib.ASSET_UNIT_DTYPE)
    offsets = np.zeros(len(queries) + 1, dtype=np.uint32)
    u = 0
    for q, listed in enumerate(queries):
        for table, t, code, instance in listed:
            units[u]["table"], units[u]["type"], units[u]["max_hamming"], units[u]["nbytes"] = table.id, t, 0 if instance else -1, len(code)
            units[u]["words"] = np.frombuffer(bytes(code).ljust(32, b"\0"), dtype=">u8")
            u += 1
        offsets[q + 1] = u
    return units, offsets


def codes_of(rng, n, nbytes=8):
    return rng.integers(0, 256, size=(n, nbytes), dtype=np.uint8)


def keys_of(rng, n):
    """n distinct keys over the whole 64-bit range, in no order."""
    return rng.permutation(np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))


def flat_tables(by_hamming, nbytes=8):
    """Score and power tables that hold ``by_hamming`` = {h: (score, power)} at an ``nbytes`` prefix, zero elsewhere."""
    score, pw = np.zeros(SIZE), np.zeros(SIZE)
    for h, (s, p) in by_hamming.items():
        score[nbytes * 257 + h], pw[nbytes * 257 + h] = s, p
    return score, pw


# -- the two sorts' sizes -----------------------------------------------------------------------------------------------------

# (records, table rows, limit, units per query, sorted in global scratch): records = units x min(rows, limit)
SORT_CASES = [
    (0, 40, 5, 1, False),            # an INSTANCE unit nothing matches
    (1, 1, 1, 1, False), (1, 40, 1, 1, False),
    (2, 2, 5, 1, False),             # a list shorter than k
    (2, 40, 1, 2, False),
    (3, 3, 7, 1, False), (3, 3, 4096, 1, False),         # (the second: scratch sized by k, the three records still sorted in LDS)
    (2047, 2047, 2048, 1, False),
    (2048, 3000, 1024, 2, False),    # both LDS arrays full
    (2048, 2048, 2048, 1, False),
    (2049, 2049, 4096, 1, True),     # the first size past LDS
    (4096, 3000, 2048, 2, True),
]


@pytest.mark.parametrize("records,rows,limit,n_units,scratch", SORT_CASES)
def test_record_counts_around_the_sort_sizes(hip_engine, records, rows, limit, n_units, scratch):
    rng = np.random.default_rng(records * 7 + rows)
    with world(hip_engine) as w:
        t = w.table(keys_of(rng, rows), codes_of(rng, rows))
        if records == 0:
            query = [(t, 0, bytes(8), True)]
        else:
            query = [(t, u, rng.integers(0, 256, size=8, dtype=np.uint8).tobytes(), False) for u in range(n_units)]
            assert n_units * min(rows, limit) == records
        # the host sizes the scratch area by k; the kernel sorts a query there when its records, padded to a power of two, exceed LDS
        padded = 1 << max(0, records - 1).bit_length()
        assert (padded > LDS_ITEMS) == scratch and (not scratch or n_units * limit >= padded)
        keys, scores, counts, types, tsc, ucnt = w.match([query], limit, n_types=2)
        assert int(ucnt.sum()) == records and int(counts[0]) <= min(limit, records)


def test_blocks_walk_several_queries_on_the_scratch_path(hip_engine):
    """More listed queries than blocks, 2 200 records each: a block's second query reuses its scratch area and the LDS header."""
    cus = hip_engine.stats()["compute_units"]
    nq, limit = cus + 44, 1100
    rng = np.random.default_rng(31)
    with world(hip_engine) as w:
        big = w.table(keys_of(rng, 3000), codes_of(rng, 3000))
        small = w.table(keys_of(rng, 3), codes_of(rng, 3))
        empty = w.table()
        code = lambda: rng.integers(0, 256, size=8, dtype=np.uint8).tobytes()
        queries, kinds = [], []
        for q in range(nq):
            kind = q % 5 if q >= cus or q < 10 else 0            # every block's first query is large, most second ones are not
            kinds.append(kind)
            if kind in (0, 4):
                queries.append([(big, 0, code(), False), (big, 1, code(), False)])
            elif kind == 1:
                queries.append([(small, 0, code(), False)])
            elif kind == 2:
                queries.append([])
            else:
                queries.append([(empty, 1, code(), False), (small, 1, code(), False), (small, 0, code(), False)])
        assert 2 * limit > LDS_ITEMS and nq > cus
        keys, scores, counts, *_ = w.match(queries, limit, n_types=2, compensated=(False,))
        assert counts.tolist() == [{0: limit, 4: limit, 1: 3, 2: 0, 3: 3}[kind] for kind in kinds]
        assert {0, 1, 2, 3} <= set(kinds[cus:])


# -- order ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("groups", [1, 2, 255, 256, 257])
def test_tie_order_and_the_limit_cut(hip_engine, groups):
    """
    Three totals only (scores 0.25 and 0.5 by the distance's parity, power = score squared), two unit types over two tables whose
    key ranges overlap: ``groups`` assets in all, their first appearances spread over both slots and every rank.
    """
    rng = np.random.default_rng(groups)
    tabs = flat_tables({h: ((0.5, 0.25) if h % 2 else (0.25, 0.0625)) for h in range(65)})
    keys = keys_of(rng, groups)
    a, b = keys[: max(1, 2 * groups // 3)], keys[groups // 3:]
    with world(hip_engine) as w:
        ta, tb = w.table(a, codes_of(rng, len(a))), w.table(b, codes_of(rng, len(b)))
        query = [(ta, 0, bytes(8), False), (tb, 1, bytes([255] * 8), False)]
        full = w.match([query, query[::-1]], 300, tabs=tabs, n_types=2)
        assert full[2].tolist() == [groups, groups]                      # the kept-group count of both queries
        top = int((full[1][0] == full[1][0, 0]).sum())                   # the leading tie group
        if groups > 2:
            assert 1 < top < groups
            order = full[0][0, :top].tolist()
            assert order != sorted(order) and order != sorted(order, reverse=True)     # first appearance is not key order
        for limit in sorted({1, 2, top - 1, top, top + 1} - {0}):
            w.match([query, query[::-1]], limit, tabs=tabs, n_types=2)


def test_grouping_over_types_lengths_and_sixty_four_units(hip_engine):
    rng = np.random.default_rng(64)
    n = 240
    keys = keys_of(rng, n)
    base = rng.integers(0, 256, size=32, dtype=np.uint8)
    with world(hip_engine) as w:
        tables = []
        for t in range(3):
            # three segments per table: rows of 8, 16 and 32 bytes, near one base code, every table holding the same assets
            tbl = w.table()
            order = rng.permutation(n)
            for s, nbytes in enumerate((8, 16, 32)):
                part = order[s::3]
                codes = np.tile(base[:nbytes], (len(part), 1))
                flips = rng.integers(0, 8 * nbytes, size=(len(part), 6))
                for r, row in enumerate(flips[:, : 1 + t * 2]):
                    for bit in row:
                        codes[r, bit // 8] ^= 1 << (bit % 8)
                w.add(tbl, keys[part], codes)
            tables.append(tbl)
            assert sorted(tbl.segments()) == [8, 16, 32]
        b = base.tobytes()
        queries = [
            [(tables[0], 0, b[:8], False), (tables[0], 0, b[:16], False)],                       # one type at two lengths
            [(tables[2], 2, b[:32], False), (tables[0], 0, b[:8], False), (tables[1], 1, b[:16], False), (tables[0], 0, b[:32], False)],
            [(tables[1], 1, flip_bits(b[:8], 3), False), (tables[2], 2, b[:16], False), (tables[0], 0, flip_bits(b[:16], 5), False)],
        ]
        keys3, _, counts, types, *_ = w.match(queries, 25, n_types=3)
        seen = {tuple(x for x in row if x != 255) for q in range(3) for row in types[q, : int(counts[q])].tolist()}
        assert len({s for s in seen if len(s) >= 2}) >= 3                  # several first-appearance orders of the types
        # 64 units of 16 types in one query
        units64 = [(tables[u % 3], u % 16, flip_bits(b[: (8, 16, 32)[(u // 3) % 3]], u % 9), False) for u in range(64)]
        assert len(units64) == _lib.MAX_ASSET_UNITS
        _, _, counts, types, *_ = w.match([units64, queries[1]], 20, n_types=16)
        assert max((row != 255).sum() for row in types[0, : int(counts[0])]) > 3
        w.match([units64], 40, n_types=16, compensated=(True,))          # 2 560 records: the same on the scratch path


# -- scores ---------------------------------------------------------------------------------------------------------------------

def _placed(w, q, placement):
    """Two tables (types 0 and 1) holding asset ``key`` at the Hamming distances ``placement[key]`` = (h0 or None, h1 or None) from q."""
    out = []
    for t in range(2):
        rows = [(key, flip_bits(q, hs[t])) for key, hs in placement.items() if hs[t] is not None]
        out.append(w.table([k for k, _ in rows], [c for _, c in rows]))
    return out


def test_threshold_equality_partial_confidence_and_the_clamp(hip_engine):
    below = float(np.nextafter(0.5, 0.0))
    tabs = flat_tables({0: (1.0, 1.0), 1: (0.5, 0.25), 2: (below, 0.9), 3: (0.75, 1.2), 4: (0.25, 0.9)})
    q = bytes(range(8, 16))
    placement = {
        11: (0, 0),         # 2 / 2 = 1.0: a full score
        3: (3, None),       # 1.2 / 0.75 = 1.6: reported 1.0, ranked above every 1.0
        17: (1, None),      # its one score EQUALS the threshold: kept, 0.25 / 0.5
        5: (2, 4),          # every type below the threshold: dropped
        2: (2, 0),          # type 0 below: out of the total (1.0 / 1.0), still listed
        29: (3, 3),         # 2.4 / 1.5 = 1.6: ties with asset 3 above the clamp
        7: (3, 0),          # 2.2 / 1.75 = 1.2571...: between them and the 1.0s
        13: (4, 1),         # type 0 below: 0.25 / 0.5 ties with asset 17
    }
    with world(hip_engine) as w:
        t0, t1 = _placed(w, q, placement)
        query = [(t0, 0, q, False), (t1, 1, q, False)]
        for limit in (3, 4, 8):                                   # (the limit is the lists' length too: short ones lose assets)
            w.match([query, query[::-1]], limit, tabs=tabs, threshold=0.5, n_types=2)
        keys, scores, counts, types, tsc, _ = w.match([query], 10, tabs=tabs, threshold=0.5, n_types=2)
        # by hand: the 1.6s in first-appearance order (distance 3 lists asset 3 before 29), then 7, then the 1.0s with 11 (distance
        # 0) first, then the 0.5s
        assert keys[0, : int(counts[0])].tolist() == [3, 29, 7, 11, 2, 17, 13]
        assert scores[0, :7].tolist() == [1.0, 1.0, 1.0, 1.0, 1.0, 0.5, 0.5]
        assert types[0, 4].tolist() == [0, 1] and tsc[0, 4].tolist() == [below, 1.0]


def test_zero_weight_group(hip_engine):
    """Threshold 0.0 and every confident score 0.0: the weight is 0.0 and the total 0.0, as ``unit_match._confidence_total`` has it."""
    from iscc_search_amd import unit_match

    tabs = flat_tables({0: (0.0, 0.0), 1: (0.0, 0.3), 2: (0.5, 0.25)})
    q = bytes(range(40, 48))
    with world(hip_engine) as w:
        t0, t1 = _placed(w, q, {9: (0, 1), 4: (1, None), 6: (2, 0), 8: (None, 2)})
        keys, scores, counts, types, tsc, _ = w.match([[(t0, 0, q, False), (t1, 1, q, False)]], 10, tabs=tabs, n_types=2)
        assert keys[0, :4].tolist() == [6, 8, 9, 4] and scores[0, :4].tolist() == [0.5, 0.5, 0.0, 0.0] and int(counts[0]) == 4
        host = unit_match._rank_aggregated({9: {"a": 0.0, "b": 0.0}, 4: {"a": 0.0}}, 0.0, 2, None, 10)
        assert [(k, s) for k, s, _ in host] == [(9, 0.0), (4, 0.0)]


def test_both_summation_rules(hip_engine):
    """Five unit types whose scores make the compensation term change the last bit of both sums' quotient."""
    vals = {1: (1.0, 0.25), 2: (1e-16, 0.25), 3: (1e-16, 0.25), 4: (1e-16, 0.125), 5: (0.5, 0.1)}
    tabs = flat_tables(vals)
    q = bytes(range(1, 9))
    with world(hip_engine) as w:
        tables = [w.table([77, 1000 + t], [flip_bits(q, t + 1), bytes(255 - b for b in q)]) for t in range(5)]
        ws, ps = [vals[h][0] for h in range(1, 6)], [vals[h][1] for h in range(1, 6)]
        totals = {c: model.float_sum(ps, c) / model.float_sum(ws, c) for c in (False, True)}
        assert totals[False] != totals[True] and max(totals.values()) < 1.0
        for comp in (False, True):
            for n in (3, 5):                                         # the three-type last-bit case, then five confident types
                query = [(tables[t], t, q, False) for t in range(n)]
                keys, scores, *_ = w.match([query], 4, tabs=tabs, n_types=5, compensated=(comp,))
                assert int(keys[0, 0]) == 77
            assert scores[0, 0] == totals[comp]
        # real scores, eight types: sums of thirds and fifths round differently under the two rules somewhere in 64 assets
        rng = np.random.default_rng(12)
        keys = keys_of(rng, 64)
        many = [w.table(keys, np.bitwise_xor(np.frombuffer(q, dtype=np.uint8), codes_of(rng, 64) & codes_of(rng, 64) & codes_of(rng, 64))) for _ in range(8)]
        w.match([[(t, i, q, False) for i, t in enumerate(many)]], 64, tabs=model.score_tables(3), threshold=0.4, n_types=8)


# -- exclusion, keys ------------------------------------------------------------------------------------------------------------

def test_self_exclusion_edges(hip_engine):
    rng = np.random.default_rng(8)
    with world(hip_engine) as w:
        keys = np.concatenate([np.array([0, 5, KEY_MAX], dtype=np.uint64), keys_of(rng, 60)])
        codes = codes_of(rng, 63)
        q = codes[1].tobytes()                        # key 5 is the exact match, key 0 one bit away
        codes[0] = np.frombuffer(flip_bits(q, 1), dtype=np.uint8)
        t = w.table(keys, codes)
        query = [(t, 0, q, False)]
        exclude = [5, 123456789, None, 0, KEY_MAX, None]          # the best; absent; none (its zero is no key); key 0; the last key
        out_keys, _, counts, *_ = w.match([query] * 6, 63, exclude=exclude)
        assert counts.tolist() == [62, 63, 63, 62, 62, 63]
        assert out_keys[0, 0] == 0 and out_keys[1, 0] == 5 and out_keys[2, :2].tolist() == [5, 0] and out_keys[3, :2].tolist() != [5, 0]
        w.match([query] * 6, 2, exclude=exclude)


@pytest.mark.parametrize("records", [3, 5, 2049])
def test_the_key_that_equals_the_sort_padding(hip_engine, records):
    rng = np.random.default_rng(records)
    with world(hip_engine) as w:
        keys = keys_of(rng, records)
        keys[records // 2] = KEY_MAX
        codes = codes_of(rng, records)
        t = w.table(keys, codes)
        near, far = codes[records // 2].tobytes(), bytes(255 - b for b in codes[records // 2].tobytes())
        limit = 4096 if records > LDS_ITEMS else records
        out_keys, _, counts, *_ = w.match([[(t, 0, near, False)], [(t, 0, far, False)]], limit)
        assert counts.tolist() == [records, records]
        assert out_keys[0, 0] == KEY_MAX and KEY_MAX in out_keys[1].tolist()
        if records < LDS_ITEMS:                                       # two lists: the key twice among 2 x records items
            w.match([[(t, 0, near, False), (t, 1, far, False)]], limit, n_types=2)


# -- shapes of the call ---------------------------------------------------------------------------------------------------------

def test_call_shapes(hip_engine):
    rng = np.random.default_rng(77)
    with world(hip_engine) as w:
        one = w.table(keys_of(rng, 500), codes_of(rng, 500))                 # one segment: queued behind one synchronisation
        three = w.table()                                                     # three segments: searched list by list
        tk = keys_of(rng, 300)
        for s, nbytes in enumerate((8, 16, 32)):
            w.add(three, tk[s::3], codes_of(rng, len(tk[s::3]), nbytes))
        empty = w.table()
        code = lambda n=8: rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        assert w.match([[(one, 0, code(), False)]], 3)[2].tolist() == [3]     # nq = 1
        queries = []
        for q in range(_lib.ASSET_QUERIES_MAX):
            units = []
            if q not in (0, 500, 1023):                                       # no units: first, in the middle, last
                units.append((one, 0, code(), False))
                if q % 4 == 1:
                    units.append((one, 0, code(), False))
                if q % 7 == 2:
                    units.append((three, 1, code(16), False))
                if q % 11 == 3:
                    units.insert(0, (empty, 2, code(), False))
                if q % 13 == 4:
                    units.append((one, 2, code(), True))
            queries.append(units)
        assert sum(1 for units in queries for u in units if u[0] is one and not u[3]) > 1024       # two chunks of one search
        _, _, counts, _, _, ucnt = w.match(queries, 3, n_types=3, compensated=(True,))
        assert counts[[0, 500, 1023]].tolist() == [0, 0, 0] and counts[1] > 0
        # a unit over an empty table alone, and every query empty
        assert w.match([[(empty, 0, code(), False)], [(empty, 0, code(), True)]], 5)[2].tolist() == [0, 0]
        assert w.match([[], [], []], 5)[2].tolist() == [0, 0, 0]


def test_rows_past_a_querys_count_are_padded_not_left_over(hip_engine):
    """Two calls of one shape, the second with fewer results: nothing of the first may show past the second's counts."""
    rng = np.random.default_rng(3)
    with world(hip_engine) as w:
        t = w.table(keys_of(rng, 40), codes_of(rng, 40))
        code = rng.integers(0, 256, size=8, dtype=np.uint8).tobytes()
        assert w.match([[(t, 0, code, False)], [(t, 1, code, False)]], 30, n_types=2)[2].tolist() == [30, 30]
        keys, scores, counts, types, tsc, _ = w.match([[(t, 0, bytes(8), True)], [(t, 1, code, False)] * 2], 30, n_types=2, first_k=3, max_k=3)
        assert counts.tolist() == [0, 30] and not keys[0].any() and not scores[0].any() and (types[0] == 255).all() and not tsc[0].any()


# -- the second round -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first_k,max_k", [(64, 4096), (64, 64), (1, 4096), (1, 1), (70, 4096), (71, 72)])
def test_second_round_over_a_query_list(hip_engine, first_k, max_k):
    rng = np.random.default_rng(70)
    prefix = rng.integers(0, 256, size=8, dtype=np.uint8)
    with world(hip_engine) as w:
        shared = np.concatenate([np.tile(prefix, (70, 1)), codes_of(rng, 70)], axis=1)         # 70 rows of 16 bytes under one prefix
        others = codes_of(rng, 30, 16)
        inst = w.table(keys_of(rng, 100), np.concatenate([shared, others]))
        sim = w.table(keys_of(rng, 100), codes_of(rng, 100))
        p, lone, miss = prefix.tobytes(), others[3].tobytes(), bytes(8)
        queries = [
            [(sim, 0, p, False)],
            [(inst, 1, p, True), (sim, 0, miss, False)],          # 70 hits
            [(inst, 1, lone, True)],                              # one hit
            [(sim, 0, lone[:8], False), (inst, 1, lone[:8], True)],
            [(inst, 1, p, True)],                                 # 70 hits
            [(inst, 1, miss, True), (sim, 0, p, False)],          # none
        ]
        for limit in (100, 10):
            *_, ucnt = w.match(queries, limit, n_types=2, first_k=first_k, max_k=max_k)
            full = 70 if (max_k > first_k or first_k >= 70) else first_k           # re-asked up to max_k, or cut at k
            assert ucnt.tolist() == [min(limit, 100), min(full, max_k), min(limit, 100), 1, min(limit, 100), 1, min(full, max_k), 0, min(limit, 100)]


def test_overflow_redo_of_a_deferred_chunk(hip_engine):
    """20 000 equal codes overflow the candidate lists of a queued search: that chunk is searched again, its queries scored again."""
    rng = np.random.default_rng(20)
    n = 20_000
    with world(hip_engine) as w:
        same = np.tile(np.frombuffer(bytes.fromhex("deadbeefcafef00d"), dtype=np.uint8), (n, 1))
        same[::1000, 7] ^= 1                                          # a few rows one bit away
        flagged = w.table(keys_of(rng, n), same)
        plain = w.table(keys_of(rng, n), codes_of(rng, n))
        small = w.table(keys_of(rng, 200), codes_of(rng, 200))
        q_same, q_near = bytes.fromhex("deadbeefcafef00d"), bytes.fromhex("deadbeefcafef00c")
        code = lambda: rng.integers(0, 256, size=8, dtype=np.uint8).tobytes()
        queries = [
            [(plain, 1, code(), False)],
            [(flagged, 0, q_same, False)],
            [(plain, 1, code(), False), (small, 2, code(), False)],
            [(plain, 1, code(), False), (flagged, 0, q_near, False)],
            [(small, 2, code(), False)],
            [(flagged, 0, code(), False), (small, 2, code(), False)],
        ]
        before = hip_engine.stats()["fallback_queries"]
        w.match(queries, 10, n_types=3, compensated=(False,))
        if DEFAULT_OPTS:
            assert hip_engine.stats()["fallback_queries"] > before
        w.match(queries[::-1], 700, n_types=3, compensated=(True,))


# -- refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_engine_answering(hip_engine):
    rng = np.random.default_rng(5)
    with world(hip_engine) as w:
        t = w.table(keys_of(rng, 50), codes_of(rng, 50))
        short = hip_engine.open_table(_lib.METRIC_NPHD, 1, 8)
        hamming = hip_engine.open_table(_lib.METRIC_HAMMING, 1, 8)
        wide = hip_engine.open_table(_lib.METRIC_NPHD, 2, 32)
        dropped = hip_engine.open_table(_lib.METRIC_NPHD, 1, 32)
        w.hip += [short, hamming, wide]
        dropped.drop()
        q = bytes(range(8))
        good = [[(t, 0, q, False), (t, 1, q, True)]]

        def call(queries=good, limit=5, first_k=64, max_k=4096, n_types=2, offsets=None, patch=None):
            units, offs = make_units(queries)
            if patch:
                units[patch[0]][0] = patch[1]
            offs = offs if offsets is None else np.array(offsets, dtype=np.uint32)
            nq = len(offs) - 1
            return hip_engine.match_assets(units, offs, limit, first_k, max_k, np.zeros(nq, np.uint64), np.zeros(nq, np.uint8), REAL[0], REAL[1], 0.0, False, n_types)

        refused = {
            "nq > 1024": dict(queries=[[]] * 1025),
            "limit 0": dict(limit=0),
            "limit 4097": dict(limit=4097),
            "instance_first_k 0": dict(first_k=0),
            "instance_first_k above instance_max_k": dict(first_k=65, max_k=64),
            "instance_max_k 4097": dict(max_k=4097),
            "n_types 0": dict(n_types=0),
            "n_types 17": dict(n_types=17),
            "65 units in one query": dict(queries=[[(t, 0, q, False)] * 65]),
            "offsets[0] != 0": dict(offsets=[1, 2]),
            "decreasing offsets": dict(queries=good * 2, offsets=[0, 2, 1]),
            "type >= n_types": dict(queries=[[(t, 2, q, False)]]),
            "max_hamming > 0": dict(patch=("max_hamming", 1)),
            "nbytes 0": dict(patch=("nbytes", 0)),
            "nbytes above 32": dict(patch=("nbytes", 33)),
            "nbytes above the table's": dict(queries=[[(short, 0, bytes(9), False)]]),
            "a Hamming table": dict(queries=[[(hamming, 0, q, False)]]),
            "a 128-bit-key table": dict(queries=[[(wide, 0, q, False)]]),
        }
        for what, kwargs in refused.items():
            with pytest.raises(ValueError):
                call(**kwargs)
                pytest.fail(f"{what} was accepted")
            w.match(good, 5, n_types=2, compensated=(False,))
        with pytest.raises(LookupError):                         # -ENOENT, as every entry point answers for a table that is not open
            call(queries=[[(dropped, 0, q, False)]])
        w.match(good, 5, n_types=2)
