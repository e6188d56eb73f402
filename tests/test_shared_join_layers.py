"""
The one shared-content join path between ``pairs.shared_sides`` and ``HipTable``: ``HipSimprintIndex.joins_shared`` / ``shared`` over
``HipIndex128.joins_shared`` / ``join_shared`` (CPU tier).

Two simprint tables on the stand-in engine of ``test_shared_match_segments``, whose four ``HipTable.join_*`` methods are answered by the
host models.  What is checked is that each ``(other, segments)`` form is the matching ``HipTable`` method with the arguments the middle
layer owes it and comes back in the one five-part shape, which forms a table is said to have, and what is refused before any join.
"""

import numpy as np
import pytest

from helpers import flip_bits
from iscc_search_amd.simprint import DOC_FREQ_DUP_LIMIT, HipSimprintIndex, pack_chunk_pointer
from oracle_engine import OracleEngine
from test_shared_content import OverlapOracleEngine, rnd
from test_shared_match_segments import LocatedOracleEngine
from test_shared_matches import SharedOracleEngine
from test_shared_segments import SegmentOracleEngine

FORMS = [(False, False), (False, True), (True, False), (True, True)]      # (cross join, segments)
THRESHOLD = 0.9


def body(key):
    return key.to_bytes(8, "big")


def method_of(cross, segments):
    return ("join_segments" if segments else "join_overlaps") + ("_between" if cross else "")


def table_of(engine, assets, ndim=64):
    """A ``HipSimprintIndex`` holding ``assets`` = {key: [simprint]}: chunk i of an asset lies at bytes 10 i .. 10 i + 10."""
    idx = HipSimprintIndex(engine, ndim=ndim)
    keys = [pack_chunk_pointer(body(k), 10 * i, 10) for k, codes in assets.items() for i in range(len(codes))]
    idx.add_raw(keys, [np.frombuffer(c, dtype=np.uint8) for codes in assets.values() for c in codes])
    return idx


def libraries():
    """Table a holds assets 1, 2, 5 and table b 5, 8, 9.  Chunks 1..3 of asset 1 are chunks 1..3 of asset 2 (within a), chunks 0..2 of
    asset 1 are chunks 2..4 of asset 8 (across, one of them two bits off), and asset 5 is the same two chunks in both tables."""
    rng = np.random.default_rng(31)
    c = [rnd(rng) for _ in range(5)]
    five = [rnd(rng), rnd(rng)]
    a = {1: c, 2: [rnd(rng), c[1], c[2], c[3]], 5: five}
    b = {5: five, 8: [rnd(rng), rnd(rng), c[0], flip_bits(c[1], 2), c[2], rnd(rng)], 9: [rnd(rng) for _ in range(3)]}
    return a, b


@pytest.fixture(scope="module")
def tables():
    engine = LocatedOracleEngine()
    a, b = libraries()
    return table_of(engine, a), table_of(engine, b), [body(k) for k in sorted(a)], [body(k) for k in sorted(b)]


def same(got, exp):
    """Array equality of two join results part by part; dicts and None by ``==``."""
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        if isinstance(e, np.ndarray):
            assert g.dtype == e.dtype and np.array_equal(g, e)
        else:
            assert g == e


@pytest.mark.parametrize("cross,segments", FORMS)
@pytest.mark.parametrize("max_doc_freq", [0, 2, DOC_FREQ_DUP_LIMIT + 7])
def test_every_form_equals_its_table_method(tables, monkeypatch, cross, segments, max_doc_freq):
    a, b, bodies_a, bodies_b = tables
    keys_a, keys_b = (np.array([int.from_bytes(x, "big") for x in bodies], dtype=np.uint64) for bodies in (bodies_a, bodies_b))
    radius, dup_limit = a._radius_for(THRESHOLD), max(DOC_FREQ_DUP_LIMIT, max_doc_freq)
    table, name = a._index._table, method_of(cross, segments)
    if cross:
        args = (b._index._table, radius, keys_a, keys_b, max_doc_freq, 1000, dup_limit, True)
        records, chunks_a, chunks_b, info, *runs = getattr(table, name)(*args)
    else:
        args = (radius, keys_a, max_doc_freq, 1000, dup_limit)
        records, chunks_a, info, *runs = getattr(table, name)(*args)
        chunks_b = chunks_a
    assert info["chunk_pairs"] >= 3 and len(runs) == segments

    calls = []
    method = getattr(table, name)
    monkeypatch.setattr(table, name, lambda *args: calls.append(args) or method(*args))
    got = a.shared(bodies_a, THRESHOLD, max_doc_freq, 1000, b if cross else None, bodies_b if cross else None, True, segments)
    same(got, (records, chunks_a, chunks_b, info, runs[0] if segments else None))
    assert cross or got[2] is got[1]
    # one call of that one method, with the radius, the keys of the bodies and the dup limit
    assert len(calls) == 1
    same(calls[0], args)
    assert calls[0][0] is args[0]
    if segments:
        # the planted run of three chunks: asset 1 is label 0 on side a; asset 2 is label 1 of a, asset 8 label 1 of b
        run = [(int(r["src"]), int(r["dst"]), int(r["first_src"]), int(r["first_dst"])) for r in got[4] if r["length"] == 3]
        assert run == ([(0, 1, 0, 2)] if cross else [(0, 1, 1, 1)])


@pytest.mark.parametrize("segments", [False, True])
def test_skip_same_asset_is_passed_through(tables, segments):
    a, b, bodies_a, bodies_b = tables
    five = (bodies_a.index(body(5)), bodies_b.index(body(5)))

    def pairs_of(**kwargs):
        records = a.shared(bodies_a, THRESHOLD, 0, 1000, b, bodies_b, segments=segments, **kwargs)[0]
        return {(int(r["src"]), int(r["dst"])) for r in records if r["reserved"] == 0}

    assert five not in pairs_of() and five not in pairs_of(skip_same_asset=True)
    assert pairs_of(skip_same_asset=False) == pairs_of() | {five}


@pytest.mark.parametrize("engine,has", [
    (OracleEngine, set()),
    (OverlapOracleEngine, {"join_overlaps"}),
    (SharedOracleEngine, {"join_overlaps", "join_overlaps_between"}),
    (SegmentOracleEngine, {"join_overlaps", "join_segments"}),
    (LocatedOracleEngine, {"join_overlaps", "join_segments", "join_overlaps_between", "join_segments_between"}),
])
def test_capability_is_the_tables_own_method(tables, engine, has):
    full = tables[0]
    a, b = libraries()
    engine = engine()
    one, two = table_of(engine, a), table_of(engine, b)
    for cross, segments in FORMS:
        assert one.joins_shared(two if cross else None, segments) is (method_of(cross, segments) in has)
        assert one._index.joins_shared(two._index if cross else None, segments) is (method_of(cross, segments) in has)
        if cross:
            # a cross form needs the method on both tables, whichever is asked
            assert full.joins_shared(one, segments) is one.joins_shared(full, segments) is (method_of(cross, segments) in has)


def test_refusals_name_the_argument(tables):
    a, b, bodies_a, bodies_b = tables
    bad = {
        "8-byte ISCC-ID bodies": [bodies_a[0][:7]],
        "ascending without repeats": bodies_a[::-1],
        "ascending without repeats: an asset's label is its position": [bodies_a[0], bodies_a[1], bodies_a[1]],
    }
    for segments in (False, True):
        for what, bodies in bad.items():
            with pytest.raises(ValueError, match=f"bodies_a must be {what}"):
                a.shared(bodies, THRESHOLD, 0, 1000, segments=segments)
            with pytest.raises(ValueError, match=f"bodies_a must be {what}"):
                a.shared(bodies, THRESHOLD, 0, 1000, b, bodies_b, segments=segments)
            with pytest.raises(ValueError, match=f"bodies_b must be {what}"):
                a.shared(bodies_a, THRESHOLD, 0, 1000, b, bodies, segments=segments)
        wide = HipSimprintIndex(a._index._table.engine, ndim=128)
        with pytest.raises(ValueError, match="one length: this table holds 64 bits, the other 128"):
            a.shared(bodies_a, THRESHOLD, 0, 1000, wide, bodies_b, segments=segments)
