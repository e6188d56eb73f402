"""
``find_shared_matches(segments=True)``: WHERE an asset of one index and an asset of another share chunks (CPU tier).

The engine is the oracle-backed stand-in of ``test_shared_matches`` with a model-backed ``join_segments_between``
(``tests/segments_between_model.py``).  What is checked is the host side -- ``pairs.shared_matches`` and ``pairs._located`` under
``HipIndex.find_shared_matches`` -- against segments worked by hand, against itself with the sides swapped, against
``find_shared_content(segments=True)`` on an index that holds both libraries, and that ``segments=False`` is the call it was.
"""

import dataclasses

import numpy as np
import pytest

from helpers import flip_bits, make_asset, make_iscc_id
from iscc_search_amd import codec
from iscc_search_amd.index import HipIndex, HipIndexManager, HipOptions
from iscc_search_amd.pairs import SharedMatch, SharedSegment
from iscc_search_amd.schema import IsccIndex
from overlap_between_model import SKIP_SAME_ASSET
from segments_between_model import model_segments_between
from test_shared_content import CT, chunks_of, library, rnd
from test_shared_matches import SharedOracleEngine, SharedOracleTable, swapped, two_indexes
from test_shared_segments import SegmentOracleTable


class LocatedOracleTable(SharedOracleTable, SegmentOracleTable):
    def join_segments_between(self, other, max_hamming, asset_keys_a, asset_keys_b, max_doc_freq, max_pairs, dup_limit=1000, skip_same_asset=True):
        """``HipTable.join_segments_between`` answered by the host model."""
        if getattr(other, "engine", None) is not self.engine:
            raise ValueError("join_segments_between needs two tables of one engine: the other table belongs to another engine")
        ka, wa, _ = self._arrays()
        kb, wb, _ = other._arrays()
        rc, records, chunks_a, chunks_b, info, segments = model_segments_between(
            ka.reshape(-1, 2), wa, kb.reshape(-1, 2), wb, asset_keys_a, asset_keys_b, max_hamming, max_doc_freq, dup_limit,
            SKIP_SAME_ASSET if skip_same_asset else 0)
        assert rc == 0
        if info["chunk_pairs"] > max_pairs:
            raise ValueError(f"{info['chunk_pairs']} chunk pairs exceed max_pairs={max_pairs}")
        return records, chunks_a, chunks_b, info, segments


class LocatedOracleEngine(SharedOracleEngine):
    def open_table(self, metric, key_words, max_bytes):
        t = LocatedOracleTable(metric, key_words, max_bytes)
        t.engine = self
        return t


class RefusingTable(SharedOracleTable):
    def join_segments_between(self, *args, **kwargs):
        raise AssertionError("segments=False reached join_segments_between")


class RefusingEngine(SharedOracleEngine):
    def open_table(self, metric, key_words, max_bytes):
        t = RefusingTable(metric, key_words, max_bytes)
        t.engine = self
        return t


def without_segments(result):
    return [dataclasses.replace(p, types={t: dataclasses.replace(c, segments=None) for t, c in p.types.items()}) for p in result]


def mirrored(result):
    """The located result with its sides exchanged, in the order find_shared_matches gives: ``swapped`` and every segment turned round."""
    turned = {}
    for r in result:
        turned[(r.iscc_id_b, r.iscc_id_a)] = {
            t: sorted((SharedSegment(s.offset_b, s.end_b, s.offset_a, s.end_a, s.first_chunk_b, s.first_chunk_a, s.chunks, s.span, s.similarity) for s in v.segments),
                      key=lambda s: (s.offset_a, s.offset_b, s.first_chunk_a, s.first_chunk_b))
            for t, v in r.types.items()}
    return [dataclasses.replace(p, types={t: dataclasses.replace(c, segments=turned[(p.iscc_id_a, p.iscc_id_b)][t]) for t, c in p.types.items()})
            for p in swapped(result)]


def clip_assets():
    """Asset 0: twelve chunks of ten bytes.  Asset 1 holds its chunks 3..8 from its own chunk 2 on, the fourth of them replaced (and
    the second four bits off).  Asset 2 holds chunks 0..5 at the same place, the third and fourth replaced.  Asset 3 shares nothing.
    Asset 7 has five chunks of its own.  The catalogue is (0, 7), the registry (1, 2, 3, 7)."""
    rng = np.random.default_rng(8)
    c = [rnd(rng) for _ in range(12)]
    one = [rnd(rng), rnd(rng), c[3], flip_bits(c[4], 4), c[5], rnd(rng), c[7], c[8], rnd(rng)]
    two = [c[0], c[1], rnd(rng), rnd(rng), c[4], c[5], rnd(rng)]
    seven = {CT: chunks_of([rnd(rng) for _ in range(5)])}
    sims = {0: {CT: chunks_of(c)}, 1: {CT: chunks_of(one)}, 2: {CT: chunks_of(two, size=7)}, 3: {CT: chunks_of([rnd(rng), rnd(rng)])}, 7: seven}
    assets = {i: make_asset(rng, i, simprints=s) for i, s in sims.items()}
    return [assets[0], assets[7]], [assets[1], assets[2], assets[3], assets[7]]


@pytest.fixture
def clips():
    return two_indexes(LocatedOracleEngine(), *clip_assets())


def segments_of(result, a, b, sp_type=CT):
    ids = (make_iscc_id(a), make_iscc_id(b))
    (pair,) = [p for p in result if (p.iscc_id_a, p.iscc_id_b) == ids]
    return pair.types[sp_type].segments


def test_segments_worked_by_hand(clips):
    a, b = clips
    got = a.find_shared_matches(b, segments=True)
    assert {(p.iscc_id_a, p.iscc_id_b) for p in got} == {(make_iscc_id(0), make_iscc_id(1)), (make_iscc_id(0), make_iscc_id(2))}
    # asset 0's chunks 3..5 are asset 1's chunks 2..4 (bytes 30..60 against 20..50), one of the three pairs four bits off; then 7..8
    assert segments_of(got, 0, 1) == [SharedSegment(30, 60, 20, 50, 3, 2, 3, 3, 1.0 - 4 / (3 * 64)), SharedSegment(70, 90, 60, 80, 7, 6, 2, 2, 1.0)]
    # asset 2's chunks are seven bytes long
    assert segments_of(got, 0, 2) == [SharedSegment(0, 20, 0, 14, 0, 0, 2, 2, 1.0), SharedSegment(40, 60, 28, 42, 4, 4, 2, 2, 1.0)]
    for p in got:
        assert isinstance(p, SharedMatch)
        for t in p.types.values():
            assert sum(s.chunks for s in t.segments) == t.chunk_pairs


def test_a_is_the_calling_indexs_asset(clips):
    a, b = clips
    got = b.find_shared_matches(a, segments=True)
    # asset 1 of the registry is a now, though its key is the larger: bytes 20..50 of it are bytes 30..60 of asset 0
    assert segments_of(got, 1, 0) == [SharedSegment(20, 50, 30, 60, 2, 3, 3, 3, 1.0 - 4 / (3 * 64)), SharedSegment(60, 80, 70, 90, 6, 7, 2, 2, 1.0)]
    assert segments_of(got, 2, 0) == [SharedSegment(0, 14, 0, 20, 0, 0, 2, 2, 1.0), SharedSegment(28, 42, 40, 60, 4, 4, 2, 2, 1.0)]
    for kwargs in ({}, {"max_gap": 1}, {"max_gap": 2, "min_segment": 4}, {"include_same_id": True}, {"threshold": 0.95}):
        forth = a.find_shared_matches(b, segments=True, **kwargs)
        assert forth and b.find_shared_matches(a, segments=True, **kwargs) == mirrored(forth), kwargs


def test_max_gap_bridges_and_min_segment_filters_after_merging(clips):
    a, b = clips
    one_missing = SharedSegment(30, 90, 20, 80, 3, 2, 5, 6, 1.0 - 4 / (5 * 64))
    two_missing = SharedSegment(0, 60, 0, 42, 0, 0, 4, 6, 1.0)
    gap0, gap1, gap2 = (a.find_shared_matches(b, segments=True, max_gap=g) for g in (0, 1, 2))
    assert len(segments_of(gap0, 0, 1)) == 2 and len(segments_of(gap0, 0, 2)) == 2
    assert segments_of(gap1, 0, 1) == [one_missing] and len(segments_of(gap1, 0, 2)) == 2
    assert segments_of(gap2, 0, 1) == [one_missing] and segments_of(gap2, 0, 2) == [two_missing]
    # nothing but the segments depends on it
    assert without_segments(gap0) == without_segments(gap1) == without_segments(gap2)
    got = a.find_shared_matches(b, segments=True, min_segment=3)
    assert [s.chunks for s in segments_of(got, 0, 1)] == [3] and segments_of(got, 0, 2) == []
    assert len(got) == 2                                           # the pairs stay listed
    got = a.find_shared_matches(b, segments=True, min_segment=4, max_gap=2)
    assert [s.chunks for s in segments_of(got, 0, 1)] == [5] and [s.chunks for s in segments_of(got, 0, 2)] == [4]
    got = a.find_shared_matches(b, segments=True, min_segment=5, max_gap=2)
    assert [s.chunks for s in segments_of(got, 0, 1)] == [5] and segments_of(got, 0, 2) == []


def test_include_same_id_is_one_run_of_all_chunks(clips):
    a, b = clips
    assert all(p.iscc_id_a != make_iscc_id(7) for p in a.find_shared_matches(b, segments=True))
    got = a.find_shared_matches(b, segments=True, include_same_id=True)
    assert segments_of(got, 7, 7) == [SharedSegment(0, 50, 0, 50, 0, 0, 5, 5, 1.0)]
    assert segments_of(got, 0, 1) == segments_of(a.find_shared_matches(b, segments=True), 0, 1)


def test_segments_false_is_the_call_it_was():
    cat, reg = clip_assets()
    a, b = two_indexes(SharedOracleEngine(), cat, reg)
    plain = a.find_shared_matches(b)
    assert plain and all(t.segments is None for p in plain for t in p.types.values())
    # a table whose join_segments_between raises: segments=False never touches it
    a, b = two_indexes(RefusingEngine(), cat, reg)
    assert a.find_shared_matches(b) == plain
    assert a.find_shared_matches(b, segments=False, min_segment=9, max_gap=9) == plain
    with pytest.raises(AssertionError, match="reached join_segments_between"):
        a.find_shared_matches(b, segments=True)
    a, b = two_indexes(LocatedOracleEngine(), cat, reg)
    assert a.find_shared_matches(b) == plain and a.find_shared_matches(b, segments=False) == plain
    located = a.find_shared_matches(b, segments=True)
    assert located != plain and without_segments(located) == plain


def test_disjoint_libraries_equal_the_cross_pairs_of_find_shared_content():
    rng = np.random.default_rng(23)
    assets = library(rng, 60, boiler=0.2)
    perm = rng.permutation(60)
    in_a = set(perm[:28].tolist())
    engine = LocatedOracleEngine()
    a, b = two_indexes(engine, [x for i, x in enumerate(assets) if i in in_a], [x for i, x in enumerate(assets) if i not in in_a])
    both = HipIndex(engine, HipOptions())
    both.add_assets(assets)
    ids_a = {x.iscc_id for i, x in enumerate(assets) if i in in_a}
    longest = turned = 0
    for kwargs in ({}, {"max_gap": 1}, {"min_segment": 2}, {"threshold": 0.9, "min_chunks": 2}):
        exp = []
        for p in both.find_shared_content(max_doc_freq=0, segments=True, **kwargs):
            if (p.iscc_id_a in ids_a) == (p.iscc_id_b in ids_a):
                continue                                       # both assets of one library
            if p.iscc_id_a in ids_a:
                exp.append(SharedMatch(p.iscc_id_a, p.iscc_id_b, p.score, p.types))
            else:
                exp.extend(mirrored([SharedMatch(p.iscc_id_a, p.iscc_id_b, p.score, p.types)]))
                turned += 1
        exp.sort(key=lambda r: (-r.score, codec.iscc_id_to_int(r.iscc_id_a), codec.iscc_id_to_int(r.iscc_id_b)))
        got = a.find_shared_matches(b, max_doc_freq=0, segments=True, **kwargs)
        assert len(got) > 5 and got == exp, kwargs
        longest = max([longest] + [s.chunks for p in got for t in p.types.values() for s in t.segments])
    assert longest >= 3 and turned > 5


def test_max_pairs_is_surfaced(clips):
    a, b = clips
    with pytest.raises(ValueError, match="exceed max_pairs"):
        a.find_shared_matches(b, segments=True, max_pairs=1)
    with pytest.raises(ValueError, match="9 chunk pairs exceed max_pairs=8"):
        a.find_shared_matches(b, segments=True, max_pairs=8)
    assert len(a.find_shared_matches(b, segments=True, max_pairs=9)) == 2


def test_tables_without_the_join_name_the_caller():
    cat, reg = clip_assets()
    a, b = two_indexes(SharedOracleEngine(), cat, reg)             # join_overlaps_between, but no join_segments_between
    assert a.find_shared_matches(b)
    with pytest.raises(NotImplementedError, match="find_shared_matches needs a single-GPU engine"):
        a.find_shared_matches(b, segments=True)


def test_manager_route_and_sharded_refusal():
    cat, reg = clip_assets()
    m = HipIndexManager("hip:///", engine=LocatedOracleEngine())
    m.create_index(IsccIndex(name="cat"))
    m.create_index(IsccIndex(name="reg"))
    m.add_assets("cat", cat)
    m.add_assets("reg", reg)
    got = m.find_shared_matches("cat", "reg", segments=True, min_segment=4, max_gap=2)
    assert got == m._indexes["cat"].find_shared_matches(m._indexes["reg"], segments=True, min_segment=4, max_gap=2)
    assert [s.chunks for s in segments_of(got, 0, 2)] == [4]
    assert all(t.segments is None for p in m.find_shared_matches("cat", "reg") for t in p.types.values())
    m.close()
    sharded = HipIndexManager("hip:///?devices=2", engine=LocatedOracleEngine())
    with pytest.raises(NotImplementedError, match="sharded"):
        sharded.find_shared_matches("cat", "reg", segments=True)
