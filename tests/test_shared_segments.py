"""
``find_shared_content(segments=True)``: WHERE two assets share chunks (CPU tier).

The engine is the oracle-backed stand-in of ``test_shared_content`` with a model-backed ``join_segments`` (``tests/segments_model.py``).
What is checked is the host side -- ``pairs.shared_content`` and ``pairs._located`` under ``HipIndex.find_shared_content`` -- against
segments worked by hand: the byte ranges, ``max_gap``, ``min_segment``, and that ``segments=False`` is the call it was.
"""

import dataclasses

import numpy as np
import pytest

from helpers import flip_bits, make_asset, make_iscc_id
from iscc_search_amd.index import HipIndex, HipIndexManager, HipOptions
from iscc_search_amd.pairs import SharedSegment
from iscc_search_amd.schema import IsccIndex
from segments_model import model_segments
from test_shared_content import CT, ST, OverlapOracleEngine, OverlapOracleTable, chunks_of, library, rnd


class SegmentOracleTable(OverlapOracleTable):
    def join_segments(self, max_hamming, asset_keys, max_doc_freq, max_pairs, dup_limit=1000):
        """``HipTable.join_segments`` answered by the host model."""
        keys, words, _ = self._arrays()
        rc, records, chunks, info, segments = model_segments(keys.reshape(-1, 2), words, asset_keys, max_hamming, max_doc_freq, dup_limit)
        assert rc == 0
        if info["chunk_pairs"] > max_pairs:
            raise ValueError(f"{info['chunk_pairs']} chunk pairs exceed max_pairs={max_pairs}")
        return records, chunks, info, segments


class SegmentOracleEngine(OverlapOracleEngine):
    def open_table(self, metric, key_words, max_bytes):
        t = SegmentOracleTable(metric, key_words, max_bytes)
        t.engine = self
        return t


class RefusingTable(OverlapOracleTable):
    def join_segments(self, *args, **kwargs):
        raise AssertionError("segments=False reached join_segments")


class RefusingEngine(OverlapOracleEngine):
    def open_table(self, metric, key_words, max_bytes):
        t = RefusingTable(metric, key_words, max_bytes)
        t.engine = self
        return t


def cpu_index(assets, engine=None):
    idx = HipIndex(engine or SegmentOracleEngine(), HipOptions())
    idx.add_assets(assets)
    return idx


def without_segments(result):
    return [dataclasses.replace(p, types={t: dataclasses.replace(c, segments=None) for t, c in p.types.items()}) for p in result]


@pytest.fixture
def clips():
    """Asset 0: twelve chunks of ten bytes.  Asset 1 holds its chunks 3..8 from its own chunk 2 on, the fourth of them replaced (and
    the second four bits off).  Asset 2 holds chunks 0..5 at the same place, the third and fourth replaced.  Asset 3 shares nothing."""
    rng = np.random.default_rng(8)
    c = [rnd(rng) for _ in range(12)]
    one = [rnd(rng), rnd(rng), c[3], flip_bits(c[4], 4), c[5], rnd(rng), c[7], c[8], rnd(rng)]
    two = [c[0], c[1], rnd(rng), rnd(rng), c[4], c[5], rnd(rng)]
    sims = [{CT: chunks_of(c)}, {CT: chunks_of(one)}, {CT: chunks_of(two, size=7)}, {CT: chunks_of([rnd(rng), rnd(rng)])}]
    return [make_asset(rng, i, simprints=s) for i, s in enumerate(sims)]


def segments_of(result, a, b, sp_type=CT):
    ids = (make_iscc_id(a), make_iscc_id(b))
    (pair,) = [p for p in result if (p.iscc_id_a, p.iscc_id_b) == ids]
    return pair.types[sp_type].segments


def test_segments_worked_by_hand(clips):
    idx = cpu_index(clips)
    got = idx.find_shared_content(segments=True)
    assert {(p.iscc_id_a, p.iscc_id_b) for p in got} == {(make_iscc_id(0), make_iscc_id(1)), (make_iscc_id(0), make_iscc_id(2)), (make_iscc_id(1), make_iscc_id(2))}
    # asset 0's chunks 3..5 are asset 1's chunks 2..4 (bytes 30..60 against 20..50), one of the three pairs four bits off; then 7..8
    assert segments_of(got, 0, 1) == [SharedSegment(30, 60, 20, 50, 3, 2, 3, 3, 1.0 - 4 / (3 * 64)), SharedSegment(70, 90, 60, 80, 7, 6, 2, 2, 1.0)]
    # asset 2's chunks are seven bytes long
    assert segments_of(got, 0, 2) == [SharedSegment(0, 20, 0, 14, 0, 0, 2, 2, 1.0), SharedSegment(40, 60, 28, 42, 4, 4, 2, 2, 1.0)]
    # assets 1 and 2 share chunks 4 (four bits off) and 5 of asset 0: chunks 3..4 of asset 1, 4..5 of asset 2
    assert segments_of(got, 1, 2) == [SharedSegment(30, 50, 28, 42, 3, 4, 2, 2, 1.0 - 4 / (2 * 64))]
    for p in got:
        for t in p.types.values():
            assert sum(s.chunks for s in t.segments) == t.chunk_pairs


def test_max_gap_bridges_missing_chunks(clips):
    idx = cpu_index(clips)
    one_missing = SharedSegment(30, 90, 20, 80, 3, 2, 5, 6, 1.0 - 4 / (5 * 64))
    two_missing = SharedSegment(0, 60, 0, 42, 0, 0, 4, 6, 1.0)
    gap0, gap1, gap2 = (idx.find_shared_content(segments=True, max_gap=g) for g in (0, 1, 2))
    assert len(segments_of(gap0, 0, 1)) == 2 and len(segments_of(gap0, 0, 2)) == 2
    assert segments_of(gap1, 0, 1) == [one_missing] and len(segments_of(gap1, 0, 2)) == 2
    assert segments_of(gap2, 0, 1) == [one_missing] and segments_of(gap2, 0, 2) == [two_missing]
    # nothing but the segments depends on it
    assert without_segments(gap0) == without_segments(gap1) == without_segments(gap2)


def test_min_segment_filters_after_merging(clips):
    idx = cpu_index(clips)
    got = idx.find_shared_content(segments=True, min_segment=3)
    assert [s.chunks for s in segments_of(got, 0, 1)] == [3] and segments_of(got, 0, 2) == [] and segments_of(got, 1, 2) == []
    assert len(got) == 3                                           # the pairs stay listed
    got = idx.find_shared_content(segments=True, min_segment=4, max_gap=2)
    assert [s.chunks for s in segments_of(got, 0, 1)] == [5] and [s.chunks for s in segments_of(got, 0, 2)] == [4]
    got = idx.find_shared_content(segments=True, min_segment=5, max_gap=2)
    assert [s.chunks for s in segments_of(got, 0, 1)] == [5] and segments_of(got, 0, 2) == []


def test_two_alignments_of_one_pair_and_the_order():
    """Asset 1 holds asset 0's chunks 4..5 at its start and 0..1 behind them: two diagonals; ordered by (offset_a, offset_b)."""
    rng = np.random.default_rng(9)
    c = [rnd(rng) for _ in range(6)]
    assets = [make_asset(rng, 0, simprints={CT: chunks_of(c)}), make_asset(rng, 1, simprints={CT: chunks_of([c[4], c[5], rnd(rng), c[0], c[1]])})]
    got = cpu_index(assets).find_shared_content(segments=True, max_gap=5)
    assert segments_of(got, 0, 1) == [SharedSegment(0, 20, 30, 50, 0, 3, 2, 2, 1.0), SharedSegment(40, 60, 0, 20, 4, 0, 2, 2, 1.0)]


def test_segments_false_is_the_call_it_was(clips):
    plain = cpu_index(clips, OverlapOracleEngine()).find_shared_content()
    assert plain and all(t.segments is None for p in plain for t in p.types.values())
    # a table whose join_segments raises: segments=False never touches it
    assert cpu_index(clips, RefusingEngine()).find_shared_content() == plain
    assert cpu_index(clips, RefusingEngine()).find_shared_content(segments=False, min_segment=9, max_gap=9) == plain
    with pytest.raises(AssertionError, match="reached join_segments"):
        cpu_index(clips, RefusingEngine()).find_shared_content(segments=True)
    located = cpu_index(clips).find_shared_content(segments=True)
    assert located != plain and without_segments(located) == plain


def test_every_type_is_located():
    rng = np.random.default_rng(10)
    c, s = [rnd(rng) for _ in range(4)], [rnd(rng, 16) for _ in range(3)]
    assets = [make_asset(rng, 0, simprints={CT: chunks_of(c), ST: chunks_of(s)}),
              make_asset(rng, 1, simprints={CT: chunks_of([rnd(rng), c[1], c[2]]), ST: chunks_of([flip_bits(s[2], 8)], size=33)})]
    (pair,) = cpu_index(assets).find_shared_content(segments=True)
    assert pair.types[CT].segments == [SharedSegment(10, 30, 10, 30, 1, 1, 2, 2, 1.0)]
    assert pair.types[ST].segments == [SharedSegment(20, 30, 0, 33, 2, 0, 1, 1, 1.0 - 8 / 128)]
    (only,) = cpu_index(assets).find_shared_content(segments=True, simprint_types=[ST])
    assert set(only.types) == {ST} and only.types[ST].segments == pair.types[ST].segments


def test_a_library_sums_up_and_max_pairs_is_surfaced():
    idx = cpu_index(library(np.random.default_rng(21), 45, boiler=0.2))
    got = idx.find_shared_content(segments=True, max_doc_freq=3)
    assert len(got) > 5 and without_segments(got) == idx.find_shared_content(max_doc_freq=3)
    longest = 0
    for p in got:
        for t in p.types.values():
            assert sum(s.chunks for s in t.segments) == t.chunk_pairs and all(s.span == s.chunks for s in t.segments)
            assert t.segments == sorted(t.segments, key=lambda s: (s.offset_a, s.offset_b))
            longest = max([longest] + [s.chunks for s in t.segments])
    assert longest >= 3
    with pytest.raises(ValueError, match="exceed max_pairs"):
        idx.find_shared_content(segments=True, max_pairs=1)


def test_tables_without_the_join_name_the_caller(clips):
    idx = cpu_index(clips, OverlapOracleEngine())                  # join_overlaps, but no join_segments
    assert idx.find_shared_content()
    with pytest.raises(NotImplementedError, match="find_shared_content needs a single-GPU engine"):
        idx.find_shared_content(segments=True)


def test_manager_route_and_sharded_refusal(clips):
    m = HipIndexManager("hip:///", engine=SegmentOracleEngine())
    m.create_index(IsccIndex(name="lib"))
    m.add_assets("lib", clips)
    got = m.find_shared_content("lib", segments=True, min_segment=4, max_gap=2)
    assert got == m._indexes["lib"].find_shared_content(segments=True, min_segment=4, max_gap=2)
    assert [s.chunks for s in segments_of(got, 0, 2)] == [4]
    assert all(t.segments is None for p in m.find_shared_content("lib") for t in p.types.values())
    m.close()
    sharded = HipIndexManager("hip:///?devices=2", engine=SegmentOracleEngine())
    with pytest.raises(NotImplementedError, match="sharded"):
        sharded.find_shared_content("lib", segments=True)
