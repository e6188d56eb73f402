"""
``find_shared_matches``: pairs (asset of one index, asset of another) that share chunks, by a cross join of the two tables of every
simprint type (CPU tier).

The engine is the oracle-backed stand-in with model-backed joins: ``join_overlaps_between`` by ``tests/overlap_between_model.py`` and
``join_overlaps`` by ``tests/overlap_model.py`` (brute force over all row pairs).  What is checked is the host side --
``pairs.shared_matches`` under ``HipIndex.find_shared_matches`` -- against values worked by hand, against itself with the sides swapped
and against ``find_shared_content`` on an index that holds both libraries.
"""

import numpy as np
import pytest

from helpers import flip_bits, make_asset, make_iscc_id
from iscc_search_amd.index import HipIndex, HipIndexManager, HipOptions
from iscc_search_amd.pairs import SharedChunks, SharedMatch
from iscc_search_amd.schema import IsccIndex
from oracle_engine import OracleEngine
from overlap_between_model import SKIP_SAME_ASSET, model_overlaps_between
from test_shared_content import CT, ST, OverlapOracleEngine, OverlapOracleTable, chunks_of, library, rnd


class SharedOracleTable(OverlapOracleTable):
    def join_overlaps_between(self, other, max_hamming, asset_keys_a, asset_keys_b, max_doc_freq, max_pairs, dup_limit=1000, skip_same_asset=True):
        """``HipTable.join_overlaps_between`` answered by the host model."""
        if getattr(other, "engine", None) is not self.engine:
            raise ValueError("join_overlaps_between needs two tables of one engine: the other table belongs to another engine")
        ka, wa, _ = self._arrays()
        kb, wb, _ = other._arrays()
        rc, records, chunks_a, chunks_b, info = model_overlaps_between(
            ka.reshape(-1, 2), wa, kb.reshape(-1, 2), wb, asset_keys_a, asset_keys_b, max_hamming, max_doc_freq, dup_limit,
            SKIP_SAME_ASSET if skip_same_asset else 0)
        assert rc == 0
        if info["chunk_pairs"] > max_pairs:
            raise ValueError(f"{info['chunk_pairs']} chunk pairs exceed max_pairs={max_pairs}")
        return records, chunks_a, chunks_b, info


class SharedOracleEngine(OverlapOracleEngine):
    def open_table(self, metric, key_words, max_bytes):
        t = SharedOracleTable(metric, key_words, max_bytes)
        t.engine = self
        return t


def two_indexes(engine, assets_a, assets_b):
    a, b = HipIndex(engine, HipOptions()), HipIndex(engine, HipOptions())
    a.add_assets(assets_a)
    b.add_assets(assets_b)
    return a, b


@pytest.fixture
def small():
    """A catalogue of four assets (0-3) and a registry of four (2, 10, 11, 12); asset 2 is held by both.  Worked by hand below."""
    rng = np.random.default_rng(14)
    c = [rnd(rng) for _ in range(4)]
    s = [rnd(rng, 16) for _ in range(2)]
    boiler = rnd(rng)
    shared = {CT: chunks_of([c[3], rnd(rng)])}
    cat = [
        make_asset(rng, 0, simprints={CT: chunks_of([c[0], flip_bits(c[1], 4), rnd(rng), rnd(rng)]), ST: chunks_of([s[0], rnd(rng, 16)])}),
        make_asset(rng, 1, simprints={CT: chunks_of([flip_bits(c[2], 2), boiler])}),
        make_asset(rng, 2, simprints=shared),
        make_asset(rng, 3, simprints={CT: chunks_of([rnd(rng), boiler, c[3]])}),
    ]
    reg = [
        make_asset(rng, 2, simprints=shared),
        make_asset(rng, 10, simprints={CT: chunks_of([c[0], c[1]]), ST: chunks_of([flip_bits(s[0], 8)])}),
        make_asset(rng, 11, simprints={CT: chunks_of([c[2], rnd(rng), boiler])}),
        make_asset(rng, 12, simprints={CT: chunks_of([boiler]), ST: chunks_of([s[1]])}),
    ]
    return two_indexes(SharedOracleEngine(), cat, reg)


def by_ids(result):
    return {(r.iscc_id_a, r.iscc_id_b): r for r in result}


def swapped(result):
    """The result with its sides exchanged, in the order find_shared_matches gives."""
    from iscc_search_amd import codec

    out = [SharedMatch(r.iscc_id_b, r.iscc_id_a, r.score,
                       {t: SharedChunks(v.matched_b, v.chunks_b, v.matched_a, v.chunks_a, v.chunk_pairs, v.coverage_b, v.coverage_a) for t, v in r.types.items()})
           for r in result]
    out.sort(key=lambda r: (-r.score, codec.iscc_id_to_int(r.iscc_id_a), codec.iscc_id_to_int(r.iscc_id_b)))
    return out


def test_coverage_score_and_order_worked_by_hand(small):
    from iscc_search_amd import codec

    a, b = small
    ids = {i: make_iscc_id(i) for i in (0, 1, 2, 3, 10, 11, 12)}
    got = a.find_shared_matches(b)
    r = by_ids(got)
    assert set(r) == {(ids[0], ids[10]), (ids[1], ids[11]), (ids[1], ids[12]), (ids[3], ids[2]), (ids[3], ids[11]), (ids[3], ids[12])}
    # 0 and 10: CONTENT two chunks at distances 0 and 4 of 64 bits; SEMANTIC one chunk at distance 8 of 128
    p = r[(ids[0], ids[10])]
    assert p.types[CT] == SharedChunks(2, 4, 2, 2, 2, (2 - 4 / 64) / 4, (2 - 4 / 64) / 2)
    assert p.types[ST] == SharedChunks(1, 2, 1, 1, 1, (1 - 8 / 128) / 2, 1 - 8 / 128)
    assert p.score == ((2 - 4 / 64) / 2 + (1 - 8 / 128)) / 2
    # 1 and 11: one chunk at distance 2 and the boilerplate chunk
    assert r[(ids[1], ids[11])].types == {CT: SharedChunks(2, 2, 2, 3, 2, (2 - 2 / 64) / 2, (2 - 2 / 64) / 3)}
    assert r[(ids[1], ids[12])].types == {CT: SharedChunks(1, 2, 1, 1, 1, 0.5, 1.0)} and r[(ids[1], ids[12])].score == 1.0
    # 3 holds a chunk of asset 2 as the registry has it; asset 2 of the catalogue does not pair with itself
    assert r[(ids[3], ids[2])].types == {CT: SharedChunks(1, 3, 1, 2, 1, 1 / 3, 1 / 2)}
    assert all(isinstance(p, SharedMatch) for p in got)
    order = [(-p.score, codec.iscc_id_to_int(p.iscc_id_a), codec.iscc_id_to_int(p.iscc_id_b)) for p in got]
    assert order == sorted(order)


def test_the_sides_swapped(small):
    a, b = small
    for kwargs in ({}, {"max_doc_freq": 1}, {"include_same_id": True}, {"threshold": 0.95}, {"min_chunks": 2}):
        got = a.find_shared_matches(b, **kwargs)
        assert got and b.find_shared_matches(a, **kwargs) == swapped(got), kwargs


def test_stop_chunks_per_index_and_include_same_id(small):
    a, b = small
    ids = {i: make_iscc_id(i) for i in (0, 1, 2, 3, 10, 11, 12)}
    # the boilerplate chunk is held by two assets of either index: above a cut of 1 on both sides.  So is, in the catalogue alone,
    # the chunk of asset 2 that asset 3 holds: the registry's one copy of it finds nothing to pair with
    cut = by_ids(a.find_shared_matches(b, max_doc_freq=1))
    assert set(cut) == {(ids[0], ids[10]), (ids[1], ids[11])}
    assert cut[(ids[1], ids[11])].types == {CT: SharedChunks(1, 2, 1, 3, 1, (1 - 2 / 64) / 2, (1 - 2 / 64) / 3)}      # stop chunks still count
    assert by_ids(a.find_shared_matches(b, max_doc_freq=2)).keys() == by_ids(a.find_shared_matches(b, max_doc_freq=0)).keys()
    same = by_ids(a.find_shared_matches(b, include_same_id=True))
    assert set(same) - set(by_ids(a.find_shared_matches(b))) == {(ids[2], ids[2])}
    assert same[(ids[2], ids[2])].types == {CT: SharedChunks(2, 2, 2, 2, 2, 1.0, 1.0)} and same[(ids[2], ids[2])].score == 1.0


def test_min_chunks_min_coverage_simprint_types_and_threshold(small):
    a, b = small
    ids = {i: make_iscc_id(i) for i in (0, 1, 2, 3, 10, 11, 12)}
    full = a.find_shared_matches(b)
    assert {(p.iscc_id_a, p.iscc_id_b) for p in a.find_shared_matches(b, min_chunks=2)} == {(ids[0], ids[10]), (ids[1], ids[11])}
    assert a.find_shared_matches(b, min_chunks=3) == []
    assert a.find_shared_matches(b, min_coverage=0.9) == [p for p in full if p.score >= 0.9]
    assert 0 < len(a.find_shared_matches(b, min_coverage=0.9)) < len(full)
    only = a.find_shared_matches(b, simprint_types=[ST])
    assert [(p.iscc_id_a, p.iscc_id_b) for p in only] == [(ids[0], ids[10])] and set(only[0].types) == {ST}
    assert only[0].score == 1 - 8 / 128                            # the mean over the types joined
    assert a.find_shared_matches(b, simprint_types=["NOPE"]) == []
    # a stricter threshold: distance 4 of 64 bits scores 0.9375, distance 2 scores 0.96875
    strict = by_ids(a.find_shared_matches(b, threshold=0.95, simprint_types=[CT]))
    assert strict[(ids[0], ids[10])].types[CT] == SharedChunks(1, 4, 1, 2, 1, 1 / 4, 1 / 2)
    assert (ids[1], ids[11]) in strict
    # the default threshold is the OTHER index's
    b._opts.match_threshold_simprints = 0.95
    assert by_ids(a.find_shared_matches(b, simprint_types=[CT])) == strict
    assert by_ids(b.find_shared_matches(a, simprint_types=[CT])) != by_ids(swapped(list(strict.values())))


def test_disjoint_libraries_equal_the_cross_pairs_of_find_shared_content():
    from iscc_search_amd import codec

    rng = np.random.default_rng(23)
    assets = library(rng, 60, boiler=0.2)
    perm = rng.permutation(60)
    in_a = set(perm[:28].tolist())
    engine = SharedOracleEngine()
    a, b = two_indexes(engine, [x for i, x in enumerate(assets) if i in in_a], [x for i, x in enumerate(assets) if i not in in_a])
    both = HipIndex(engine, HipOptions())
    both.add_assets(assets)
    ids_a = {x.iscc_id for i, x in enumerate(assets) if i in in_a}
    for kwargs in ({}, {"threshold": 0.9}, {"min_chunks": 2}):
        exp = []
        for p in both.find_shared_content(max_doc_freq=0, **kwargs):
            if (p.iscc_id_a in ids_a) == (p.iscc_id_b in ids_a):
                continue                                       # both assets of one library
            if p.iscc_id_a in ids_a:
                exp.append(SharedMatch(p.iscc_id_a, p.iscc_id_b, p.score, p.types))
            else:
                exp.extend(swapped([SharedMatch(p.iscc_id_a, p.iscc_id_b, p.score, p.types)]))
        exp.sort(key=lambda r: (-r.score, codec.iscc_id_to_int(r.iscc_id_a), codec.iscc_id_to_int(r.iscc_id_b)))
        got = a.find_shared_matches(b, max_doc_freq=0, **kwargs)
        assert len(got) > 5 and got == exp, kwargs


def test_each_side_builds_ids_with_its_own_realm(small):
    a, b = small
    b._realm_id = 1
    got = a.find_shared_matches(b)
    assert got and all(p.iscc_id_a == make_iscc_id_of(p.iscc_id_a, 0) and p.iscc_id_b == make_iscc_id_of(p.iscc_id_b, 1) for p in got)


def make_iscc_id_of(iscc_id, realm):
    from iscc_search_amd import codec

    return codec.iscc_id_from_int(codec.iscc_id_to_int(iscc_id), realm)


def test_max_pairs_is_surfaced(small):
    a, b = small
    with pytest.raises(ValueError, match="exceed max_pairs"):
        a.find_shared_matches(b, max_pairs=1)
    with pytest.raises(ValueError, match="8 chunk pairs exceed max_pairs=7"):
        a.find_shared_matches(b, max_pairs=7)
    assert len(a.find_shared_matches(b, max_pairs=8)) == 6         # CONTENT has 8 chunk pairs within the default cut, SEMANTIC 1


def test_refusals(small):
    a, b = small
    with pytest.raises(ValueError, match="find_shared_content lists the pairs within one"):
        a.find_shared_matches(a)
    rng = np.random.default_rng(6)
    elsewhere = HipIndex(SharedOracleEngine(), HipOptions())
    elsewhere.add_assets(library(rng, 4))
    with pytest.raises(ValueError, match="one engine"):
        a.find_shared_matches(elsewhere)
    # CONTENT simprints of 128 bits against the catalogue's 64
    wide = HipIndex(a._engine, HipOptions())
    wide.add_assets(library(rng, 4, nbytes=16))
    with pytest.raises(ValueError, match="one length"):
        a.find_shared_matches(wide, simprint_types=[CT])


def test_tables_without_the_join_name_the_caller():
    rng = np.random.default_rng(4)
    a, b = two_indexes(OracleEngine(), library(rng, 5), library(rng, 5, first=100))      # tables without the join, as a sharded engine's
    with pytest.raises(NotImplementedError, match="find_shared_matches needs a single-GPU engine"):
        a.find_shared_matches(b)
    a, b = two_indexes(OverlapOracleEngine(), library(rng, 5), library(rng, 5, first=100))   # the self-join alone does not do
    with pytest.raises(NotImplementedError, match="find_shared_matches needs a single-GPU engine"):
        a.find_shared_matches(b)


def test_manager_route_sharded_refusal_and_one_name_twice():
    rng = np.random.default_rng(3)
    m = HipIndexManager("hip:///", engine=SharedOracleEngine())
    m.create_index(IsccIndex(name="cat"))
    m.create_index(IsccIndex(name="reg"))
    assets = library(rng, 40)
    m.add_assets("cat", assets[:20])
    m.add_assets("reg", assets[20:])
    got = m.find_shared_matches("cat", "reg", min_chunks=1, max_doc_freq=50)
    assert got and got == m._indexes["cat"].find_shared_matches(m._indexes["reg"], min_chunks=1, max_doc_freq=50)
    with pytest.raises(ValueError, match="'cat' twice"):
        m.find_shared_matches("cat", "cat")
    with pytest.raises(FileNotFoundError):
        m.find_shared_matches("cat", "nope")
    m.close()
    sharded = HipIndexManager("hip:///?devices=2", engine=SharedOracleEngine())
    with pytest.raises(NotImplementedError, match="sharded"):
        sharded.find_shared_matches("cat", "reg")
