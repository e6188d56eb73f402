"""
``find_shared_content``: asset pairs that share chunks, by a self-join of every simprint table (CPU tier).

The engine is the oracle-backed stand-in with a model-backed ``join_overlaps`` (``tests/overlap_model.py``: brute force over all row
pairs).  What is checked is the host side -- ``pairs.shared_content`` under ``HipIndex.find_shared_content`` -- against values worked
by hand and against the definition spelled out over the index's own simprints.
"""

import numpy as np
import pytest

from helpers import flip_bits, make_asset, make_iscc_id, sp
from iscc_search_amd import codec
from iscc_search_amd.index import HipIndex, HipIndexManager, HipOptions
from iscc_search_amd.pairs import SharedChunks, SharedContent
from iscc_search_amd.schema import IsccIndex
from oracle_engine import OracleEngine, OracleTable
from overlap_model import model_overlaps

CT, ST = "CONTENT_TEXT_V0", "SEMANTIC_TEXT_V0"


class OverlapOracleTable(OracleTable):
    def join_overlaps(self, max_hamming, asset_keys, max_doc_freq, max_pairs, dup_limit=1000):
        """``HipTable.join_overlaps`` answered by the host model."""
        keys, words, _ = self._arrays()
        rc, records, chunks, info = model_overlaps(keys.reshape(-1, 2), words, asset_keys, max_hamming, max_doc_freq, dup_limit)
        assert rc == 0
        if info["chunk_pairs"] > max_pairs:
            raise ValueError(f"{info['chunk_pairs']} chunk pairs exceed max_pairs={max_pairs}")
        return records, chunks, info


class OverlapOracleEngine(OracleEngine):
    def open_table(self, metric, key_words, max_bytes):
        t = OverlapOracleTable(metric, key_words, max_bytes)
        t.engine = self
        return t


def rnd(rng, nbytes=8):
    return rng.integers(0, 256, size=nbytes, dtype=np.uint8).tobytes()


def chunks_of(codes, size=10):
    return [sp(c, i * size, size) for i, c in enumerate(codes)]


def hamming(a, b):
    return bin(int.from_bytes(a, "big") ^ int.from_bytes(b, "big")).count("1")


def definition(index, threshold=None, max_doc_freq=100, simprint_types=None):
    """{(id_a, id_b): {sp_type: SharedChunks}} spelled out over the index's own simprints (``_sp_assets``), asset pair by asset pair."""
    threshold = index._opts.match_threshold_simprints if threshold is None else threshold
    out = {}
    for sp_type, by_body in index._sp_assets.items():
        if simprint_types is not None and sp_type not in simprint_types:
            continue
        ndim = index._sp_tables[sp_type].ndim
        holders = {}
        for body, pairs in by_body.items():
            for code in {c for c, _ in pairs}:
                holders[code] = holders.get(code, 0) + 1
        usable = {body: [c for c, _ in pairs if not (max_doc_freq and holders[c] > max_doc_freq)] for body, pairs in by_body.items()}
        bodies = sorted(by_body)
        for x, a in enumerate(bodies):
            for b in bodies[x + 1:]:
                best_a = [min((hamming(c, d) for d in usable[b]), default=ndim + 1) for c in usable[a]]
                best_b = [min((hamming(c, d) for c in usable[a]), default=ndim + 1) for d in usable[b]]
                hit_a = [h for h in best_a if 1.0 - h / ndim >= threshold and h <= ndim]
                hit_b = [h for h in best_b if 1.0 - h / ndim >= threshold and h <= ndim]
                if not hit_a:
                    continue
                n_pairs = sum(1 for c in usable[a] for d in usable[b] if 1.0 - hamming(c, d) / ndim >= threshold)
                ids = tuple(codec.iscc_id_from_int(int.from_bytes(k, "big"), index._realm_id or 0) for k in (a, b))
                out.setdefault(ids, {})[sp_type] = SharedChunks(
                    len(hit_a), len(by_body[a]), len(hit_b), len(by_body[b]), n_pairs,
                    (len(hit_a) - sum(hit_a) / ndim) / len(by_body[a]), (len(hit_b) - sum(hit_b) / ndim) / len(by_body[b]))
    return out


def library(rng, n, first=0, chunks=(2, 9), nbytes=8, reuse=0.5, boiler=0.0):
    """n assets of one simprint type; about ``reuse`` of them contain a run of an earlier asset's chunks, some with flipped bits."""
    assets, runs = [], []
    boilerplate = rnd(rng, nbytes)
    for i in range(n):
        codes = [rnd(rng, nbytes) for _ in range(int(rng.integers(chunks[0], chunks[1])))]
        if runs and rng.random() < reuse:
            src = runs[int(rng.integers(0, len(runs)))]
            lo = int(rng.integers(0, len(src)))
            run = [flip_bits(c, int(rng.integers(0, 6))) for c in src[lo:lo + int(rng.integers(1, 6))]]
            at = int(rng.integers(0, len(codes) + 1))
            codes = codes[:at] + run + codes[at:]
        if rng.random() < boiler:
            codes.append(boilerplate)
        runs.append(codes)
        assets.append(make_asset(rng, first + i, simprints={CT: chunks_of(codes)}))
    return assets


@pytest.fixture
def small():
    """Six assets whose overlaps are worked by hand in the tests below."""
    rng = np.random.default_rng(12)
    c = [rnd(rng) for _ in range(4)]
    s = [rnd(rng, 16) for _ in range(3)]
    boiler = rnd(rng)
    sims = [
        {CT: chunks_of(c), ST: chunks_of(s[:2])},                                                   # 0
        {CT: chunks_of([c[0], flip_bits(c[1], 4)]), ST: chunks_of([s[1]])},                          # 1: two of 0's chunks, and s1
        {CT: chunks_of([flip_bits(c[2], 2), rnd(rng), rnd(rng)])},                                   # 2: one of 0's chunks
        {CT: chunks_of([rnd(rng), boiler]), ST: chunks_of([flip_bits(s[0], 8), s[2]])},              # 3: 0's s0 in SEMANTIC only
        {CT: chunks_of([rnd(rng), boiler])},                                                         # 4
        {CT: chunks_of([boiler, rnd(rng), rnd(rng)])},                                               # 5
    ]
    idx = HipIndex(OverlapOracleEngine(), HipOptions())
    idx.add_assets([make_asset(rng, i, simprints=sim) for i, sim in enumerate(sims)])
    return idx


def by_ids(result):
    return {(r.iscc_id_a, r.iscc_id_b): r for r in result}


def test_coverage_score_and_order_worked_by_hand(small):
    got = small.find_shared_content()
    ids = [make_iscc_id(i) for i in range(6)]
    r = by_ids(got)
    assert set(r) == {(ids[0], ids[1]), (ids[0], ids[2]), (ids[0], ids[3]), (ids[3], ids[4]), (ids[3], ids[5]), (ids[4], ids[5])}
    # 0 and 1: CONTENT two chunks at distances 0 and 4 of 64 bits; SEMANTIC one chunk at distance 0
    p = r[(ids[0], ids[1])]
    assert p.types[CT] == SharedChunks(2, 4, 2, 2, 2, (2 - 4 / 64) / 4, (2 - 4 / 64) / 2)
    assert p.types[ST] == SharedChunks(1, 2, 1, 1, 1, 1 / 2, 1.0)
    assert p.score == ((2 - 4 / 64) / 2 + 1.0) / 2
    # 0 and 2: one chunk at distance 2; the smaller asset's coverage is the type's score
    p = r[(ids[0], ids[2])]
    assert p.types == {CT: SharedChunks(1, 4, 1, 3, 1, (1 - 2 / 64) / 4, (1 - 2 / 64) / 3)} and p.score == (1 - 2 / 64) / 3
    # 0 and 3: a pair in SEMANTIC only (128 bits, distance 8): the mean runs over that one type
    p = r[(ids[0], ids[3])]
    assert p.types == {ST: SharedChunks(1, 2, 1, 2, 1, (1 - 8 / 128) / 2, (1 - 8 / 128) / 2)} and p.score == (1 - 8 / 128) / 2
    # the boilerplate chunk of 3, 4 and 5
    assert r[(ids[3], ids[4])].types == {CT: SharedChunks(1, 2, 1, 2, 1, 0.5, 0.5)}
    assert r[(ids[4], ids[5])].types == {CT: SharedChunks(1, 2, 1, 3, 1, 1 / 2, 1 / 3)}
    # score descending, then (key_a, key_b)
    order = [(-p.score, codec.iscc_id_to_int(p.iscc_id_a), codec.iscc_id_to_int(p.iscc_id_b)) for p in got]
    assert order == sorted(order)
    assert all(isinstance(p, SharedContent) and codec.iscc_id_to_int(p.iscc_id_a) < codec.iscc_id_to_int(p.iscc_id_b) for p in got)
    assert {(p.iscc_id_a, p.iscc_id_b): p.types for p in got} == definition(small)


def test_stop_chunks_still_count_as_chunks(small):
    ids = [make_iscc_id(i) for i in range(6)]
    r = by_ids(small.find_shared_content(max_doc_freq=2))          # three assets hold the boilerplate chunk: above the cut
    assert set(r) == {(ids[0], ids[1]), (ids[0], ids[2]), (ids[0], ids[3])}
    assert by_ids(small.find_shared_content(max_doc_freq=3)).keys() == by_ids(small.find_shared_content(max_doc_freq=0)).keys()
    assert len(by_ids(small.find_shared_content(max_doc_freq=3))) == 6
    assert {k: p.types for k, p in r.items()} == definition(small, max_doc_freq=2)


def test_min_chunks_min_coverage_and_simprint_types(small):
    full = small.find_shared_content()
    ids = [make_iscc_id(i) for i in range(6)]
    assert [(p.iscc_id_a, p.iscc_id_b) for p in small.find_shared_content(min_chunks=2)] == [(ids[0], ids[1])]
    assert small.find_shared_content(min_chunks=3) == []
    assert small.find_shared_content(min_coverage=0.5) == [p for p in full if p.score >= 0.5]
    assert 0 < len(small.find_shared_content(min_coverage=0.5)) < len(full)
    only = small.find_shared_content(simprint_types=[ST])
    assert {(p.iscc_id_a, p.iscc_id_b) for p in only} == {(ids[0], ids[1]), (ids[0], ids[3])}
    assert all(set(p.types) == {ST} for p in only)
    assert by_ids(only)[(ids[0], ids[1])].score == 1.0             # the mean over the types joined
    assert small.find_shared_content(simprint_types=["NOPE"]) == []
    # a stricter threshold: distance 4 of 64 bits scores 0.9375, distance 2 scores 0.96875
    strict = by_ids(small.find_shared_content(threshold=0.95, simprint_types=[CT]))
    assert strict[(ids[0], ids[1])].types[CT] == SharedChunks(1, 4, 1, 2, 1, 1 / 4, 1 / 2)
    assert (ids[0], ids[2]) in strict


def test_an_updated_assets_old_chunks_are_gone(small):
    rng = np.random.default_rng(5)
    ids = [make_iscc_id(i) for i in range(6)]
    fresh = [rnd(rng), rnd(rng), rnd(rng)]
    small.add_assets([make_asset(rng, 1, simprints={CT: chunks_of(fresh)})])
    r = by_ids(small.find_shared_content())
    assert set(r[(ids[0], ids[1])].types) == {ST}                  # its CONTENT chunks no longer match; SEMANTIC was not updated
    assert {k: p.types for k, p in r.items()} == definition(small)
    small.add_assets([make_asset(rng, 2, simprints={CT: chunks_of([fresh[0], fresh[2]])})])
    r = by_ids(small.find_shared_content())
    assert (ids[0], ids[2]) not in r
    assert r[(ids[1], ids[2])].types == {CT: SharedChunks(2, 3, 2, 2, 2, 2 / 3, 1.0)}


def test_a_library_equals_the_definition():
    rng = np.random.default_rng(21)
    idx = HipIndex(OverlapOracleEngine(), HipOptions())
    idx.add_assets(library(rng, 45, boiler=0.2))
    for kwargs in ({}, {"max_doc_freq": 3}, {"threshold": 0.9}, {"threshold": 1.0, "max_doc_freq": 0}):
        got = idx.find_shared_content(**kwargs)
        exp = definition(idx, kwargs.get("threshold"), kwargs.get("max_doc_freq", 100))
        assert len(got) > 5
        assert {(p.iscc_id_a, p.iscc_id_b): p.types for p in got} == exp
        for p in got:
            scores = [max(t.coverage_a, t.coverage_b) for t in p.types.values()]
            assert p.score == sum(scores) / len(scores)


def test_max_pairs_is_surfaced(small):
    with pytest.raises(ValueError, match="exceed max_pairs"):
        small.find_shared_content(max_pairs=1)
    with pytest.raises(ValueError, match="6 chunk pairs exceed max_pairs=5"):
        small.find_shared_content(max_pairs=5)
    assert len(small.find_shared_content(max_pairs=6)) == 6        # CONTENT has 6 chunk pairs within the default cut, SEMANTIC 2


def test_manager_route_and_sharded_refusal():
    rng = np.random.default_rng(3)
    m = HipIndexManager("hip:///", engine=OverlapOracleEngine())
    m.create_index(IsccIndex(name="lib"))
    m.add_assets("lib", library(rng, 25))
    got = m.find_shared_content("lib", min_chunks=2, max_doc_freq=50)
    assert got and got == m._indexes["lib"].find_shared_content(min_chunks=2, max_doc_freq=50)
    with pytest.raises(FileNotFoundError):
        m.find_shared_content("nope")
    m.close()
    sharded = HipIndexManager("hip:///?devices=2", engine=OverlapOracleEngine())
    with pytest.raises(NotImplementedError, match="sharded"):
        sharded.find_shared_content("lib")


def test_tables_without_the_join_name_the_caller():
    rng = np.random.default_rng(4)
    idx = HipIndex(OracleEngine(), HipOptions())                   # a table that has no join_overlaps, as a sharded engine's
    idx.add_assets(library(rng, 5))
    with pytest.raises(NotImplementedError, match="find_shared_content needs a single-GPU engine"):
        idx.find_shared_content()
