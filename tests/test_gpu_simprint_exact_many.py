"""
``isccsearch_simprint_exact_many`` (many hard-boundary simprint requests looked up and scored in one library call, requests
kept apart): ``HipSimprintIndex.search_exact_many`` must return, request by request, exactly what the request gives alone --
``_search_exact_device`` (``isccsearch_simprint_exact``) and ``_search_exact_host`` (sequential float64 sums on the host) --
compared with ``==`` on ``(iscc_id_body, score, queried, matches, chunks...)``; one library search per round, not per request;
and the hard-boundary simprint part of ``search_assets_many`` what ``search_assets`` returns per query.
"""

import os

import numpy as np
import pytest

from helpers import hip_manager, make_iscc_id, sp
from iscc_search_amd import codec
from iscc_search_amd._lib import MAX_SCORED_SIMPRINTS
from iscc_search_amd.schema import IsccEntry, IsccIndex, IsccQuery
from iscc_search_amd.simprint import HipSimprintIndex, pack_chunk_pointer

pytestmark = pytest.mark.gpu

N_SEEDS = int(os.environ.get("ISCC_FUZZ_SEEDS", "8"))
# a limit that cuts, a threshold that drops, dup_limit below and above the collision counts
ROWS = ((10, 0.0, 1000), (3, 0.0, 25), (50, 0.2, 70), (1000, 0.05, 1000), (5, 0.9, 1))


def _key(results):
    return [[(r.iscc_id_body, r.score, r.queried, r.matches,
              None if r.chunks is None else [(c.query, c.match, c.score, c.offset, c.size, c.freq) for c in r.chunks]) for r in res]
            for res in results]


def _skewed(hip_engine, ndim, rows, pool_size=30, seed=0):
    """The skewed-pool corpus: a few simprints collide hundreds of times, most a few times; asset ids include 0 and 2^64 - 1."""
    rng = np.random.default_rng(7000 + ndim + seed)
    nb = ndim // 8
    pool = [rng.integers(0, 256, size=nb, dtype=np.uint8).tobytes() for _ in range(pool_size)]
    keys, vecs, seen = [], [], set()
    ids = [0xFFFFFFFFFFFFFFFF, 0] + list(range(1, 120))
    while len(keys) < rows:
        body = ids[int(rng.integers(0, len(ids)))].to_bytes(8, "big")
        off, size = int(rng.integers(0, 60 * max(1, rows // 2500))), int(rng.integers(1, 4))
        if (body, off, size) in seen:
            continue
        seen.add((body, off, size))
        spr = pool[min(int(rng.exponential(4.0)), len(pool) - 1)]
        keys.append(pack_chunk_pointer(body, off, size))
        vecs.append(np.frombuffer(spr, dtype=np.uint8))
    index = HipSimprintIndex(hip_engine, ndim=ndim)
    index.add_raw(keys, vecs)
    absent = [rng.integers(0, 256, size=nb, dtype=np.uint8).tobytes() for _ in range(24)]
    return index, pool, absent


@pytest.fixture(scope="module")
def skewed(hip_engine):
    built = {ndim: _skewed(hip_engine, ndim, 2500) for ndim in (64, 128, 256)}
    yield built
    for index, _, _ in built.values():
        index.close()


@pytest.fixture(scope="module")
def wide(hip_engine):
    """About 4 200 distinct simprints over 5 000 rows of 150 assets: every pool simprint is stored, most once."""
    rng = np.random.default_rng(31)
    pool = [rng.integers(0, 256, size=16, dtype=np.uint8).tobytes() for _ in range(4200)]
    keys = [pack_chunk_pointer((1 + (i * 7) % 150).to_bytes(8, "big"), i, 1) for i in range(5000)]
    vecs = [np.frombuffer(pool[i % len(pool)], dtype=np.uint8) for i in range(5000)]
    index = HipSimprintIndex(hip_engine, ndim=128)
    index.add_raw(keys, vecs)
    yield index, pool
    index.close()


def _mix(pool, absent):
    """The requests of one round; see the test below for what each is there for."""
    return [
        [pool[0]],                                                          # 0: one simprint; score 1.0 for many assets: ties
        [],                                                                 # 1: empty
        [b"\x01\x02\x03"],                                                  # 2: only a simprint of another length
        [pool[0], pool[1], pool[0], pool[5], absent[0], pool[29], b"\x01\x02\x03"],   # 3: repeats, an absent one, queried counts the wrong length
        [pool[0], pool[2]],                                                 # 4: pool[0] again: its assets have runs in several requests
        [pool[1]],                                                          # 5: kept at every threshold of ROWS
        [pool[2]] + absent[1:20],                                           # 6: coverage 1 / 20: every asset below 0.2
        [pool[3]],                                                          # 7: kept
        [pool[i % 30] for i in range(70)],                                  # 8: 70 simprints, 30 distinct
        [pool[4], pool[7], pool[4]],                                        # 9 and 10: identical content
        [pool[4], pool[7], pool[4]],
        [absent[20]],                                                       # 11: matches nothing
    ]


def _alone(index, reqs, limit, threshold, dup_limit):
    """Every request by itself, on the device and on the host (which must agree), detailed."""
    nb = index.ndim // 8
    out = []
    for query in reqs:
        distinct = [s for s in dict.fromkeys(query) if len(s) == nb]
        if not query or not distinct or len(query) > MAX_SCORED_SIMPRINTS:
            out.append(index.search_exact(query, limit=limit, threshold=threshold, detailed=True, dup_limit=dup_limit))
            continue
        host = index._search_exact_host(query, distinct, limit, threshold, True, dup_limit)
        device = index._search_exact_device(query, distinct, limit, threshold, True, dup_limit)
        assert _key([device]) == _key([host])
        out.append(host)
    return out


def _plain(results):
    return [[(r.iscc_id_body, r.score, r.queried, r.matches, None) for r in res] for res in results]


@pytest.mark.parametrize("ndim", [64, 128, 256])
def test_a_round_of_mixed_requests_equals_every_request_alone(skewed, ndim):
    index, pool, absent = skewed[ndim]
    reqs = _mix(pool, absent)
    for limit, threshold, dup_limit in ROWS:
        want = _alone(index, reqs, limit, threshold, dup_limit)
        got = index.search_exact_many(reqs, limit=limit, threshold=threshold, detailed=True, dup_limit=dup_limit)
        assert _key(got) == _key(want), (limit, threshold, dup_limit)
        plain = index.search_exact_many(reqs, limit=limit, threshold=threshold, detailed=False, dup_limit=dup_limit)
        assert _key(plain) == _plain(want), (limit, threshold, dup_limit)
        assert got[1] == [] and got[2] == [] and got[11] == []
        assert got[0] and got[5] and got[7]
        assert all(r.queried == 7 for r in got[3]) and (threshold > 0.5 or got[3])
        assert _key([got[9]]) == _key([got[10]]) and (threshold > 0.5 or got[9])
        if threshold >= 0.2:
            assert got[6] == []                                             # dropped between two requests that keep theirs
        # ties in score come out in ascending asset order
        scores = [r.score for r in got[0]]
        if len(scores) > 1:
            assert len(scores) != len(set(scores))
        for res in got:
            for a, b in zip(res, res[1:]):
                assert (-a.score, a.iscc_id_body) < (-b.score, b.iscc_id_body)
    # an asset has runs in two requests of the round
    got = index.search_exact_many(reqs, limit=1000, detailed=False)
    assert {r.iscc_id_body for r in got[0]} <= {r.iscc_id_body for r in got[4]}


def test_a_table_the_scan_path_answers(hip_engine):
    """20 011 rows: past ``tiny_rows``, the scan path feeds the sink instead of the one-launch search."""
    index, pool, absent = _skewed(hip_engine, 128, 20011, seed=1)
    reqs = _mix(pool, absent)
    for limit, threshold, dup_limit in ((10, 0.0, 1000), (50, 0.2, 70)):
        want = _alone(index, reqs, limit, threshold, dup_limit)
        assert _key(index.search_exact_many(reqs, limit=limit, threshold=threshold, detailed=True, dup_limit=dup_limit)) == _key(want)
    index.close()


@pytest.mark.parametrize("sizes", [(3, 64, 65, 2048), (2049, 3, 3, 3), (3, 3, 3, 4096), (4097, 3, 3, 3)], ids=lambda s: "-".join(map(str, s)))
def test_lds_rows_are_per_request_at_every_block_size(wide, hip_engine, sizes):
    """
    A request's LDS row holds ceil(distinct / 64) words: 64 and 65 distinct simprints are one and two words; the largest request of
    a round decides the launch -- 32 words (256 threads), 33 and 64 (128), 65 (64).  Every pool simprint is stored, so each request
    is matched at its highest local index; the 3-simprint request of the same round shows the row is the request's own.
    """
    index, pool = wide
    reqs = [[pool[(11 * j + i) % len(pool)] for i in range(n)] for j, n in enumerate(sizes)]
    want = _alone(index, reqs, 200, 0.0, 1000)                              # (150 assets: every one is listed)
    before = hip_engine.stats()["searches"]
    got = index.search_exact_many(reqs, limit=200, threshold=0.0, detailed=True, dup_limit=1000)
    assert hip_engine.stats()["searches"] - before == 1
    assert _key(got) == _key(want) and all(got)
    for query, res in zip(reqs, got):
        assert any(c.query == query[-1] for r in res for c in r.chunks)


def test_one_library_search_per_round_not_per_request(wide, hip_engine):
    index, pool = wide
    reqs = [[pool[(211 * j + i) % len(pool)] for i in range(500)] for j in range(20)]
    kw = dict(limit=8, threshold=0.0, detailed=True, dup_limit=1000)
    before = hip_engine.stats()["searches"]
    got = index.search_exact_many(reqs, **kw)
    assert hip_engine.stats()["searches"] - before == 2                     # 10 000 given simprints: rounds of 16 and 4 requests
    assert _key(got) == _key(_alone(index, reqs, 8, 0.0, 1000)) and all(got)


def test_lookups_of_a_round_span_several_search_batches(wide):
    """More than 1 024 distinct simprints in a round: hits and offsets are prepared after the search, not behind its one batch."""
    index, pool = wide
    reqs = [pool[:600] + pool[:50], pool[300:900], [pool[5]], [pool[4100], pool[5]]]
    got = index.search_exact_many(reqs, limit=30, threshold=0.0, detailed=True)
    assert _key(got) == _key(_alone(index, reqs, 30, 0.0, 1000)) and all(got)


def test_rounds_that_mix_the_single_and_the_many_pipeline(wide, hip_engine):
    """6 000 + 1 000 + 1 000 given simprints are a round of three requests, the 8 000 behind them a round of one; then a request too large for any."""
    index, pool = wide
    mixed = [[pool[(i + 97 * j) % len(pool)] for i in range(n)] for j, n in enumerate((6000, 1000, 1000, 8000))]
    before = hip_engine.stats()["searches"]
    got = index.search_exact_many(mixed, limit=2, threshold=0.0, detailed=True)
    assert hip_engine.stats()["searches"] - before == 2
    assert _key(got) == _key(_alone(index, mixed, 2, 0.0, 1000))
    huge = [pool[i % len(pool)] for i in range(MAX_SCORED_SIMPRINTS + 10)]
    small = [[pool[1], pool[2]], [pool[3]], [pool[2], pool[4000]], [pool[7], pool[7]]]
    reqs = small[:2] + [huge] + small[2:]
    got = index.search_exact_many(reqs, limit=5, threshold=0.0, detailed=True)
    assert _key(got) == _key(_alone(index, reqs, 5, 0.0, 1000)) and all(got)


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_fuzz_random_request_mixes(skewed, wide, seed):
    rng = np.random.default_rng(900 + seed)
    if seed % 2:
        index, pool = wide
        absent = [rng.integers(0, 256, size=16, dtype=np.uint8).tobytes() for _ in range(4)]
    else:
        index, pool, absent = skewed[(64, 128, 256)[(seed // 2) % 3]]
    reqs = []
    for _ in range(int(rng.integers(2, 24))):
        n = int(rng.choice([0, 1, 2, 5, 17, 64, 65, 130, 300]))
        query = [pool[int(i)] for i in rng.integers(0, len(pool), n)]
        for _ in range(int(rng.integers(0, 3))):
            query.insert(int(rng.integers(0, len(query) + 1)), absent[int(rng.integers(0, len(absent)))] if rng.integers(0, 2) else b"\x07\x07")
        reqs.append(query)
    limit, threshold, dup_limit = ROWS[int(rng.integers(0, len(ROWS)))]
    detailed = bool(rng.integers(0, 2))
    want = _alone(index, reqs, limit, threshold, dup_limit)
    got = index.search_exact_many(reqs, limit=limit, threshold=threshold, detailed=detailed, dup_limit=dup_limit)
    assert _key(got) == (_key(want) if detailed else _plain(want))


# -- through the product ---------------------------------------------------------------------------------------------------------

def _sp_assets(n, seed=21):
    rng = np.random.default_rng(seed)
    base = [rng.integers(0, 256, size=8, dtype=np.uint8).tobytes() for _ in range(8)]
    meta_base = [rng.integers(0, 256, size=8, dtype=np.uint8).tobytes() for _ in range(3)]
    assets = []
    for i in range(n):
        units = [codec.encode_unit(codec.MT_META, 0, 0, meta_base[i % 3]),
                 codec.encode_unit(codec.MT_INSTANCE, 0, 0, rng.integers(0, 256, size=8, dtype=np.uint8).tobytes())]
        sps = {"CONTENT_TEXT_V0": [sp(base[(i + j) % 8], 10 * j, 10) for j in range(4)]}
        if i % 2:
            sps["SEMANTIC_TEXT_V0"] = [sp(base[(i * 3 + j) % 8], 10 * j, 10) for j in range(2)]
        assets.append(IsccEntry(iscc_id=make_iscc_id(i), units=units, simprints=sps))
    return assets, base


@pytest.fixture(scope="module")
def manager():
    m = hip_manager()
    m.create_index(IsccIndex(name="s"))
    assets, base = _sp_assets(200)
    m.add_assets("s", assets)
    yield m, assets, base
    m.close()


def test_search_assets_many_exact_equals_per_query_search_assets(manager):
    m, assets, base = manager
    idx = m._index("s")
    b64 = codec.encode_base64
    rng = np.random.default_rng(8)
    queries = []
    for j in range(40):
        form = j % 5
        a = assets[int(rng.integers(0, len(assets)))]
        if form == 0:
            queries.append(IsccQuery(simprints={"CONTENT_TEXT_V0": [b64(base[int(i)]) for i in rng.integers(0, 8, 3)]}))
        elif form == 1:
            queries.append(IsccQuery(units=list(a.units), simprints={"SEMANTIC_TEXT_V0": [b64(base[j % 8])], "CONTENT_TEXT_V0": [b64(base[(j + 1) % 8])]}))
        elif form == 2:
            queries.append(IsccQuery(iscc_id=a.iscc_id))                    # (its own asset is left out of the results)
        elif form == 3:
            queries.append(IsccQuery(units=list(a.units)))                  # no simprints
        else:
            queries.append(IsccQuery(units=list(a.units), simprints={"CONTENT_TEXT_V0": [b64(bytes(8))]}))
    for limit in (1, 10, 100):
        got = idx.search_assets_many(queries, limit, exact=True)
        exp = [idx.search_assets(q, limit, exact=True) for q in queries]
        assert [g.model_dump() for g in got] == [e.model_dump() for e in exp]
        assert any(r.chunk_matches for r in got)


def test_one_library_search_per_simprint_type_and_round(manager):
    m, assets, base = manager
    idx = m._index("s")
    b64 = codec.encode_base64
    queries = [IsccQuery(simprints={"CONTENT_TEXT_V0": [b64(base[i % 8]), b64(base[(i + 3) % 8])], "SEMANTIC_TEXT_V0": [b64(base[(i + 1) % 8])]})
               for i in range(64)]
    before = idx._engine.stats()["searches"]
    got = idx.search_assets_many(queries, 10, exact=True)
    assert idx._engine.stats()["searches"] - before == 2                    # two types, one round each: not 128 searches
    assert any(r.chunk_matches for r in got)
