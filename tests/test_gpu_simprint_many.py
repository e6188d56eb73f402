"""
``isccsearch_simprint_score_many`` (many simprint requests searched and scored in one library call, requests kept apart):
``HipSimprintIndex.search_raw_many`` must return, request by request, exactly what ``search_raw`` returns for it alone --
float64 scores compared with ``==``, the order (-score, asset), every matched chunk -- and the simprint part of
``search_assets_many`` what ``search_assets`` returns per query, with one library search per (simprint type, round).
"""

import numpy as np
import pytest

from helpers import flip_bits, hip_manager, make_iscc_id, sp
from iscc_search_amd import codec
from iscc_search_amd._lib import MAX_K, MAX_SCORED_SIMPRINTS
from iscc_search_amd.schema import IsccEntry, IsccIndex, IsccQuery
from iscc_search_amd.simprint import DOC_FREQ_DUP_LIMIT, HipSimprintIndex, pack_chunk_pointer
from oracle_engine import OracleEngine
from simprint_checker import score_lists

pytestmark = pytest.mark.gpu


def _key(results):
    return [[(r.iscc_id_body, r.score, r.queried, r.matches,
              None if r.chunks is None else [(c.query, c.match, c.score, c.offset, c.size, c.freq) for c in r.chunks]) for r in res]
            for res in results]


def _corpus(rng, ndim, assets=300, per_asset=6, pool_size=40, twins=12):
    """Chunks near a pool of simprints; the last `twins` assets hold identical chunks (equal scores: ascending asset order)."""
    nbytes = ndim // 8
    pool = [rng.integers(0, 256, size=nbytes, dtype=np.uint8).tobytes() for _ in range(pool_size)]
    keys, vecs = [], []
    for a in range(assets):
        for c in range(per_asset):
            v = flip_bits(pool[int(rng.integers(0, pool_size))], int(rng.integers(0, max(2, ndim // 16))))
            keys.append(pack_chunk_pointer((a + 1).to_bytes(8, "big"), c * 10, 10 + c))
            vecs.append(np.frombuffer(v, dtype=np.uint8))
    for a in range(twins):
        for c in range(3):
            keys.append(pack_chunk_pointer((5000 + 7 * (twins - a)).to_bytes(8, "big"), c, 5))
            vecs.append(np.frombuffer(flip_bits(pool[c], 1), dtype=np.uint8))
    return pool, keys, vecs


def _mixed_requests(rng, pool, ndim):
    nbytes = ndim // 8
    near = lambda n, flips: [flip_bits(pool[int(rng.integers(0, len(pool)))], int(rng.integers(0, flips + 1))) for _ in range(n)]
    noise = [rng.integers(0, 256, size=nbytes, dtype=np.uint8).tobytes()]
    return [
        near(3, 3),
        [],
        [pool[0], flip_bits(pool[1], 1), flip_bits(pool[2], 1)],           # the twins' chunks: ties
        near(64, ndim // 32),
        noise,                                                              # matches nothing at 0.8, between two that do
        near(1, 2),
        near(700, ndim // 16),
        [pool[0]],                                                          # the same simprint as request 2, same round
        near(3, 1),
    ]


@pytest.fixture(scope="module")
def indexes(hip_engine):
    built = {}
    for ndim in (64, 128, 256):
        rng = np.random.default_rng(4000 + ndim)
        pool, keys, vecs = _corpus(rng, ndim)
        idx = HipSimprintIndex(hip_engine, ndim=ndim)
        idx.add_raw(keys, vecs)
        built[ndim] = (idx, pool, keys, vecs)
    yield built
    for idx, _, _, _ in built.values():
        idx.close()


@pytest.mark.parametrize("ndim", [64, 128, 256])
@pytest.mark.parametrize("device_doc_freq", [True, False])
@pytest.mark.parametrize("detailed", [True, False])
@pytest.mark.parametrize("threshold", [0.0, 0.8])
def test_many_equals_per_request_device_path(indexes, ndim, device_doc_freq, detailed, threshold):
    idx, pool, _, _ = indexes[ndim]
    reqs = _mixed_requests(np.random.default_rng(ndim + int(threshold * 10)), pool, ndim)
    kw = dict(limit=10, threshold=threshold, detailed=detailed, total_assets=312, device_doc_freq=device_doc_freq)
    got = idx.search_raw_many(reqs, **kw)
    exp = [idx.search_raw(r, **kw) for r in reqs]
    assert _key(got) == _key(exp)
    assert got[1] == [] and all(got[i] for i in (0, 2, 3, 6, 7))
    if threshold > 0:
        assert got[4] == []
    scores = [r.score for r in got[2]]
    assert len(scores) != len(set(scores))                                 # ties, in ascending asset order
    for a, b in zip(got[2], got[2][1:]):
        assert (-a.score, a.iscc_id_body) < (-b.score, b.iscc_id_body)


def test_many_rounds_and_a_request_too_large_for_one(indexes, hip_engine):
    idx, pool, _, _ = indexes[64]
    rng = np.random.default_rng(77)
    reqs = [[flip_bits(pool[int(i)], int(f)) for i, f in zip(rng.integers(0, len(pool), 500), rng.integers(0, 5, 500))] for _ in range(20)]
    kw = dict(limit=8, threshold=0.75, detailed=True, total_assets=312, device_doc_freq=True)
    idx.search_raw_many(reqs, **kw)                                         # (warm-up)
    before = hip_engine.stats()["searches"]
    got = idx.search_raw_many(reqs, **kw)
    assert hip_engine.stats()["searches"] - before <= 2                     # 10 000 simprints: two rounds of <= 8 192, not 20 searches
    assert _key(got) == _key([idx.search_raw(r, **kw) for r in reqs])
    huge = [flip_bits(pool[i % len(pool)], i % 7) for i in range(MAX_SCORED_SIMPRINTS + 10)]
    got = idx.search_raw_many([reqs[0], huge, reqs[1]], **kw)
    assert _key(got) == _key([idx.search_raw(r, **kw) for r in (reqs[0], huge, reqs[1])])
    # one call whose rounds mix the two pipelines, scratch and staging reused in between: 6 000 + 1 000 + 1 000 simprints are a round
    # of three requests (the many form), the 8 000 behind them a round of one (the single form) -- the smallest such shape
    mixed = [[flip_bits(pool[i % len(pool)], (i // len(pool)) % 5) for i in range(n)] for n in (6000, 1000, 1000, 8000)]
    kw = dict(kw, limit=2)
    idx.search_raw(mixed[3], **kw)                                          # (warm-up: the lazy frequency column)
    before = hip_engine.stats()["searches"]
    got = idx.search_raw_many(mixed, **kw)
    assert hip_engine.stats()["searches"] - before == 2
    assert _key(got) == _key([idx.search_raw(r, **kw) for r in mixed])


def test_radius_path_and_its_error(hip_engine):
    idx = HipSimprintIndex(hip_engine, ndim=64, oversampling_factor=20)
    base, crowded = bytes([0xAA] * 8), bytes([0x0F] * 8)
    keys = [pack_chunk_pointer((1000 + i).to_bytes(8, "big"), 0, 10) for i in range(40)]
    vecs = [np.frombuffer(flip_bits(base, i % 5), dtype=np.uint8) for i in range(40)]
    keys += [pack_chunk_pointer((9000 + i).to_bytes(8, "big"), 0, 10) for i in range(MAX_K + 10)]
    vecs += [np.frombuffer(crowded, dtype=np.uint8)] * (MAX_K + 10)
    idx.add_raw(keys, vecs)
    kw = dict(limit=1000, threshold=0.9, total_assets=40, detailed=True, device_doc_freq=True)
    got = idx.search_raw_many([[base], [], [flip_bits(base, 2), base]], **kw)
    assert _key(got) == _key([idx.search_raw(r, **kw) for r in ([base], [], [flip_bits(base, 2), base])])
    assert len(got[0]) == 40
    with pytest.raises(ValueError) as single:
        idx.search_raw([crowded], **kw)
    with pytest.raises(ValueError) as many:
        idx.search_raw_many([[base], [crowded], [base, crowded]], **kw)
    assert str(many.value) == str(single.value)
    idx.close()


def test_against_the_independent_checker(indexes):
    idx_dev, pool, keys, vecs = indexes[128]
    oracle = HipSimprintIndex(OracleEngine(), ndim=128)
    oracle.add_raw(keys, vecs)
    rng = np.random.default_rng(5)
    reqs = [[flip_bits(pool[int(i)], 3) for i in rng.integers(0, len(pool), n)] for n in (5, 1, 12)]
    limit, threshold, total = 10, 0.8, 312
    got = idx_dev.search_raw_many(reqs, limit=limit, threshold=threshold, detailed=True, total_assets=total, device_doc_freq=True)
    for simprints, res in zip(reqs, got):
        queries = np.stack([np.frombuffer(s, dtype=np.uint8) for s in simprints])
        batch = oracle._index.search(queries, count=limit * oracle.oversampling_factor)
        lists = [[(bytes(k), int(h)) for k, h in zip(batch[q].keys, batch[q].hamming)] for q in range(len(simprints))]
        freq = lambda s: int(oracle._index.doc_freq(np.frombuffer(s, dtype=np.uint8).reshape(1, -1), DOC_FREQ_DUP_LIMIT)[0])
        stored = lambda key: (lambda v: None if v is None else v.tobytes())(oracle._index.get(key))
        want = score_lists(simprints, lists, 128, limit, threshold, stored, freq, total)
        assert [(r.iscc_id_body, r.score, r.matches) for r in res] == [(w[0], w[1], w[2]) for w in want]
        for r, w in zip(res, want):
            assert [(c.query, c.match, c.score, c.offset, c.size, c.freq) for c in r.chunks] == \
                   [(simprints[qi], m, s, o, z, f) for qi, m, s, o, z, f in w[3]]


def test_a_million_chunks(hip_engine):
    """1 M random 128-bit chunks (40 per asset) + planted near-duplicates; 64 requests of 16 simprints against the per-request path."""
    rng = np.random.default_rng(99)
    idx = HipSimprintIndex(hip_engine, ndim=128)
    n = 1 << 20
    rows = np.arange(n, dtype=np.uint64)
    keys = np.stack([rows // np.uint64(40) + np.uint64(1), ((rows % np.uint64(40)) << np.uint64(32)) | np.uint64(100)], axis=1)
    vecs = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    idx._index.add(keys, vecs, trusted_unique=True)
    reqs = []
    for r in range(64):
        q = vecs[rng.integers(0, n, 16)].copy()
        q[:, 0] ^= np.uint8(3)
        reqs.append([bytes(x) for x in q])
    kw = dict(limit=20, threshold=0.75, detailed=True, total_assets=n // 40, device_doc_freq=True)
    got = idx.search_raw_many(reqs, **kw)
    assert _key(got) == _key([idx.search_raw(r, **kw) for r in reqs])
    assert all(got)
    idx.close()


def _sp_assets(n, seed=21):
    rng = np.random.default_rng(seed)
    base = [rng.integers(0, 256, size=8, dtype=np.uint8).tobytes() for _ in range(8)]
    meta_base = [rng.integers(0, 256, size=8, dtype=np.uint8).tobytes() for _ in range(3)]
    assets = []
    for i in range(n):
        units = [codec.encode_unit(codec.MT_META, 0, 0, flip_bits(meta_base[i % 3], i % 3)),
                 codec.encode_unit(codec.MT_CONTENT, 0, 0, flip_bits(meta_base[(i + 1) % 3], i % 5)),
                 codec.encode_unit(codec.MT_INSTANCE, 0, 0, rng.integers(0, 256, size=8, dtype=np.uint8).tobytes())]
        sps = {"CONTENT_TEXT_V0": [sp(flip_bits(base[(i + j) % 8], j % 3), 10 * j, 10) for j in range(4)]}
        if i % 2:
            sps["SEMANTIC_TEXT_V0"] = [sp(flip_bits(base[(i * 3 + j) % 8], 1), 10 * j, 10) for j in range(2)]
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


def test_search_assets_many_equals_per_query_search_assets(manager):
    m, assets, base = manager
    b64 = codec.encode_base64
    rng = np.random.default_rng(8)
    queries = []
    for j in range(60):
        form = j % 5
        a = assets[int(rng.integers(0, len(assets)))]
        if form == 0:
            queries.append(IsccQuery(simprints={"CONTENT_TEXT_V0": [b64(flip_bits(base[int(i)], 1)) for i in rng.integers(0, 8, 3)]}))
        elif form == 1:
            queries.append(IsccQuery(units=list(a.units[:2]), simprints={"SEMANTIC_TEXT_V0": [b64(base[j % 8])], "CONTENT_TEXT_V0": [b64(base[(j + 1) % 8])]}))
        elif form == 2:
            queries.append(IsccQuery(iscc_id=a.iscc_id))
        elif form == 3:
            queries.append(IsccQuery(units=list(a.units)))
        else:
            queries.append(IsccQuery(units=list(a.units[:2]), simprints={"CONTENT_TEXT_V0": [b64(bytes(8))]}))
    for limit in (1, 10, 100):
        got = m.search_assets_many("s", queries, limit)
        exp = [m.search_assets("s", q, limit) for q in queries]
        assert [g.model_dump() for g in got] == [e.model_dump() for e in exp]
        assert any(r.chunk_matches for r in got)


def test_one_library_search_per_simprint_type(manager):
    m, assets, base = manager
    b64 = codec.encode_base64
    queries = [IsccQuery(simprints={"CONTENT_TEXT_V0": [b64(flip_bits(base[i % 8], i % 3)), b64(base[(i + 3) % 8])]}) for i in range(64)]
    m.search_assets_many("s", queries, 10)                                  # (warm-up: frequency column, buffers)
    eng = m._index("s")._engine
    before = eng.stats()["searches"]
    got = m.search_assets_many("s", queries, 10)
    assert eng.stats()["searches"] - before <= 1                            # one type, one round: not 64 searches
    assert any(r.chunk_matches for r in got)
