"""
``HipSimprintIndex.search_raw_many`` and the simprint part of ``search_assets_many``, on CPU.

``search_raw_many`` must return, for every request, what ``search_raw`` returns for it alone.  The oracle table has no
``simprint_score_many``, so its index runs the per-request fallback; a shim table that has one -- written in the
``isccsearch_simprint_score_many`` output layout from per-request ``simprint_score`` calls -- runs the device form's
unpacking without a GPU.
"""

import numpy as np
import pytest

from helpers import flip_bits, make_iscc_id, sp
from iscc_search_amd import _lib, codec
from iscc_search_amd.index import HipIndexManager
from iscc_search_amd.schema import IsccEntry, IsccIndex, IsccQuery
from iscc_search_amd.simprint import HipSimprintIndex, pack_chunk_pointer
from oracle_engine import OracleEngine


class ManyShim:
    """An oracle table with ``simprint_score_many``: one ``simprint_score`` per request, outputs in the C-ABI's layout."""

    def __init__(self, table):
        self._t = table
        self.calls = 0

    def __getattr__(self, name):
        return getattr(self._t, name)

    def simprint_score_many(self, q_words, offsets, count, max_hamming, threshold, limit, total_assets, dup_limit, detailed):
        self.calls += 1
        q_words = np.asarray(q_words, dtype=np.uint64).reshape(-1, self.max_words)
        offsets = np.asarray(offsets, dtype=np.uint32)
        n_req, nq = len(offsets) - 1, q_words.shape[0]
        results = np.zeros((n_req, limit), dtype=_lib.SIMPRINT_RESULT_DTYPE)
        info = np.zeros((n_req, 4), dtype=np.uint32)
        chunks = np.zeros(limit * nq, dtype=_lib.SIMPRINT_CHUNK_DTYPE) if detailed else None
        words = np.zeros((limit * nq, self.max_words), dtype=np.uint64) if detailed else None
        for r in range(n_req):
            lo, hi = int(offsets[r]), int(offsets[r + 1])
            if hi == lo:
                continue
            res, ch, wd, inf = self._t.simprint_score(q_words[lo:hi], count, max_hamming, threshold, limit, total_assets, dup_limit, detailed)
            info[r] = inf
            results[r, : len(res)] = res
            if detailed:
                at = limit * lo
                chunks[at : at + len(ch)] = ch
                words[at : at + len(ch)] = wd
        return results, chunks, words, info


def _corpus(seed, ndim=64, assets=60, per_asset=5, pool_size=12):
    rng = np.random.default_rng(seed)
    nbytes = ndim // 8
    pool = [rng.integers(0, 256, size=nbytes, dtype=np.uint8).tobytes() for _ in range(pool_size)]
    keys, vecs = [], []
    for a in range(assets):
        for c in range(per_asset):
            v = flip_bits(pool[int(rng.integers(0, pool_size))], int(rng.integers(0, 4)))
            keys.append(pack_chunk_pointer((a + 1).to_bytes(8, "big"), c * 10, 10 + c))
            vecs.append(np.frombuffer(v, dtype=np.uint8))
    return pool, keys, vecs


def _requests(pool, seed, ndim=64):
    rng = np.random.default_rng(seed)
    nbytes = ndim // 8
    miss = [rng.integers(0, 256, size=nbytes, dtype=np.uint8).tobytes()]
    return [
        [flip_bits(pool[i % len(pool)], i % 3) for i in range(5)],
        [],
        [pool[0]],
        miss,                                                               # matches nothing at a threshold
        [pool[1], pool[1], flip_bits(pool[2], 1)],                          # a repeated simprint
        [flip_bits(pool[i % len(pool)], 2) for i in range(17)],
        [pool[0]],                                                          # the same simprint in two requests
    ]


def _key(results):
    return [[(r.iscc_id_body, r.score, r.queried, r.matches,
              None if r.chunks is None else [(c.query, c.match, c.score, c.offset, c.size, c.freq) for c in r.chunks]) for r in res]
            for res in results]


@pytest.fixture(scope="module", params=["fallback", "shim"])
def index(request):
    pool, keys, vecs = _corpus(5)
    idx = HipSimprintIndex(OracleEngine(), ndim=64, oversampling_factor=4)
    idx.add_raw(keys, vecs)
    if request.param == "shim":
        idx._index._table = ManyShim(idx._index._table)
    return idx, pool


@pytest.mark.parametrize("detailed", [False, True])
@pytest.mark.parametrize("threshold", [0.0, 0.9])
@pytest.mark.parametrize("device_doc_freq", [False, True])
def test_many_equals_per_request_search_raw(index, detailed, threshold, device_doc_freq):
    idx, pool = index
    reqs = _requests(pool, 11)
    kw = dict(limit=7, threshold=threshold, detailed=detailed, total_assets=60, device_doc_freq=device_doc_freq)
    got = idx.search_raw_many(reqs, **kw)
    exp = [idx.search_raw(r, **kw) for r in reqs]
    assert _key(got) == _key(exp)
    assert any(got)
    assert got[1] == []


def test_the_shim_is_called_once_per_batch():
    pool, keys, vecs = _corpus(6)
    idx = HipSimprintIndex(OracleEngine(), ndim=64, oversampling_factor=4)
    idx.add_raw(keys, vecs)
    shim = idx._index._table = ManyShim(idx._index._table)
    assert idx._index.scores_many_on_device
    got = idx.search_raw_many(_requests(pool, 3), limit=5, detailed=True, total_assets=60)
    assert shim.calls == 1 and any(got)


def test_oracle_table_takes_the_fallback():
    idx = HipSimprintIndex(OracleEngine(), ndim=64)
    assert not idx._index.scores_many_on_device


def test_empty_index_and_empty_requests():
    idx = HipSimprintIndex(OracleEngine(), ndim=64)
    assert idx.search_raw_many([[bytes(8)], []], limit=3) == [[], []]
    assert idx.search_raw_many([], limit=3) == []


def test_rejected_request_raises_what_search_raw_raises(index):
    idx, pool = index
    bad = [pool[0][:4]]                                                     # a simprint of the wrong length
    with pytest.raises(Exception) as single:
        idx.search_raw(bad, limit=3)
    with pytest.raises(type(single.value)) as many:
        idx.search_raw_many([[pool[1]], bad], limit=3)
    assert str(many.value) == str(single.value)


def _sp_assets(n, seed=21):
    rng = np.random.default_rng(seed)
    base = [rng.integers(0, 256, size=8, dtype=np.uint8).tobytes() for _ in range(6)]
    meta_base = [rng.integers(0, 256, size=8, dtype=np.uint8).tobytes() for _ in range(3)]
    assets = []
    for i in range(n):
        units = [codec.encode_unit(codec.MT_META, 0, 0, flip_bits(meta_base[i % 3], i % 3)),
                 codec.encode_unit(codec.MT_INSTANCE, 0, 0, rng.integers(0, 256, size=8, dtype=np.uint8).tobytes())]
        sps = {"CONTENT_TEXT_V0": [sp(flip_bits(base[(i + j) % 6], j % 3), 10 * j, 10) for j in range(3)]}
        if i % 2:
            sps["SEMANTIC_TEXT_V0"] = [sp(flip_bits(base[(i * 3 + j) % 6], 1), 10 * j, 10) for j in range(2)]
        assets.append(IsccEntry(iscc_id=make_iscc_id(i), units=units, simprints=sps))
    return assets, base


@pytest.mark.parametrize("shim", [False, True])
def test_search_assets_many_with_simprints_equals_the_loop(shim):
    m = HipIndexManager("hip:///", engine=OracleEngine())
    try:
        m.create_index(IsccIndex(name="s"))
        assets, base = _sp_assets(40)
        m.add_assets("s", assets)
        if shim:
            for table in m._index("s")._sp_tables.values():
                table._index._table = ManyShim(table._index._table)
        b64 = codec.encode_base64
        queries = [
            IsccQuery(simprints={"CONTENT_TEXT_V0": [b64(base[0]), b64(flip_bits(base[1], 1))]}),
            IsccQuery(units=list(assets[3].units), simprints={"CONTENT_TEXT_V0": [b64(base[2])], "SEMANTIC_TEXT_V0": [b64(base[3])]}),
            IsccQuery(iscc_id=assets[5].iscc_id),
            IsccQuery(units=list(assets[7].units)),
            IsccQuery(simprints={"SEMANTIC_TEXT_V0": [b64(base[4]), b64(base[5])], "CONTENT_TEXT_V0": [b64(base[4])]}),
            IsccQuery(simprints={"CONTENT_TEXT_V0": [b64(bytes(8))]}),
        ]
        for limit in (1, 5, 50):
            got = m.search_assets_many("s", queries, limit)
            exp = [m.search_assets("s", q, limit) for q in queries]
            assert [g.model_dump() for g in got] == [e.model_dump() for e in exp]
            assert any(r.chunk_matches for r in got)
    finally:
        m.close()
