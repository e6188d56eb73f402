"""
``HipSimprintIndex.search_exact_many`` and the hard-boundary simprint part of ``search_assets_many``, on CPU.

``search_exact_many`` must return, for every request, what ``search_exact`` returns for it alone.  The oracle table has no
``simprint_exact_many``, so its index runs the per-request fallback; a shim table that has one -- written in the
``isccsearch_simprint_exact_many`` output layout from ``_search_exact_host`` per request -- runs the device form's packing
(offsets, local ``given`` indices, ``queried``) and unpacking (the chunk layout at ``k * given_offsets[r]``) without a GPU.
"""

import numpy as np
import pytest

from helpers import flip_bits, make_iscc_id, sp
from iscc_search_amd import _lib, codec
from iscc_search_amd.index import HipIndexManager
from iscc_search_amd.schema import IsccEntry, IsccIndex, IsccQuery
from iscc_search_amd.simprint import EXACT_MANY_FROM, HipSimprintIndex, pack_chunk_pointer
from oracle_engine import OracleEngine


class ExactManyShim:
    """An oracle table with ``simprint_exact_many``: ``_search_exact_host`` per request, outputs in the C-ABI's layout."""

    def __init__(self, table, index):
        self._t = table
        self._index = index          # the HipSimprintIndex whose host scoring answers
        self.calls = 0
        self.seen = []

    def __getattr__(self, name):
        return getattr(self._t, name)

    def simprint_exact_many(self, q_words, distinct_offsets, given, given_offsets, queried, dup_limit, threshold, limit, detailed):
        self.calls += 1
        nbytes = self._index.ndim // 8
        q_words = np.asarray(q_words, dtype=np.uint64).reshape(-1, self.max_words)
        n_req = len(queried)
        assert len(distinct_offsets) == n_req + 1 and len(given_offsets) == n_req + 1
        assert distinct_offsets[0] == 0 and given_offsets[0] == 0
        assert distinct_offsets[-1] == q_words.shape[0] and given_offsets[-1] == len(given)
        k = min(int(dup_limit), _lib.MAX_K)
        results = np.zeros((n_req, limit), dtype=_lib.SIMPRINT_RESULT_DTYPE)
        info = np.zeros((n_req, 4), dtype=np.uint32)
        chunks = np.zeros(k * len(given), dtype=_lib.SIMPRINT_CHUNK_DTYPE) if detailed else None
        raw = q_words.astype(">u8").tobytes()
        stride = 8 * self.max_words
        for r in range(n_req):
            d0, d1, g0, g1 = int(distinct_offsets[r]), int(distinct_offsets[r + 1]), int(given_offsets[r]), int(given_offsets[r + 1])
            distinct = [raw[d * stride : d * stride + nbytes] for d in range(d0, d1)]
            local = [int(g) for g in given[g0:g1]]
            assert len(set(distinct)) == len(distinct) and all(0 <= g < d1 - d0 for g in local)
            assert int(queried[r]) >= g1 - g0 >= 1
            valid = [distinct[g] for g in local]
            # the wrong-length simprints of the request are gone: stand-ins of another length keep `queried` what it was
            as_given = valid + [b"\x00"] * (int(queried[r]) - len(valid))
            self.seen.append((valid, int(queried[r])))
            res = self._index._search_exact_host(as_given, distinct, limit, threshold, True, dup_limit)
            info[r, 0] = info[r, 1] = len(res)
            at = 0
            for j, m in enumerate(res):
                results[r, j] = (int.from_bytes(m.iscc_id_body, "big"), m.score, m.matches, at)
                if detailed:
                    for c, g in zip(m.chunks, _visiting_positions(valid, m.chunks)):
                        chunks[k * g0 + at] = ((c.offset << 32) | c.size, g, 0, c.freq, 0)
                        at += 1
            info[r, 3] = at if detailed else 0
        return results, chunks, info


def _visiting_positions(valid, chunks):
    """Position in ``valid`` of every chunk of one asset: the host lists them per given simprint in order, repeats included."""
    out, g, seen_here = [], 0, set()
    for c in chunks:
        while valid[g] != c.query or (c.offset, c.size) in seen_here:
            g += 1
            seen_here = set()
        seen_here.add((c.offset, c.size))
        out.append(g)
    return out


def _corpus(seed, ndim=64, assets=40, pool_size=10):
    rng = np.random.default_rng(seed)
    nbytes = ndim // 8
    pool = [rng.integers(0, 256, size=nbytes, dtype=np.uint8).tobytes() for _ in range(pool_size)]
    keys, vecs = [], []
    for a in range(assets):
        for c in range(5):
            # skewed: the first simprints of the pool collide often
            v = pool[min(int(rng.exponential(2.5)), pool_size - 1)]
            keys.append(pack_chunk_pointer((a + 1).to_bytes(8, "big"), c * 10, 10 + c))
            vecs.append(np.frombuffer(v, dtype=np.uint8))
    return pool, keys, vecs


def _requests(pool, seed, ndim=64):
    rng = np.random.default_rng(seed)
    absent = rng.integers(0, 256, size=ndim // 8, dtype=np.uint8).tobytes()
    return [
        [pool[0]],
        [],
        [b"\x01\x02\x03"],                                                  # only a simprint of another length
        [pool[0], pool[1], pool[0], pool[5], absent, pool[9], b"\x01\x02\x03"],   # repeats, an absent one, a wrong length counted in queried
        [absent],
        [pool[i % len(pool)] for i in range(23)],
        [pool[0]],                                                          # the same simprint in two requests
        [pool[3], pool[2]],
    ]


def _key(results):
    return [[(r.iscc_id_body, r.score, r.queried, r.matches,
              None if r.chunks is None else [(c.query, c.match, c.score, c.offset, c.size, c.freq) for c in r.chunks]) for r in res]
            for res in results]


def _index(seed, shim):
    pool, keys, vecs = _corpus(seed)
    idx = HipSimprintIndex(OracleEngine(), ndim=64)
    idx.add_raw(keys, vecs)
    if shim:
        idx._index._table = ExactManyShim(idx._index._table, idx)
    return idx, pool


@pytest.fixture(scope="module", params=["fallback", "shim"])
def index(request):
    return _index(5, request.param == "shim")


@pytest.mark.parametrize("detailed", [False, True])
@pytest.mark.parametrize("limit,threshold,dup_limit", [(10, 0.0, 1000), (3, 0.0, 4), (50, 0.2, 70), (5, 0.9, 1)])
def test_many_equals_per_request_search_exact(index, detailed, limit, threshold, dup_limit):
    idx, pool = index
    reqs = _requests(pool, 11)
    kw = dict(limit=limit, threshold=threshold, detailed=detailed, dup_limit=dup_limit)
    got = idx.search_exact_many(reqs, **kw)
    exp = [idx.search_exact(r, **kw) for r in reqs]
    assert _key(got) == _key(exp)
    assert any(got) and got[1] == [] and got[2] == [] and got[4] == []
    assert _key([got[0]]) == _key([got[6]])
    if got[3]:
        assert got[3][0].queried == 7


def test_the_oracle_table_takes_the_fallback():
    idx, pool = _index(6, False)
    assert not idx._index.scores_exact_many_on_device and not hasattr(idx._index._table, "simprint_exact_many")
    assert _key(idx.search_exact_many([[pool[0]], [pool[1]]], limit=4, detailed=True)) == \
           _key([idx.search_exact([pool[0]], limit=4, detailed=True), idx.search_exact([pool[1]], limit=4, detailed=True)])


def test_the_shim_is_called_once_per_batch_with_local_indices():
    idx, pool = _index(6, True)
    shim = idx._index._table
    assert idx._index.scores_exact_many_on_device
    reqs = _requests(pool, 3)
    got = idx.search_exact_many(reqs, limit=5, detailed=True)
    assert shim.calls == 1 and any(got)
    # the batchable requests, in order: their given simprints of valid length and what they were given in all
    batchable = [r for r in reqs if any(len(s) == 8 for s in r)]
    assert shim.seen == [([s for s in r if len(s) == 8], len(r)) for r in batchable]
    # fewer than EXACT_MANY_FROM batchable requests: the loop
    shim.calls = 0
    few = [[pool[0]], [], [b"\x01"]] + [[pool[i]] for i in range(1, EXACT_MANY_FROM - 1)]
    assert _key(idx.search_exact_many(few, limit=5)) == _key([idx.search_exact(r, limit=5) for r in few])
    assert shim.calls == 0
    assert idx.search_exact_many(few + [[pool[5]]], limit=5) and shim.calls == 1


def test_empty_index_and_empty_requests():
    idx = HipSimprintIndex(OracleEngine(), ndim=64)
    assert idx.search_exact_many([[bytes(8)], []], limit=3) == [[], []]
    assert idx.search_exact_many([], limit=3) == []
    idx, pool = _index(5, True)
    assert idx.search_exact_many([], limit=3) == []
    assert idx.search_exact_many([[], []], limit=3) == [[], []]


def test_a_request_that_raises_decides_as_in_the_loop():
    idx, pool = _index(5, True)

    class Boom(Exception):
        pass

    def broken(simprints, **kw):
        raise Boom(len(simprints))

    idx.search_exact = broken                                               # the loop's own answer, whatever it is
    with pytest.raises(Boom) as e:
        idx.search_exact_many([[pool[i]] for i in range(EXACT_MANY_FROM)] + [[], [pool[2]] * (_lib.MAX_SCORED_SIMPRINTS + 1)], limit=3)
    assert e.value.args == (0,)                                             # the first request the loop takes, in order


def _sp_assets(n, seed=21):
    rng = np.random.default_rng(seed)
    base = [rng.integers(0, 256, size=8, dtype=np.uint8).tobytes() for _ in range(6)]
    meta_base = [rng.integers(0, 256, size=8, dtype=np.uint8).tobytes() for _ in range(3)]
    assets = []
    for i in range(n):
        units = [codec.encode_unit(codec.MT_META, 0, 0, flip_bits(meta_base[i % 3], i % 3)),
                 codec.encode_unit(codec.MT_INSTANCE, 0, 0, rng.integers(0, 256, size=8, dtype=np.uint8).tobytes())]
        sps = {"CONTENT_TEXT_V0": [sp(base[(i + j) % 6], 10 * j, 10) for j in range(3)]}
        if i % 2:
            sps["SEMANTIC_TEXT_V0"] = [sp(base[(i * 3 + j) % 6], 10 * j, 10) for j in range(2)]
        assets.append(IsccEntry(iscc_id=make_iscc_id(i), units=units, simprints=sps))
    return assets, base


@pytest.mark.parametrize("shim", [False, True])
def test_search_assets_many_exact_equals_the_loop(shim):
    m = HipIndexManager("hip:///", engine=OracleEngine())
    try:
        m.create_index(IsccIndex(name="s"))
        assets, base = _sp_assets(40)
        m.add_assets("s", assets)
        idx = m._index("s")
        shims = []
        if shim:
            for table in idx._sp_tables.values():
                table._index._table = ExactManyShim(table._index._table, table)
                shims.append(table._index._table)
        b64 = codec.encode_base64
        queries = [
            IsccQuery(simprints={"CONTENT_TEXT_V0": [b64(base[0]), b64(base[1])]}),
            IsccQuery(units=list(assets[3].units), simprints={"CONTENT_TEXT_V0": [b64(base[2])], "SEMANTIC_TEXT_V0": [b64(base[3])]}),
            IsccQuery(iscc_id=assets[5].iscc_id),
            IsccQuery(units=list(assets[7].units)),
            IsccQuery(simprints={"SEMANTIC_TEXT_V0": [b64(base[4]), b64(base[5])], "CONTENT_TEXT_V0": [b64(base[4]), b64(base[4])]}),
            IsccQuery(simprints={"CONTENT_TEXT_V0": [b64(bytes(8))]}),
            IsccQuery(simprints={"SEMANTIC_TEXT_V0": [b64(base[1])]}),
            IsccQuery(simprints={"SEMANTIC_TEXT_V0": [b64(base[0]), b64(base[2]), b64(base[0])]}),
        ]
        for limit in (1, 5, 50):
            got = idx.search_assets_many(queries, limit, exact=True)
            exp = [idx.search_assets(q, limit, exact=True) for q in queries]
            assert [g.model_dump() for g in got] == [e.model_dump() for e in exp]
            assert any(r.chunk_matches for r in got)
        if shim:
            assert all(s.calls == 3 for s in shims)                         # one call per simprint type and search_assets_many
    finally:
        m.close()
