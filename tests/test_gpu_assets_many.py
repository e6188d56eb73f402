"""
Bulk asset search on the GPU (isccsearch_match_assets, csrc/asset_score.hip): equality with per-query ``search_assets`` over
segments large enough for the matrix cores, the batch shapes around the per-call cap, the large-limit sort path, the
searches per batch, and the kernel's two summation rules against Python restatements.
"""

import numpy as np
import pytest

from helpers import hip_manager, make_iscc_id
from iscc_search_amd import _lib, codec
from iscc_search_amd.engine import pack_bytes
from iscc_search_amd.index import HipIndex
from iscc_search_amd.schema import IsccEntry, IsccIndex, IsccQuery
from test_assets_many import _flip, assert_same

pytestmark = pytest.mark.gpu

N_BIG = 70_000          # rows per unit type: above mfma_min_rows (65 536), so batches take the matrix cores


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(21)
    bases = [rng.integers(0, 256, size=16, dtype=np.uint8).tobytes() for _ in range(64)]
    assets = []
    for i in range(N_BIG):
        b = bases[i % 64]
        meta = codec.encode_unit(codec.MT_META, 0, 0, _flip(b[:8], rng, int(rng.integers(0, 4))))
        data_bits = 128 if i % 3 == 0 else 64
        data = codec.encode_unit(codec.MT_DATA, 0, 0, _flip(b[:data_bits // 8], rng, int(rng.integers(0, 4))))
        inst = codec.encode_unit(codec.MT_INSTANCE, 0, 0, b[:4] + rng.integers(0, 256, size=4, dtype=np.uint8).tobytes())
        assets.append(IsccEntry(iscc_id=make_iscc_id(i), units=[meta, data, inst]))
    m = hip_manager()
    m.create_index(IsccIndex(name="big"))
    for i in range(0, N_BIG, 10_000):
        m.add_assets("big", assets[i:i + 10_000])
    yield m, assets, rng
    m.close()


def _queries(assets, rng, n):
    out = []
    for j in range(n):
        a = assets[int(rng.integers(0, len(assets)))]
        if j % 3 == 0:
            out.append(IsccQuery(iscc_id=a.iscc_id))
        elif j % 3 == 1:
            out.append(IsccQuery(units=list(a.units[:2])))
        else:
            out.append(IsccQuery(units=[a.units[0], codec.encode_unit(codec.MT_DATA, 0, 0, _flip(codec.Iscc(a.units[1]).body, rng, 2))]))
    return out


@pytest.mark.parametrize("n", [1, 17, 1024, 1500])
def test_batches_equal_per_query_search(big, n):
    m, assets, rng = big
    queries = _queries(assets, np.random.default_rng(n), n)
    got = m.search_assets_many("big", queries, 10)
    assert_same(got, [m.search_assets("big", q, 10) for q in queries])


def test_large_limit_takes_the_global_sort_path(big):
    m, assets, _ = big
    queries = _queries(assets, np.random.default_rng(5), 3)
    got = m.search_assets_many("big", queries, 4096)
    # (2 x 4 096 records per query: more than the 2 048 items a sort array holds in LDS; ~1 000 assets pass the threshold)
    assert max(len(r.global_matches) for r in got) > 1000
    assert_same(got, [m.search_assets("big", q, 4096) for q in queries])


def test_one_search_per_unit_type_and_length(big):
    m, assets, _ = big
    idx = m._index("big")
    rng = np.random.default_rng(9)
    queries = [IsccQuery(units=[assets[int(i)].units[0], codec.encode_unit(codec.MT_DATA, 0, 0, rng.integers(0, 256, size=8, dtype=np.uint8).tobytes())])
               for i in rng.integers(0, N_BIG, size=300)]
    eng = idx._engine
    before = eng.stats()["searches"]
    idx.match_units_many(queries, 10)
    assert eng.stats()["searches"] - before == 2          # META 64-bit, DATA 64-bit: one batched search each, not 300 x 2


def _neumaier(xs):
    s, c = 0.0, 0.0
    for x in xs:
        t = s + x
        c += (s - t) + x if abs(s) >= abs(x) else (x - t) + s
        s = t
    return s + c if c else s


def test_kernel_summation_rules(hip_engine):
    """Three unit types whose scores (from the caller's tables) make the compensation term change the last bit."""
    tabs = [hip_engine.open_table(_lib.METRIC_NPHD, 1, 32) for _ in range(3)]
    q = bytes(range(1, 9))
    for t, tbl in enumerate(tabs):
        rows = [_flip(q, np.random.default_rng(t), t + 1), bytes(8 - i for i in range(8))]
        words, nb = pack_bytes(rows, tbl.max_words)
        tbl.add(np.array([77, 1000 + t], dtype=np.uint64), words, nb)
    size = (_lib.MAX_BYTES + 1) * 257
    score, pw = np.zeros(size), np.zeros(size)
    # sum(ws) = 1.0 sequentially, 1.0000000000000002 compensated; sum(ps) = 0.75 either way: totals 0.75 and 0.7499999999999999,
    # both below the cut at 1.0
    vals = {1: (1.0, 0.25), 2: (1e-16, 0.25), 3: (1e-16, 0.25)}
    for h, (s, p) in vals.items():
        score[8 * 257 + h], pw[8 * 257 + h] = s, p
    ws, ps = [vals[h][0] for h in (1, 2, 3)], [vals[h][1] for h in (1, 2, 3)]
    plain, compensated_total = sum(ps) / sum(ws), _neumaier(ps) / _neumaier(ws)
    assert plain != compensated_total and max(plain, compensated_total) < 1.0
    units = np.zeros(3, dtype=_lib.ASSET_UNIT_DTYPE)
    for t, tbl in enumerate(tabs):
        words, nb = pack_bytes([q], tbl.max_words)
        units[t]["table"], units[t]["type"], units[t]["max_hamming"], units[t]["nbytes"] = tbl.id, t, -1, 8
        units[t]["words"][: tbl.max_words] = words[0]
    for compensated, total in ((0, plain), (1, compensated_total)):
        keys, scores, counts, types, tsc, ucnt = hip_engine.match_assets(
            units, np.array([0, 3]), 4, 64, 4096, np.zeros(1), np.zeros(1), score, pw, 0.0, compensated, 3)
        assert int(counts[0]) >= 1 and int(keys[0, 0]) == 77
        assert scores[0, 0] == total
        assert types[0, 0].tolist() == [0, 1, 2] and tsc[0, 0].tolist() == ws
        assert ucnt.tolist() == [2, 2, 2]
    for tbl in tabs:
        tbl.drop()


def test_index_passes_the_interpreters_rule(big, monkeypatch):
    """HipIndex hands the engine compensated = (Python >= 3.12), as CPython's sum() decides."""
    import sys

    m, assets, _ = big
    idx = m._index("big")
    seen = []
    real = idx._engine.match_assets

    def spy(*args):
        seen.append(args[10])
        return real(*args)

    monkeypatch.setattr(idx._engine, "match_assets", spy)
    idx.match_units_many([IsccQuery(units=list(assets[0].units))], 5)
    assert seen == [sys.version_info >= (3, 12)]
    assert isinstance(idx, HipIndex)
