"""
Bulk asset search: ``search_assets_many`` / ``match_units_many`` answer exactly what a loop of ``search_assets`` answers.

The index is clustered on purpose: a few base codes per unit type, every asset a near-duplicate of one of them (1-3 bits
flipped), so that keys turn up in several unit lists and scores tie; INSTANCE codes share prefixes and the units mix 64- to
256-bit lengths.  Runs on CPU through the oracle-backed engine (the host aggregation the engines without the device entry point
use) and, marked gpu, through the HIP engine (isccsearch_match_assets).
"""

import numpy as np
import pytest

from helpers import hip_manager, make_iscc_id, sp
from iscc_search_amd import codec
from iscc_search_amd.index import HipIndexManager, INSTANCE_FIRST_K
from iscc_search_amd.schema import IsccEntry, IsccIndex, IsccQuery
from oracle_engine import OracleEngine


def _flip(data, rng, nbits):
    ba = bytearray(data)
    for b in rng.choice(len(ba) * 8, size=nbits, replace=False):
        ba[b // 8] ^= 1 << (7 - b % 8)
    return bytes(ba)


def clustered_assets(n, seed=7, bases=4, simprints=False):
    """n assets: META / CONTENT / DATA near-duplicates of `bases` base codes of mixed lengths, INSTANCE codes sharing prefixes."""
    rng = np.random.default_rng(seed)
    base = {
        mt: [rng.integers(0, 256, size=32, dtype=np.uint8).tobytes() for _ in range(bases)]
        for mt in (codec.MT_META, codec.MT_CONTENT, codec.MT_DATA, codec.MT_INSTANCE)
    }
    assets = []
    for i in range(n):
        b = int(rng.integers(0, bases))
        units = []
        for mt in (codec.MT_META, codec.MT_CONTENT, codec.MT_DATA):
            if mt == codec.MT_META and i % 5 == 4:
                continue                                               # not every asset carries every type
            bits = int(rng.choice([64, 128, 256])) if mt != codec.MT_META else 64
            body = _flip(base[mt][b][: bits // 8], rng, int(rng.integers(0, 4)))
            units.append(codec.encode_unit(mt, 0, 0, body))
        inst_bits = int(rng.choice([64, 128, 256]))
        inst = base[codec.MT_INSTANCE][b % 2][:8] + rng.integers(0, 256, size=24, dtype=np.uint8).tobytes()
        if i % 3 == 0:
            inst = _flip(inst, rng, 1)
        units.append(codec.encode_unit(codec.MT_INSTANCE, 0, 0, inst[: inst_bits // 8]))
        sps = None
        if simprints and i % 4 == 0:
            sps = {"CONTENT_TEXT_V0": [sp(_flip(base[codec.MT_CONTENT][b][:8], rng, int(rng.integers(0, 3))), 0, 10 + i)]}
        assets.append(IsccEntry(iscc_id=make_iscc_id(i), units=units, simprints=sps))
    return assets, base


def mixed_queries(assets, base, rng, n):
    """Every query form: iscc_code, units (two of one type, unindexed types), iscc_id, simprints."""
    out = []
    for j in range(n):
        a = assets[int(rng.integers(0, len(assets)))]
        form = j % 6
        if form == 0:
            out.append(IsccQuery(units=list(a.units)))
        elif form == 1:
            out.append(IsccQuery(iscc_id=a.iscc_id))
        elif form == 2:
            b = int(rng.integers(0, len(base[codec.MT_DATA])))
            extra = codec.encode_unit(codec.MT_DATA, 0, 0, _flip(base[codec.MT_DATA][b][:16], rng, 2))
            out.append(IsccQuery(units=list(a.units) + [extra]))             # two DATA units
        elif form == 3:
            out.append(IsccQuery(units=[codec.encode_unit(codec.MT_SEMANTIC, 0, 0, bytes(8)), a.units[-1]]))   # SEMANTIC is not indexed
        elif form == 4:
            try:
                out.append(IsccQuery(iscc_code=codec.gen_iscc_code(list(a.units))))
            except ValueError:
                out.append(IsccQuery(units=list(a.units[-2:])))
        else:
            b = int(rng.integers(0, len(base[codec.MT_CONTENT])))
            out.append(IsccQuery(units=list(a.units[:2]), simprints={"CONTENT_TEXT_V0": [codec.encode_base64(base[codec.MT_CONTENT][b][:8])]}))
    return out


def assert_same(got, exp):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert g.model_dump() == e.model_dump()
        assert [list(m.types) for m in g.global_matches] == [list(m.types) for m in e.global_matches]
        assert [m.iscc_id for m in g.global_matches] == [m.iscc_id for m in e.global_matches]


@pytest.fixture(params=["oracle", pytest.param("hip", marks=pytest.mark.gpu)])
def manager(request):
    if request.param == "oracle":
        m = HipIndexManager("hip:///", engine=OracleEngine())
    else:
        m = hip_manager()
    yield m
    m.close()


@pytest.fixture
def clustered(manager):
    assets, base = clustered_assets(400, simprints=True)
    manager.create_index(IsccIndex(name="c"))
    manager.add_assets("c", assets)
    return manager, assets, base


@pytest.mark.parametrize("limit", [1, 10, 100])
def test_many_equals_loop_of_single_searches(clustered, limit):
    m, assets, base = clustered
    queries = mixed_queries(assets, base, np.random.default_rng(limit), 48)
    got = m.search_assets_many("c", queries, limit)
    exp = [m.search_assets("c", q, limit) for q in queries]
    assert_same(got, exp)
    assert any(len(r.global_matches) >= min(limit, 2) for r in got)
    assert any(r.chunk_matches for r in got)


def test_self_exclusion_and_ties(clustered):
    m, assets, _ = clustered
    queries = [IsccQuery(iscc_id=a.iscc_id) for a in assets[:40]]
    got = m.search_assets_many("c", queries, 100)
    for q, r in zip(queries, got):
        assert q.iscc_id not in [x.iscc_id for x in r.global_matches]
    scores = [x.score for r in got for x in r.global_matches]
    assert len(scores) != len(set(scores))                                  # the clustered data has ties
    assert_same(got, [m.search_assets("c", q, 100) for q in queries])


def test_raw_form_matches_the_results(clustered):
    m, assets, base = clustered
    queries = mixed_queries(assets, base, np.random.default_rng(3), 24)
    idx = m._index("c")
    raw = idx.match_units_many(queries, 10)
    res = m.search_assets_many("c", queries, 10)
    for q, r in enumerate(res):
        c = int(raw.counts[q])
        assert c == len(r.global_matches)
        assert [codec.iscc_id_from_int(int(k), 0) for k in raw.keys[q, :c]] == [x.iscc_id for x in r.global_matches]
        assert raw.scores[q, :c].tolist() == [x.score for x in r.global_matches]
        for j, x in enumerate(r.global_matches):
            names = [raw.types[t] for t in raw.type_index[q, j].tolist() if t != 255]
            assert names == list(x.types)
            assert raw.type_scores[q, j, : len(names)].tolist() == list(x.types.values())


def test_instance_second_pass(manager):
    """More than INSTANCE_FIRST_K assets share an INSTANCE prefix: the full lists are asked again."""
    rng = np.random.default_rng(11)
    inst = rng.integers(0, 256, size=32, dtype=np.uint8).tobytes()
    n = INSTANCE_FIRST_K + 30
    manager.create_index(IsccIndex(name="i"))
    manager.add_assets("i", [IsccEntry(iscc_id=make_iscc_id(i), units=[codec.encode_unit(codec.MT_DATA, 0, 0, rng.integers(0, 256, size=8, dtype=np.uint8).tobytes()),
                                                                          codec.encode_unit(codec.MT_INSTANCE, 0, 0, inst[: 8 * (1 + i % 4)])]) for i in range(n)])
    queries = [IsccQuery(units=[codec.encode_unit(codec.MT_INSTANCE, 0, 0, inst[:8])]), IsccQuery(iscc_id=make_iscc_id(3)),
               IsccQuery(units=[codec.encode_unit(codec.MT_INSTANCE, 0, 0, inst[:16])])]
    got = manager.search_assets_many("i", queries, 200)
    assert len(got[0].global_matches) == n
    assert_same(got, [manager.search_assets("i", q, 200) for q in queries])


def test_rejections_name_the_query(clustered):
    m, assets, _ = clustered
    good = IsccQuery(iscc_id=assets[0].iscc_id)
    with pytest.raises(FileNotFoundError, match=r"queries\[1\]: Asset .* not found in index 'c'"):
        m.search_assets_many("c", [good, IsccQuery(iscc_id=make_iscc_id(99999))])
    with pytest.raises(ValueError, match=r"queries\[2\]: "):
        m.search_assets_many("c", [good, good, IsccQuery(units=["ISCC:NOTAUNIT"])])
    with pytest.raises(ValueError, match=r"queries\[0\]: Query must have"):
        m.search_assets_many("c", [IsccQuery(simprints=None, units=None, iscc_code=None)])
    with pytest.raises(FileNotFoundError):
        m.search_assets_many("missing", [good])
    assert m.search_assets_many("c", []) == []


def test_instance_cap_names_the_query(manager, monkeypatch):
    from iscc_search_amd import unit_match

    rng = np.random.default_rng(5)
    inst = rng.integers(0, 256, size=8, dtype=np.uint8).tobytes()
    manager.create_index(IsccIndex(name="cap"))
    manager.add_assets("cap", [IsccEntry(iscc_id=make_iscc_id(i), units=[codec.encode_unit(codec.MT_DATA, 0, 0, bytes(8)), codec.encode_unit(codec.MT_INSTANCE, 0, 0, inst)]) for i in range(80)])
    monkeypatch.setattr(unit_match, "_check_instance_hits", lambda count, unit_type: (_ for _ in ()).throw(ValueError(f"cap {unit_type}")) if count >= 70 else None)
    with pytest.raises(ValueError, match=r"queries\[1\]: cap INSTANCE_NONE_V0"):
        manager.search_assets_many("cap", [IsccQuery(units=[codec.encode_unit(codec.MT_DATA, 0, 0, bytes(8))]),
                                           IsccQuery(units=[codec.encode_unit(codec.MT_INSTANCE, 0, 0, inst)])])


def test_batches_beyond_one_call_are_split(clustered):
    from iscc_search_amd import _lib

    m, assets, base = clustered
    queries = [IsccQuery(units=list(assets[i % len(assets)].units)) for i in range(_lib.ASSET_QUERIES_MAX + 37)]
    got = m.search_assets_many("c", queries, 5)
    assert len(got) == len(queries)
    picks = [0, 1, _lib.ASSET_QUERIES_MAX - 1, _lib.ASSET_QUERIES_MAX, len(queries) - 1]
    assert_same([got[i] for i in picks], [m.search_assets("c", queries[i], 5) for i in picks])


def test_limit_outside_the_engine_range_behaves_as_search_assets(clustered):
    m, assets, _ = clustered
    q = [IsccQuery(units=[assets[0].units[-1]])]                            # INSTANCE only: search_assets takes any limit
    assert_same(m.search_assets_many("c", q, 5000), [m.search_assets("c", q[0], 5000)])
    with pytest.raises(ValueError, match=r"queries\[0\]: limit 5000 exceeds"):
        m.search_assets_many("c", [IsccQuery(units=list(assets[0].units))], 5000)


def test_sharded_exchange_keeps_items_of_one_block_size_on_one_table_apart():
    """(nq, k) = (3, 4) and (4, 3) on one table fill blocks of one size, which HipShardOps.buffer caches by size: no shared exchange."""
    from types import SimpleNamespace

    from iscc_search_amd.sharded import ShardedTable

    ops = SimpleNamespace()
    t = SimpleNamespace(world_size=2, ops=ops, group=None)
    items = [(t, np.zeros((3, 1), np.uint64), None, 4, None), (t, np.zeros((4, 1), np.uint64), None, 3, None)]
    assert ShardedTable.search_many(items) is None
