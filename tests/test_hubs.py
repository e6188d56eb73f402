"""
``find_hubs`` and ``max_degree`` of ``find_duplicates`` / ``find_duplicate_groups`` (CPU tier).

The engine is the oracle-backed stand-in of ``test_duplicate_groups`` whose tables get the two new joins from the host model
(``degree_model``): ``join_degrees`` and ``join_within`` with ``live_keys``.  The index holds one hub -- 40 assets with one CONTENT
unit -- two small cliques (3 assets near in META, 4 near in DATA), one member of each also near the hub's CONTENT unit, and singles.
What is checked is the definition: the degree of (asset, type) is the number of pairs ``find_duplicates`` lists with that type
confident; with ``max_degree`` a pair keeps a type only if neither asset is a hub of it, and the groups are the components of those
pairs.
"""

import numpy as np
import pytest

import degree_model as model
from helpers import flip_bits, make_iscc_id
from iscc_search_amd import codec
from iscc_search_amd.index import HipIndex, HipIndexManager, HipOptions, _unit_max_hamming
from iscc_search_amd.pairs import DuplicatePair, Hub
from iscc_search_amd.schema import IsccEntry, IsccIndex
from iscc_search_amd.unit_match import _confidence_total
from test_duplicate_groups import ComponentsOracleEngine, ComponentsOracleTable, bfs_groups
from test_duplicates import unit

N_HUB, N_A, N_B, N_SINGLE = 40, 3, 4, 10
A0, B0 = N_HUB, N_HUB + N_A                       # the clique members whose CONTENT unit is near the hub's
N_ASSETS = N_HUB + N_A + N_B + N_SINGLE
CONTENT, META, DATA = "CONTENT_TEXT_V0", "META_NONE_V0", "DATA_NONE_V0"


class HubOracleTable(ComponentsOracleTable):
    """The two joins over listed rows by the host model; every join call is noted in ``engine.calls``."""

    def join_within(self, max_hamming_by_prefix, max_pairs, live_keys=None):
        self.engine.calls.append("join_within" if live_keys is None else "join_within_live")
        if live_keys is None:
            return super().join_within(max_hamming_by_prefix, max_pairs)
        out = model.join_within_live(*self._arrays(), max_hamming_by_prefix, live_keys)
        if len(out[2]) > max_pairs:
            raise ValueError(f"{len(out[2])} pairs exceed max_pairs={max_pairs}")
        return out

    def join_degrees(self, max_hamming_by_prefix, live_keys):
        self.engine.calls.append("join_degrees")
        return model.join_degrees(*self._arrays(), max_hamming_by_prefix, live_keys)


class HubOracleEngine(ComponentsOracleEngine):
    def __init__(self):
        super().__init__()
        self.calls = []

    def open_table(self, metric, key_words, max_bytes):
        t = HubOracleTable(metric, key_words, max_bytes)
        t.engine = self
        return t


def hub_assets(seed=5):
    """The index of this file: [IsccEntry] in asset order (hub 0..39, clique A 40..42, clique B 43..46, singles)."""
    rng = np.random.default_rng(seed)
    assert int(_unit_max_hamming(HipOptions().match_threshold_units)[8]) >= 3           # the planted distances are at most 3 bits

    def rnd():
        return rng.integers(0, 256, size=8, dtype=np.uint8).tobytes()

    hub, meta_a, data_b = rnd(), rnd(), rnd()
    assets = []
    for i in range(N_ASSETS):
        meta, content, data = rnd(), rnd(), rnd()
        if i < N_HUB:
            content = hub
        elif i < B0:
            meta = flip_bits(meta_a, i - A0)
            content = flip_bits(hub, 1) if i == A0 else content
        elif i < B0 + N_B:
            data = flip_bits(data_b, i - B0)
            content = flip_bits(hub, 2) if i == B0 else content
        assets.append(IsccEntry(iscc_id=make_iscc_id(i), units=[unit(codec.MT_META, meta), unit(codec.MT_CONTENT, content), unit(codec.MT_DATA, data)]))
    return assets


def ids(numbers):
    return [make_iscc_id(i) for i in numbers]


def build(engine=None, assets=None):
    idx = HipIndex(engine or HubOracleEngine(), HipOptions())
    idx.add_assets(assets or hub_assets())
    return idx


@pytest.fixture(scope="module")
def index():
    return build()


@pytest.fixture(scope="module")
def all_pairs(index):
    return index.find_duplicates()


def degrees_of(pairs):
    """{(iscc_id, type): pairs that list the type} -- the degree by its definition"""
    out = {}
    for p in pairs:
        for t in p.types:
            for i in (p.iscc_id_a, p.iscc_id_b):
                out[(i, t)] = out.get((i, t), 0) + 1
    return out


def without_hubs(index, pairs, max_degree):
    """``pairs`` with every type dropped in which one of the two assets is a hub, rescored and reordered as find_duplicates does"""
    degree = degrees_of(pairs)
    key = codec.iscc_id_to_int
    out = []
    for p in pairs:
        types = {t: s for t, s in p.types.items() if degree[(p.iscc_id_a, t)] <= max_degree and degree[(p.iscc_id_b, t)] <= max_degree}
        if types:
            out.append(DuplicatePair(p.iscc_id_a, p.iscc_id_b, min(1.0, _confidence_total(types, index._opts.confidence_exponent)), types))
    out.sort(key=lambda p: (-p.score, key(p.iscc_id_a), key(p.iscc_id_b)))
    return out


def test_without_max_degree_the_hub_floods(index, all_pairs):
    hub_pairs = [p for p in all_pairs if CONTENT in p.types]
    assert len(hub_pairs) == (N_HUB + 2) * (N_HUB + 1) // 2 and len(all_pairs) >= 780
    assert len(all_pairs) == len(hub_pairs) + 3 + 6
    with pytest.raises(ValueError, match="exceed max_pairs=500"):
        index.find_duplicates(max_pairs=500)
    groups = index.find_duplicate_groups()
    assert [g.iscc_ids for g in groups] == [ids(range(N_HUB + N_A + N_B))]          # everything near the hub is one group


def test_max_degree_leaves_the_cliques(index, all_pairs):
    got = index.find_duplicates(max_degree=10, max_pairs=500)
    assert got == without_hubs(index, all_pairs, 10)
    clique_a, clique_b = ids(range(A0, B0)), ids(range(B0, B0 + N_B))
    assert {(p.iscc_id_a, p.iscc_id_b) for p in got} == {(a, b) for c in (clique_a, clique_b) for x, a in enumerate(c) for b in c[x + 1:]}
    assert all(set(p.types) == ({META} if p.iscc_id_a in clique_a else {DATA}) for p in got)
    groups = index.find_duplicate_groups(max_degree=10)
    assert [g.iscc_ids for g in groups] == [clique_b, clique_a] == bfs_groups(index, got)
    # a bound no degree exceeds changes nothing; 0 leaves out every row that has a partner
    assert index.find_duplicates(max_degree=N_HUB + 1) == all_pairs
    assert [g.iscc_ids for g in index.find_duplicate_groups(max_degree=N_HUB + 1)] == [ids(range(N_HUB + N_A + N_B))]
    assert index.find_duplicates(max_degree=0) == [] and index.find_duplicate_groups(max_degree=0) == []
    # the degree is taken once, in the full table: at max_degree = 2 the clique of 4 (degree 3 each) is gone though 3 of its rows
    # would have degree 2 once one is left out; the clique of 3 stays
    assert {(p.iscc_id_a, p.iscc_id_b) for p in index.find_duplicates(max_degree=2)} == {(a, b) for x, a in enumerate(clique_a) for b in clique_a[x + 1:]}
    # per table: with the CONTENT table alone the hubs leave nothing, the other tables are not touched by CONTENT's hubs
    assert index.find_duplicates(max_degree=10, unit_types=[CONTENT]) == []
    assert len(index.find_duplicates(max_degree=10, unit_types=[META, DATA])) == 9


def test_find_hubs(index, all_pairs):
    degree = degrees_of(all_pairs)
    key = codec.iscc_id_to_int
    got = index.find_hubs()
    assert all(isinstance(h, Hub) for h in got)
    assert {(h.iscc_id, h.unit_type): h.degree for h in got} == degree and len(got) == len(degree)
    assert [(-h.degree, key(h.iscc_id), h.unit_type) for h in got] == sorted((-h.degree, key(h.iscc_id), h.unit_type) for h in got)
    # the hub's members, and the two clique members near it
    hubs = index.find_hubs(min_degree=11)
    assert [h.iscc_id for h in hubs] == ids(list(range(N_HUB)) + [A0, B0]) and {(h.unit_type, h.degree) for h in hubs} == {(CONTENT, N_HUB + 1)}
    assert index.find_hubs(min_degree=N_HUB + 2) == []
    assert [(h.iscc_id, h.degree) for h in index.find_hubs(unit_types=[DATA])] == [(i, 3) for i in ids(range(B0, B0 + N_B))]
    # min_degree = 0 lists every (asset, type) the index holds
    assert len(index.find_hubs(min_degree=0)) == 3 * N_ASSETS
    # a stricter threshold: at distance 0 only the hub's own 40 rows are partners
    strict = index.find_hubs(threshold=1.0)
    assert [h.iscc_id for h in strict] == ids(range(N_HUB)) and {(h.unit_type, h.degree) for h in strict} == {(CONTENT, N_HUB - 1)}
    for bad in (0, -0.5, 1.5):
        with pytest.raises(ValueError, match="threshold"):
            index.find_hubs(threshold=bad)
    for finder in (index.find_duplicates, index.find_duplicate_groups):
        with pytest.raises(ValueError, match="max_degree"):
            finder(max_degree=-1)


def test_none_is_todays_call():
    engine = HubOracleEngine()
    idx = build(engine)
    engine.calls.clear()
    pairs = idx.find_duplicates()
    groups = idx.find_duplicate_groups()
    assert engine.calls == ["join_within"] * 3            # one plain join per unit table, no degree pass, no list
    # tables that have neither new join -- join_within takes (max_hamming, max_pairs) only -- answer the same
    plain = build(ComponentsOracleEngine())
    assert plain.find_duplicates() == pairs and plain.find_duplicate_groups() == groups
    assert plain.find_duplicates(max_degree=None) == pairs and plain.find_duplicate_groups(max_degree=None) == groups
    for call in (lambda: plain.find_duplicates(max_degree=10), lambda: plain.find_duplicate_groups(max_degree=10), plain.find_hubs):
        with pytest.raises(NotImplementedError, match="single-GPU engine"):
            call()
    engine.calls.clear()
    idx.find_duplicates(max_degree=10)
    assert engine.calls == ["join_degrees", "join_within_live"] * 3
    engine.calls.clear()
    idx.find_duplicate_groups(max_degree=10)
    idx.find_hubs()
    assert engine.calls == ["join_degrees"] * 6


def test_a_stale_row_counts_for_nothing():
    assets = hub_assets()
    idx = build(assets=assets)
    assert {h.degree for h in idx.find_hubs(unit_types=[CONTENT])} == {N_HUB + 1}
    # asset 5 again, without its CONTENT unit: its row stays in the CONTENT table
    idx.add_assets([IsccEntry(iscc_id=assets[5].iscc_id, units=[assets[5].units[0], assets[5].units[2]])])
    assert CONTENT not in idx._asset_units[codec.iscc_id_to_int(assets[5].iscc_id)]
    assert idx._unit_tables[CONTENT]._table.size == N_ASSETS
    hubs = idx.find_hubs(unit_types=[CONTENT])
    assert [h.iscc_id for h in hubs] == ids([i for i in range(N_HUB) if i != 5] + [A0, B0]) and {h.degree for h in hubs} == {N_HUB}
    # ... so at max_degree = 40 nothing is a hub any more, where the index before the update had 42 of them
    assert len(idx.find_duplicates(max_degree=N_HUB)) == len(idx.find_duplicates()) == (N_HUB + 1) * N_HUB // 2 + 9
    assert len(build(assets=assets).find_duplicates(max_degree=N_HUB)) == 9
    assert [g.size for g in idx.find_duplicate_groups(max_degree=N_HUB)] == [N_HUB - 1 + N_A + N_B]


def test_manager_and_sharded_refusal():
    m = HipIndexManager("hip:///", engine=HubOracleEngine())
    m.create_index(IsccIndex(name="hubs"))
    m.add_assets("hubs", hub_assets())
    idx = m._indexes["hubs"]
    assert m.find_hubs("hubs", min_degree=11) == idx.find_hubs(min_degree=11) != []
    assert m.find_hubs("hubs", min_degree=2, unit_types=[META], threshold=0.9) == idx.find_hubs(min_degree=2, unit_types=[META], threshold=0.9)
    assert m.find_duplicates("hubs", max_degree=10) == idx.find_duplicates(max_degree=10) != []
    assert m.find_duplicate_groups("hubs", max_degree=10) == idx.find_duplicate_groups(max_degree=10) != []
    with pytest.raises(FileNotFoundError):
        m.find_hubs("nope")
    m.close()
    sharded = HipIndexManager("hip:///?devices=2", engine=HubOracleEngine())
    for call in (lambda: sharded.find_hubs("hubs"), lambda: sharded.find_duplicates("hubs", max_degree=10),
                 lambda: sharded.find_duplicate_groups("hubs", max_degree=10)):
        with pytest.raises(NotImplementedError, match="sharded"):
            call()
