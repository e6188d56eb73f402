"""
``find_duplicate_groups``: the connected components of an index's near-duplicate pairs (CPU tier).

The engine is the oracle-backed stand-in of ``test_duplicates`` with a numpy ``join_components`` built on the host model
(``components_model``).  What is checked is the definition: the groups are the components, found by a plain BFS, of the graph whose
edges are the pairs ``find_duplicates`` lists -- for all unit types, for a subset, and at another threshold against a second index
built with that threshold -- and their order, ``min_size``, stale rows of an update and the refusals.
"""

import numpy as np
import pytest

import components_model as model
from helpers import flip_bits, make_iscc_id
from iscc_search_amd import codec
from iscc_search_amd.index import HipIndex, HipIndexManager, HipOptions, _unit_max_hamming
from iscc_search_amd.pairs import DuplicateGroup
from iscc_search_amd.schema import IsccEntry, IsccIndex
from test_duplicates import JoinOracleEngine, JoinOracleTable, build_assets, unit


class ComponentsOracleTable(JoinOracleTable):
    def join_components(self, max_hamming_by_prefix, live_keys, live_labels, parent):
        keys, words, nb = self._arrays()
        out, links = model.join_components(keys, words, nb, max_hamming_by_prefix, live_keys, live_labels, parent)
        parent[:] = out
        return links


class ComponentsOracleEngine(JoinOracleEngine):
    def open_table(self, metric, key_words, max_bytes):
        t = ComponentsOracleTable(metric, key_words, max_bytes)
        t.engine = self
        return t


def bfs_groups(index, pairs, min_size=2):
    """The components of the assets of ``index`` under ``pairs``, as lists of iscc_ids in the order find_duplicate_groups promises."""
    key = codec.iscc_id_to_int
    ids = [e.iscc_id for _, e in sorted(index._assets.items())]
    near = {i: set() for i in ids}
    for p in pairs:
        near[p.iscc_id_a].add(p.iscc_id_b)
        near[p.iscc_id_b].add(p.iscc_id_a)
    seen, groups = set(), []
    for start in ids:
        if start in seen:
            continue
        seen.add(start)
        queue, members = [start], []
        while queue:
            v = queue.pop(0)
            members.append(v)
            for w in near[v] - seen:
                seen.add(w)
                queue.append(w)
        if len(members) >= min_size:
            groups.append(sorted(members, key=key))
    groups.sort(key=lambda g: (-len(g), key(g[0])))
    return groups


def build_index(options=None, n=220, seed=7):
    idx = HipIndex(ComponentsOracleEngine(), options or HipOptions())
    idx.add_assets(build_assets(np.random.default_rng(seed), n))
    return idx


@pytest.fixture(scope="module")
def index():
    return build_index()


def test_groups_are_the_components_of_find_duplicates(index):
    got = index.find_duplicate_groups()
    exp = bfs_groups(index, index.find_duplicates())
    assert all(isinstance(g, DuplicateGroup) and g.size == len(g.iscc_ids) for g in got)
    assert [g.iscc_ids for g in got] == exp
    assert len(exp) > 5 and len(exp[0]) > 2            # several groups, one of more than a pair


def test_unit_types_restrict_the_edges(index):
    for types in (["DATA_NONE_V0"], ["META_NONE_V0", "INSTANCE_NONE_V0"]):
        got = index.find_duplicate_groups(unit_types=types)
        assert got and [g.iscc_ids for g in got] == bfs_groups(index, index.find_duplicates(unit_types=types))
    assert [g.iscc_ids for g in index.find_duplicate_groups(unit_types=["DATA_NONE_V0"])] != [g.iscc_ids for g in index.find_duplicate_groups()]


def test_threshold_is_that_of_an_index_built_with_it(index):
    strict = build_index(HipOptions(match_threshold_units=0.9))
    exp = bfs_groups(strict, strict.find_duplicates())
    assert exp and [g.iscc_ids for g in index.find_duplicate_groups(threshold=0.9)] == exp
    assert [g.iscc_ids for g in strict.find_duplicate_groups()] == exp
    assert exp != [g.iscc_ids for g in index.find_duplicate_groups()]


def test_order_and_min_size(index):
    key = codec.iscc_id_to_int
    groups = index.find_duplicate_groups(min_size=1)
    assert sum(g.size for g in groups) == len(index)            # every asset is in exactly one group
    assert len({i for g in groups for i in g.iscc_ids}) == len(index)
    assert [(-g.size, key(g.iscc_ids[0])) for g in groups] == sorted((-g.size, key(g.iscc_ids[0])) for g in groups)
    assert all(g.iscc_ids == sorted(g.iscc_ids, key=key) for g in groups)
    assert [g.iscc_ids for g in groups] == bfs_groups(index, index.find_duplicates(), min_size=1)
    for m in (2, 3, 4):
        assert index.find_duplicate_groups(min_size=m) == [g for g in groups if g.size >= m]
    assert index.find_duplicate_groups(min_size=10_000) == []


def test_an_update_that_dropped_a_unit_bridges_nothing():
    rng = np.random.default_rng(11)
    thr = HipOptions().match_threshold_units
    m = int(_unit_max_hamming(thr)[8])
    assert 1 <= m and 2 * m <= 64
    base = rng.integers(0, 256, size=8, dtype=np.uint8).tobytes()

    def asset(i, meta):
        units = [unit(codec.MT_CONTENT, rng.integers(0, 256, size=8, dtype=np.uint8).tobytes()),
                 unit(codec.MT_DATA, rng.integers(0, 256, size=8, dtype=np.uint8).tobytes())]
        return IsccEntry(iscc_id=make_iscc_id(i), units=([unit(codec.MT_META, meta)] if meta is not None else []) + units)

    # META: A ~ S ~ B at m bits each, A and B 2 m bits apart; nothing else is near
    idx = HipIndex(ComponentsOracleEngine(), HipOptions())
    idx.add_assets([asset(0, base), asset(1, flip_bits(base, m)), asset(2, flip_bits(base, 2 * m))])
    ids = [make_iscc_id(i) for i in range(3)]
    assert [g.iscc_ids for g in idx.find_duplicate_groups()] == [ids]
    idx.add_assets([asset(1, None)])                   # S again, without its META unit: its row stays in the META table
    assert idx._unit_tables["META_NONE_V0"]._table.size == 3
    assert idx.find_duplicates() == [] and idx.find_duplicate_groups() == []
    assert [g.iscc_ids for g in idx.find_duplicate_groups(min_size=1)] == [[i] for i in ids]


def test_refusals(index):
    for bad in (0, 0.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="threshold"):
            index.find_duplicate_groups(threshold=bad)
    assert index.find_duplicate_groups(threshold=1.0) is not None
    # tables with join_within only, as a sharded engine's tables have neither
    plain = HipIndex(JoinOracleEngine(), HipOptions())
    plain.add_assets(build_assets(np.random.default_rng(2), 10))
    with pytest.raises(NotImplementedError, match="find_duplicate_groups"):
        plain.find_duplicate_groups()


def test_manager_find_duplicate_groups_and_sharded_refusal():
    m = HipIndexManager("hip:///", engine=ComponentsOracleEngine())
    m.create_index(IsccIndex(name="dups"))
    m.add_assets("dups", build_assets(np.random.default_rng(3), 40))
    got = m.find_duplicate_groups("dups")
    assert got and got == m._indexes["dups"].find_duplicate_groups()
    assert m.find_duplicate_groups("dups", unit_types=["DATA_NONE_V0"], threshold=0.9, min_size=1) == \
        m._indexes["dups"].find_duplicate_groups(unit_types=["DATA_NONE_V0"], threshold=0.9, min_size=1)
    with pytest.raises(FileNotFoundError):
        m.find_duplicate_groups("nope")
    m.close()
    sharded = HipIndexManager("hip:///?devices=2", engine=ComponentsOracleEngine())
    with pytest.raises(NotImplementedError, match="sharded"):
        sharded.find_duplicate_groups("dups")
