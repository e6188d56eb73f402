"""
The host model of ``match_assets`` (``tests/asset_score_model.py``) checked without a GPU: behind an oracle-backed index it must
give what the per-unit reference (``tests/unit_match_reference.py``) and the host path (``unit_match.match_host``) give, and a few
hand-computed lists pin its tie order, its clamp and its two summation rules.
"""

import numpy as np
import pytest

import asset_score_model as model
import unit_match_reference as reference
from helpers import flip_bits, make_iscc_id
from iscc_search_amd import codec, unit_match
from iscc_search_amd.index import HipIndexManager, INSTANCE_FIRST_K
from iscc_search_amd.schema import IsccEntry, IsccIndex, IsccQuery
from oracle_engine import OracleEngine

SHARED = 70          # assets sharing one INSTANCE prefix


class ModelEngine(OracleEngine):
    """``OracleEngine`` whose ``match_assets`` is the model over the rows its tables hold."""

    def __init__(self):
        self.tables = {}
        self.calls = 0

    def open_table(self, metric, key_words, max_bytes):
        t = super().open_table(metric, key_words, max_bytes)
        t.id = len(self.tables) + 1
        self.tables[t.id] = t
        return t

    def match_assets(self, units, offsets, *rest):
        self.calls += 1
        tables = {}
        for tid in np.unique(units["table"]).tolist():
            tables[tid] = model.ModelTable()
            tables[tid].add(*self.tables[tid]._arrays())
        return model.match_assets(tables, units, offsets, *rest)


def _unit(mtype, body):
    return codec.encode_unit(mtype, 0, 0, body)


@pytest.fixture(scope="module")
def clustered():
    """120 near-duplicate assets as ``test_unit_match.clustered``: META codes of 8, 16 and 32 bytes, ``SHARED`` under one INSTANCE prefix."""
    assert SHARED > INSTANCE_FIRST_K
    rng = np.random.default_rng(23)
    base = {mt: rng.integers(0, 256, size=32, dtype=np.uint8).tobytes() for mt in (codec.MT_META, codec.MT_CONTENT, codec.MT_DATA, codec.MT_INSTANCE)}
    assets = []
    for i in range(120):
        inst = base[codec.MT_INSTANCE][:8] if i < SHARED else rng.integers(0, 256, size=8, dtype=np.uint8).tobytes()
        inst += rng.integers(0, 256, size=(0, 8, 24)[i % 3], dtype=np.uint8).tobytes()
        assets.append(IsccEntry(iscc_id=make_iscc_id(i), units=[
            _unit(codec.MT_META, flip_bits(base[codec.MT_META][: (8, 16, 32)[i % 3]], i % 5)),
            _unit(codec.MT_CONTENT, flip_bits(base[codec.MT_CONTENT][: (16, 8)[i % 2]], i % 4)),
            _unit(codec.MT_DATA, flip_bits(base[codec.MT_DATA][:8], i % 7) if i % 4 else rng.integers(0, 256, size=8, dtype=np.uint8).tobytes()),
            _unit(codec.MT_INSTANCE, inst),
        ]))
    engine = ModelEngine()
    m = HipIndexManager("hip:///", engine=engine)
    m.create_index(IsccIndex(name="t"))
    m.add_assets("t", assets)
    queries = [
        IsccQuery(units=list(assets[7].units)),
        IsccQuery(iscc_id=assets[9].iscc_id),                                              # self-exclusion, > INSTANCE_FIRST_K identity hits
        IsccQuery(units=[assets[0].units[0], assets[2].units[0], assets[1].units[2]]),    # two META units: 8 and 32 bytes
        IsccQuery(units=[assets[3].units[3]]),                                             # INSTANCE only
        IsccQuery(iscc_code=codec.gen_iscc_code(list(assets[100].units))),
        IsccQuery(units=[_unit(codec.MT_SEMANTIC, bytes(8)), assets[80].units[1]]),       # SEMANTIC is not indexed
    ]
    yield m._index("t"), queries, engine
    m.close()


@pytest.mark.parametrize("limit", [1, 5, 100])
def test_model_equals_the_per_unit_reference_and_the_host_path(clustered, limit):
    idx, queries, engine = clustered
    assert {len(codec.Iscc(a.units[0]).body) for a in idx._assets.values()} == {8, 16, 32}
    before = engine.calls
    got = idx.match_units_many(queries, limit)
    assert engine.calls == before + 1                                      # the model answered, not the host path
    host = unit_match.match_host(engine, idx._unit_tables, idx._opts, idx._prepare_many(queries), limit)
    for q, query in enumerate(queries):
        c = int(got.counts[q])
        listed = []
        for r in range(c):
            types = {got.types[t]: s for t, s in zip(got.type_index[q, r].tolist(), got.type_scores[q, r].tolist()) if t != 255}
            listed.append((int(got.keys[q, r]), float(got.scores[q, r]), types))
            assert not got.type_scores[q, r][got.type_index[q, r] == 255].any()
        assert not got.keys[q, c:].any() and not got.scores[q, c:].any() and (got.type_index[q, c:] == 255).all()
        expected = reference.global_matches(idx, query, limit)
        assert [(codec.iscc_id_from_int(k, idx._realm_id or 0), s, t) for k, s, t in listed] == expected
        assert [list(t) for _, _, t in listed] == [list(t) for _, _, t in expected]
        assert listed == [(k, min(1.0, total), t) for k, total, t in host[q]]
        assert [list(t) for _, _, t in listed] == [list(t) for _, _, t in host[q]]
    if limit == 100:
        assert int(got.counts[3]) == SHARED                                # through the second, full-length INSTANCE lists
        assert int(got.counts[1]) >= SHARED - 1 and codec.iscc_id_to_int(queries[1].iscc_id) not in got.keys[1].tolist()
        assert any((got.type_index[0, r] != 255).sum() > 1 for r in range(int(got.counts[0])))


def _tables(entries):
    """Score and power tables with the given {table index: (score, power)}, zero elsewhere."""
    score, pw = [0.0] * (33 * 257), [0.0] * (33 * 257)
    for i, (s, p) in entries.items():
        score[i], pw[i] = s, p
    return score, pw


def test_ties_keep_their_first_appearance_and_the_limit_cuts_through_them():
    score, pw = _tables({1: (0.5, 0.25), 2: (1.0, 1.0), 3: (0.25, 0.125)})
    # unit 0 (type 0) lists 5, 3; unit 1 (type 1) lists 9, 7, 3: totals 5 -> 0.5, 3 -> (0.25 + 0.125) / 0.75 = 0.5, 9 -> 0.5, 7 -> 1.0
    lists = [([5, 3], [1, 1]), ([9, 7, 3], [1, 2, 3])]
    ranked = model.score_lists(lists, [0, 1], None, score, pw, 0.0, False, 10)
    assert ranked == [(7, 1.0, {1: 1.0}), (5, 0.5, {0: 0.5}), (3, 0.5, {0: 0.5, 1: 0.25}), (9, 0.5, {1: 0.5})]
    assert [k for k, _, _ in model.score_lists(lists, [0, 1], None, score, pw, 0.0, False, 2)] == [7, 5]
    assert [k for k, _, _ in model.score_lists(lists, [0, 1], 5, score, pw, 0.0, False, 2)] == [7, 3]
    # at threshold 0.5 asset 3 loses its second type from the total, not from its listed types
    assert model.score_lists(lists, [0, 1], None, score, pw, 0.5, False, 10)[2] == (3, 0.5, {0: 0.5, 1: 0.25})
    # the max per (key, type) keeps the type's first place: one type listing 3 twice, the better score second
    assert model.score_lists([([3], [3]), ([3], [1])], [0, 0], None, score, pw, 0.0, False, 10) == [(3, 0.5, {0: 0.5})]


def test_totals_above_one_order_unclamped_and_report_one():
    score, pw = _tables({1: (0.5, 0.625), 2: (0.5, 0.75), 3: (1.0, 1.0)})
    lists = [([4, 6, 8], [3, 1, 2])]                                     # totals 1.0, 1.25, 1.5
    ranked = model.score_lists(lists, [0], None, score, pw, 0.0, False, 10)
    assert [(k, t) for k, t, _ in ranked] == [(8, 1.5), (6, 1.25), (4, 1.0)]
    units = np.zeros(1, dtype=model.UNIT_DTYPE)
    keys, scores, counts, types, tsc, ucnt = model.match_assets({}, units, [0, 1], 4, 64, 4096, [0], [0], score, pw, 0.0, False, 2, lists=lists)
    assert keys.tolist() == [[8, 6, 4, 0]] and scores.tolist() == [[1.0, 1.0, 1.0, 0.0]] and counts.tolist() == [3]
    assert types.tolist() == [[[0, 255], [0, 255], [0, 255], [255, 255]]] and tsc[0, :, 0].tolist() == [0.5, 0.5, 1.0, 0.0]
    assert ucnt.tolist() == [3]


def test_both_summation_rules_by_hand():
    xs = [1.0, 1e-16, 1e-16]
    assert model.float_sum(xs, False) == 1.0                             # each 1e-16 is lost to rounding
    assert model.float_sum(xs, True) == 1.0000000000000002               # the compensation term carries them: 2e-16 rounds up one ulp
    assert model.float_sum([], True) == 0.0 and model.float_sum([0.25] * 4, True) == 1.0
    score, pw = _tables({1: (1.0, 0.25), 2: (1e-16, 0.25), 3: (1e-16, 0.25)})
    lists = [([77], [1]), ([77], [2]), ([77], [3])]
    plain = model.score_lists(lists, [0, 1, 2], None, score, pw, 0.0, False, 1)[0][1]
    compensated = model.score_lists(lists, [0, 1, 2], None, score, pw, 0.0, True, 1)[0][1]
    assert plain == 0.75 and compensated == 0.75 / 1.0000000000000002 and compensated == 0.7499999999999999


def test_a_zero_weight_group_scores_zero():
    score, pw = _tables({1: (0.0, 1.0)})
    assert model.score_lists([([9], [1])], [0], None, score, pw, 0.0, False, 1) == [(9, 0.0, {0: 0.0})]
    assert unit_match._rank_aggregated({9: {"a": 0.0}}, 0.0, 2, None, 1) == [(9, 0.0, {"a": 0.0})]


def test_brute_force_lists_order_by_exact_distance_then_key():
    t = model.ModelTable()
    codes = np.zeros((5, 32), dtype=np.uint8)
    codes[1, 0] = 0x80                  # 1 bit of 64 away
    codes[2, 0] = 0x80                  # 1 bit of 128
    codes[3, 0], codes[3, 9] = 0xC0, 1  # 3 bits of 128; the bit in byte 9 lies past an 8-byte prefix, which leaves 2 of 64
    words = codes.view(">u8").astype(np.uint64).reshape(5, 4)
    t.add([50, 40, 30, 20, 10], words, [8, 8, 16, 16, 16])
    q = np.zeros((1, 32), dtype=np.uint8)
    # 8-byte query: every prefix is 8 bytes -- (0, 10), (0, 50), (1/64, 30), (1/64, 40), (2/64, 20)
    assert t.lists(q, 8, 5, False) == [([10, 50, 30, 40, 20], [8 * 257, 8 * 257, 8 * 257 + 1, 8 * 257 + 1, 8 * 257 + 2])]
    # 16-byte query: 1/128 < 1/64 = 2/128 < 3/128
    assert t.lists(q, 16, 4, False) == [([10, 50, 30, 40], [16 * 257, 8 * 257, 16 * 257 + 1, 8 * 257 + 1])]
    assert t.lists(q, 16, 9, True) == [([10, 50], [16 * 257, 8 * 257])]
    assert t.lists(q, 16, 1, True) == [([10], [16 * 257])]
