"""
Mixed-length NPHD search where the code lengths INTERLEAVE and TIE (tests/nphd_cases.py), against that file's exact host model.

The random-data NPHD tests (test_gpu_parity.py, test_gpu_many.py) fill their lists from the shortest compared prefix alone.  Here:

  (a) the sweep table -- one row per (byte length p, distance h), tie classes spanning all 32 lengths, k cutting inside them -- through
      every search path: one-launch segments, the XOR + popcount scan with levels, the matrix-core kernels (packed one-word prefixes,
      2-4 words, partial last words) as the single pass and as levels, and with speculation off;
  (b) ``dist_rank`` of every record against ``model_rank``: each of the 4 256 entries of the 33 x 257 rank table;
  (c) the same tables through ``search_within`` and ``search_many``;
  (d) the ratio speculation held to ``MHintModel``: hit, hit exactly at ratio + 1/32 (in the 256-, 64- and 192-bit segment), miss one
      bit further out, the per-segment radius in segments whose bits / 32 is fractional (24 and 104 bits), the decay of the hint;
  (e) the shape of test_gpu_many.py's mixed-length test on the clustered table, whose lists hold four and more lengths per query.

Every comparison is exact: keys, hamming, prefix_bits and count.
"""

import functools

import numpy as np
import pytest

import nphd_cases as nc
from test_gpu_device_lists import _search as search_device_records

pytestmark = pytest.mark.gpu

METRIC_NPHD = 1
NAMES = ("keys", "hamming", "prefix_bits", "count")
MATRIX = dict(tiny_rows=0, mfma=1, mfma_pack=1, mfma_min_rows=1, mfma_min_queries=1)
OPTION_SETS = {
    "one_launch": {},                                   # the defaults: every segment is small enough for tiny_search_kernel
    "valu_levels": dict(tiny_rows=0),
    "matrix_single": dict(MATRIX, self_tighten=1),
    "matrix_levels": dict(MATRIX, self_tighten=0),
    "no_speculation": dict(speculate=0),
}
COUNTERS = ("scan_launches", "mfma_launches", "mfma_pack_launches")


def _same(got, exp, what):
    for g, e, name in zip(got, exp, NAMES):
        np.testing.assert_array_equal(g, e, err_msg=f"{what}: {name}")


def _open(engine, data):
    t = engine.open_table(METRIC_NPHD, 2 if np.asarray(data.keys).ndim == 2 else 1, 32)
    t.add(data.keys, data.words, data.lens)
    return t


@pytest.fixture(scope="module")
def sweep_tables(hip_engine):
    tables = {kw: _open(hip_engine, nc.sweep_table(kw)) for kw in (1, 2)}
    yield tables
    for t in tables.values():
        t.drop()


@pytest.fixture(scope="module")
def clustered_tables(hip_engine):
    tables = {kw: _open(hip_engine, nc.clustered_table(kw)) for kw in (1, 2)}
    yield tables
    for t in tables.values():
        t.drop()


@functools.lru_cache(maxsize=None)
def _sweep_batches(key_words):
    """The queries of (a): the nine of every kind in one call, 160 of 32 bytes and 160 of 13 bytes (a partial last word)."""
    Q = nc.sweep_table(key_words).Q
    return (("mixed 9",) + nc.sweep_queries(Q), ("160 x 32 bytes",) + nc.sweep_queries_many(Q, 160, 32), ("160 x 13 bytes",) + nc.sweep_queries_many(Q, 160, 13))


@functools.lru_cache(maxsize=None)
def _sweep_expected(key_words, k, radius=None):
    sw = nc.sweep_table(key_words)
    return tuple(nc.model_topk(sw.keys, sw.words, sw.lens, q, ql, k, radius) for _, q, ql in _sweep_batches(key_words))


# ---------------------------------------------------------------------------------------------------------------------
# (a) the sweep table through every path
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_words", [1, 2])
@pytest.mark.parametrize("k", [1, 10, 544, 2144])
@pytest.mark.parametrize("path", list(OPTION_SETS))
def test_sweep_table_through_every_path(hip_engine, sweep_tables, path, k, key_words):
    t = sweep_tables[key_words]
    assert len(t.segments()) == 32 and t.size == nc.SWEEP_ROWS
    with hip_engine.options(**OPTION_SETS[path]):
        for (label, q, ql), exp in zip(_sweep_batches(key_words), _sweep_expected(key_words, k)):
            before = hip_engine.stats()
            got = t.search(q, ql, k)
            after = hip_engine.stats()
            _same(got, exp, f"{path} k={k} {label}")
            d = {c: after[c] - before[c] for c in COUNTERS}
            if path.startswith("matrix"):
                # every scan on the matrix cores; the prefixes of one word (1..8 bytes) on the packed kernel
                assert d["mfma_launches"] >= 32 and d["mfma_pack_launches"] >= 8, d
            else:
                assert d["mfma_launches"] == 0 and d["scan_launches"] >= 32, d
            if path == "no_speculation":
                assert (after["spec_hits"], after["spec_misses"]) == (before["spec_hits"], before["spec_misses"])


# ---------------------------------------------------------------------------------------------------------------------
# (b) the rank table, entry by entry
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["one_launch", "valu_levels", "matrix_single"])
def test_every_entry_of_the_rank_table(hip_engine, sweep_tables, path):
    """Q reaches h = 0..4p of every length p, ~Q reaches 8p - h: at k = 2 144 both lists hold every row, and together every (p, h)."""
    sw = nc.sweep_table(1)
    q = nc.to_words(np.array([sw.Q, ~sw.Q], dtype=np.uint8))
    ql = np.full(2, 32, dtype=np.uint8)
    exp = nc.model_topk(sw.keys, sw.words, sw.lens, q, ql, nc.SWEEP_ROWS)
    with hip_engine.options(**OPTION_SETS[path]):
        rec, cnt = search_device_records(sweep_tables[1], q, ql, nc.SWEEP_ROWS)
    assert cnt.tolist() == [nc.SWEEP_ROWS, nc.SWEEP_ROWS]
    np.testing.assert_array_equal(rec["key_lo"], exp[0])
    np.testing.assert_array_equal(rec["hamming"], exp[1])
    np.testing.assert_array_equal(rec["prefix_bits"], exp[2])
    assert not rec["key_hi"].any()
    seen = set()
    for r in rec.reshape(-1):
        p, h = int(r["prefix_bits"]) // 8, int(r["hamming"])
        assert int(r["dist_rank"]) == nc.model_rank(p, h), f"dist_rank {int(r['dist_rank'])} of {h} / (8 x {p})"
        seen.add((p, h))
    assert seen == {(p, h) for p in range(1, 33) for h in range(8 * p + 1)}


# ---------------------------------------------------------------------------------------------------------------------
# (c) search_within and search_many
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _within_case(name, key_words):
    if name == "sweep":
        data = nc.sweep_table(key_words)
        q, ql = nc.sweep_queries(data.Q)
        q2, ql2 = nc.sweep_queries_many(data.Q, 20, 13)
        return data, np.concatenate([q, q2]), np.concatenate([ql, ql2])
    data = nc.clustered_table(key_words)
    return (data,) + nc.clustered_queries(data, 48)


@pytest.mark.parametrize("path", ["one_launch", "valu_levels", "matrix_single"])
@pytest.mark.parametrize("name,key_words", [("sweep", 1), ("sweep", 2), ("clustered", 1), ("clustered", 2)])
def test_within_and_many_equal_the_model(hip_engine, sweep_tables, clustered_tables, name, key_words, path):
    data, q, ql = _within_case(name, key_words)
    t = (sweep_tables if name == "sweep" else clustered_tables)[key_words]
    k = 300
    with hip_engine.options(**OPTION_SETS[path]):
        for radius in (0, 3, 20, 256):                  # 256: every row is within it
            exp = nc.model_topk(data.keys, data.words, data.lens, q, ql, k, radius)
            if radius == 256:
                assert (exp[3] == k).all()
            elif radius <= 3:
                assert exp[3].min() < k, "some list must end at the radius, not at k"
            _same(t.search_within(q, ql, k, radius), exp, f"{name} {path} within {radius}")
        got = hip_engine.search_many([(t, q, ql, 10, None), (t, q, ql, k, 3), (t, q[ql == 32], ql[ql == 32], 100, None)])
        _same(got[0], nc.model_topk(data.keys, data.words, data.lens, q, ql, 10), f"{name} {path} many: top-10")
        _same(got[1], nc.model_topk(data.keys, data.words, data.lens, q, ql, k, 3), f"{name} {path} many: within 3")
        _same(got[2], nc.model_topk(data.keys, data.words, data.lens, q[ql == 32], 32, 100), f"{name} {path} many: top-100")


# ---------------------------------------------------------------------------------------------------------------------
# (d) the ratio speculation against MHintModel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qlen", [32, 13])
@pytest.mark.parametrize("m,options", [(1, {}), (5, {}), (160, {}), (160, dict(mfma=1, mfma_pack=1, mfma_min_rows=1, mfma_min_queries=1))],
                         ids=["1", "5", "160", "160-matrix"])
def test_ratio_speculation_follows_the_hint_model(hip_engine, qlen, m, options):
    """
    tests/nphd_cases.py::SCENARIO_STEPS, batch by batch: the answer equals the model whatever the verdict, and the verdict --
    (spec_hits, spec_misses) of the batch -- is the one the documented rule gives.  Batches of 1 and 5 list each segment's rows
    within floor((ratio + 1/32) x bits + 1e-9); batches of 160 (above spec_max_queries) start each segment's pass under that value
    ("160-matrix": the single pass on the matrix cores, which really starts there) and are verified alike.
    """
    sc = nc.hint_scenario(qlen)
    model = nc.MHintModel(sc.keys, sc.words, sc.lens)
    assert m <= hip_engine.get_option("spec_max_queries") or m == 160
    t = _open(hip_engine, sc)                           # a table of its own: its hints start empty
    try:
        with hip_engine.options(tiny_rows=0, **options):
            for i, (label, _, k, verdict) in enumerate(sc.steps):
                q = nc.scenario_batch(sc, i, m)
                ql = np.full(m, qlen, dtype=np.uint8)
                exp = nc.model_topk(sc.keys, sc.words, sc.lens, q, ql, k)
                hint = model.hint(m, qlen).ratio
                ruled = model.step(q, qlen, k)
                assert ruled == verdict, f"step {i} ({label}): the scenario is not what it claims"
                before = hip_engine.stats()
                got = t.search(q, ql, k)
                after = hip_engine.stats()
                _same(got, exp, f"step {i} ({label})")
                delta = (after["spec_hits"] - before["spec_hits"], after["spec_misses"] - before["spec_misses"])
                assert delta == verdict, f"step {i} ({label}): hint {hint}, worst k-th {max(nc.kth_ratios(exp, k))}: (hits, misses) {delta}, the rule gives {verdict}"
    finally:
        t.drop()


# ---------------------------------------------------------------------------------------------------------------------
# (e) the existing mixed-length shape, on lists that interleave
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_words", [1, 2])
def test_clustered_lists_hold_four_lengths_per_query(hip_engine, clustered_tables, key_words):
    """256-bit queries at k = 10 under the default options, twice (the second batch speculates): every list of the DEVICE holds
    at least 4 distinct prefix lengths -- what lists over uniformly random codes never do."""
    data = nc.clustered_table(key_words)
    t = clustered_tables[key_words]
    assert t.segments() == {b: 2500 for b in nc.CLUSTER_LENGTHS}
    for nq in (5, 100, 200):
        q, ql = nc.clustered_queries(data, nq, seed=40 + nq, lengths=(32,))
        exp = nc.model_topk(data.keys, data.words, data.lens, q, ql, 10)
        for again in range(2):
            got = t.search(q, ql, 10)
            _same(got, exp, f"{nq} queries, pass {again}")
            assert min(len(set(row.tolist())) for row in got[2]) >= 4
            assert (got[2] >= 128).mean() >= 0.25
