"""
Every path that answers an OVERFLOWED candidate list, against the oracle, at small shapes.

A list that outgrows the per-query buffer (``Batch::reserve``) is flagged by the select and answered again: by the retry with levels,
by ``Batch::fix_query`` (full histogram, key radix over the table, private buffer, second select) or -- device-resident lists -- by
the ``COUNT_OVERFLOW`` marker.  Nothing repairs a wrong answer of these paths afterwards.  Option ``candidate_cap`` shrinks the buffer
to 64 entries, so tables of 5 003 rows reach all of them; tests/overflow_cases.py plants the classes that force each overflow and
tests/test_overflow_cases.py proves, on the CPU, that they do.

  (a) the four scan paths x every code form (1 - 4 words, masked 13-byte codes, 64- and 128-bit keys, NPHD segments)
  (b) a list of exactly ``cap`` rows against one of ``cap + 1``
  (c) the fallback's key radix through key bytes 0 .. 5 (64-bit keys) and 0 .. 13 (128-bit keys, cut in the low word)
  (d) the select's own key radix without any overflow
  (e) NPHD tables with one and with two overflowing segments
  (f) ``search_many``, ``search_device`` and the asynchronous search + ``merge_device``
  (g) ``doc_freq`` / ``doc_freq_counted`` / ``get_freq``
  (h) the three simprint scoring calls over overflowing lists

Every expected value comes from the oracle (``oracle_topk`` / ``np_within``), an ``OracleEngine``-backed twin index or the plain-loop
checker fed by that twin; every comparison is ``==`` on integers or float64 values.  Counters are asserted only in a session without
``ISCC_HIP_OPTS``.
"""

import os

import numpy as np
import pytest

import overflow_cases as oc
from iscc_search_amd import _lib
from iscc_search_amd.simprint import DOC_FREQ_DUP_LIMIT, HipSimprintIndex
from oracle import np_within
from oracle_engine import OracleEngine
from simprint_checker import score_lists
from test_gpu_thresholds import PATHS

pytestmark = pytest.mark.gpu

COUNTERS = not os.environ.get("ISCC_HIP_OPTS")
BASE = dict(candidate_cap=oc.CANDIDATE_CAP, tiny_rows=0, speculate=0)
NAMES = ("keys", "hamming", "prefix_bits", "count")
TWO_PATHS = ["xor8", "mfma_single"]


def _same(got, exp, what):
    for g, e, name in zip(got, exp, NAMES):
        np.testing.assert_array_equal(g, e, err_msg=f"{what}: {name}")


def _counted(engine, call):
    before = engine.stats()
    got = call()
    after = engine.stats()
    return got, {name: after[name] - before[name] for name in after}


class World:
    """The device tables of the cases, opened once each, and the oracle's answers, computed once each."""

    def __init__(self, engine):
        self.engine, self.tables, self.expected = engine, {}, {}

    def table(self, name):
        if name not in self.tables:
            c = oc.case(name)
            t = self.engine.open_table(c.metric, c.key_words, c.max_bytes)
            self.tables[name] = t
            t.add(c.keys, c.words, c.lens)
            assert t.size == c.n
        return self.tables[name]

    def expect(self, name, tag, b, k, radius=None):
        key = (name, tag, k, radius)
        if key not in self.expected:
            self.expected[key] = oc.expect(oc.case(name), b, k, radius)
        return self.expected[key]

    def close(self):
        for t in self.tables.values():
            t.drop()
        self.tables.clear()


@pytest.fixture(scope="module")
def world(hip_engine):
    w = World(hip_engine)
    try:
        yield w
    finally:
        w.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) the scan paths
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,k,zero", oc.SCAN_BATCHES, ids=[f"q{q}-k{k}{'-zero' if z else ''}" for q, k, z in oc.SCAN_BATCHES])
@pytest.mark.parametrize("form", list(oc.SCAN_FORMS))
@pytest.mark.parametrize("path", list(PATHS))
def test_every_scan_path_answers_its_overflowed_lists_exactly(world, path, form, nq, k, zero):
    """
    Hot queries at the first and last position and at both sides of every query-group edge, each with one row more than the buffer
    holds or several times as many; quiet random queries between them.  cap = max(64, 16 k) = 64 | 160 with levels and
    max(cap, 64 k) = 256 | 640 in the single pass, for k = 4 | 10.
    """
    engine, name = world.engine, f"scan_{form}"
    cap = oc.cap_of(oc.CANDIDATE_CAP, k, oc.SINGLE_PASS[path])
    b = oc.scan_batch(name, nq, cap, zero)
    t = world.table(name)
    with engine.options(**BASE, **PATHS[path]):
        got, delta = _counted(engine, lambda: t.search(b.q, b.qn, k))
    _same(got, world.expect(name, ("scan", nq, cap, zero), b, k), f"{path} {form} nq={nq} k={k}")
    if COUNTERS:
        assert delta["fallback_queries"] == len(b.hot_at), "every hot query takes the exact fallback, no quiet one does"
        assert delta["self_retries"] == (1 if path == "mfma_single" else 0), "an overflowed single pass is retried once per batch"
        assert (delta["mfma_launches"] > 0) == (not path.startswith("xor"))
        if not path.startswith("xor") and form in ("b8k1", "b8k2"):
            assert (delta["mfma_pack_launches"] > 0) == (not zero), "an all-zero query keeps 64-bit codes on the unpacked kernel"


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) cap against cap + 1
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
def test_a_list_of_exactly_cap_rows_fits_and_one_more_row_overflows(world, path):
    """
    ``search_within(radius = 9)`` over classes of exactly 64, 65, 1 040 and 1 041 rows within the radius (hot queries 0 .. 3).
    k = 4 under candidate_cap = 64: cap = max(64, 16 x 4) = 64.  The buffer is never smaller than 16 k, so no k reaches cap + 1
    itself; the second pair takes the first k that spans the whole 65-row class, k = 65, under candidate_cap = 1 040 = 16 x 65, so
    that 16 k does not move cap: cap = 1 040.  The quiet neighbours have no row within the radius: count 0, every slot zero.
    (``fix_query``'s own ``need == 0`` branch is not reached here or by any other call of the library: a list flagged under a plain
    radius holds more than cap > 0 rows within it, the ratio form and top-k searches count every row as within, and k = 0 is refused
    at the entry points.  The branch stays untested.)
    """
    engine, c = world.engine, oc.case("boundary")
    t = world.table("boundary")
    whole = oc.mixed_batch("boundary", 7)
    assert whole.hot_at == {0: 0, 2: 1, 4: 2, 6: 3}
    for candidate_cap, k, fits, over in ((oc.CANDIDATE_CAP, oc.BOUNDARY_K, 0, 1), (oc.BOUNDARY_WIDE_CAP, oc.BOUNDARY_WIDE_K, 2, 3)):
        cap = oc.cap_of(candidate_cap, k, False)
        with engine.options(**dict(BASE, candidate_cap=candidate_cap), **PATHS[path]):
            for h, flagged in ((fits, 0), (over, 1)):
                q = c.hot[h : h + 1]
                got, delta = _counted(engine, lambda: t.search_within(q, None, k, 9))
                _same(got, oc.expect_within(c.keys, c.words, None, c.metric, c.max_bytes, q, None, k, 9), f"{path} k={k} hot {h}")
                assert int(got[3][0]) == k
                if COUNTERS:
                    assert delta["fallback_queries"] == flagged, f"{c.size_of(h)} rows within the radius, cap {cap}"
            got, delta = _counted(engine, lambda: t.search_within(whole.q, None, k, 9))
        _same(got, world.expect("boundary", "whole", whole, k, 9), f"{path} k={k} whole batch")
        for i in whole.quiet():
            assert got[3][i] == 0 and not got[0][i].any() and not got[1][i].any() and not got[2][i].any()
        if COUNTERS:
            assert delta["fallback_queries"] == sum(c.size_of(h) > cap for h in range(4))


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) the key radix of fix_query
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10, 700])
@pytest.mark.parametrize("path", TWO_PATHS)
@pytest.mark.parametrize("name", list(oc.RADIX_TABLES))
def test_fallback_key_radix_walks_past_the_first_key_bytes(world, name, path, k):
    """
    70 001 rows, all at distance 9 of the hot query: the fallback cannot collect them (floor 65 536) and pins the k smallest keys down
    byte by byte -- 0xFF five times, then the cut (64-bit keys); the asset's eight bytes, 0xFF five times, then the cut in the LOW
    word (128-bit keys).  k = 700: the second select's own radix then runs over the 65 536 collected rows to the last key byte.
    """
    engine = world.engine
    b = oc.mixed_batch(name, 3)
    t = world.table(name)
    with engine.options(**BASE, **PATHS[path]):
        got, delta = _counted(engine, lambda: t.search(b.q, None, k))
    _same(got, world.expect(name, "radix", b, k), f"{name} {path} k={k}")
    if COUNTERS:
        assert delta["fallback_queries"] >= 1


@pytest.mark.parametrize("path", TWO_PATHS)
@pytest.mark.parametrize("name", list(oc.RADIX_TABLES))
def test_fallback_key_radix_of_a_range_limited_search(world, name, path):
    engine = world.engine
    b = oc.mixed_batch(name, 3)
    t = world.table(name)
    with engine.options(**BASE, **PATHS[path]):
        got, delta = _counted(engine, lambda: t.search_within(b.q, None, 4096, 9))
    _same(got, world.expect(name, "radix", b, 4096, 9), f"{name} {path} within 9")
    assert int(got[3][0]) == 4096
    if COUNTERS:
        assert delta["fallback_queries"] >= 1


# ---------------------------------------------------------------------------------------------------------------------------------
# (d) the select's radix, no overflow
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide_from", [1024, 1 << 30])
@pytest.mark.parametrize("k", [10, 257, 1500])
@pytest.mark.parametrize("tiny", ["tiny", "scan"])
@pytest.mark.parametrize("name", list(oc.SELECT_TABLES))
def test_select_radix_over_keys_with_high_bytes_without_an_overflow(world, name, tiny, k, wide_from):
    """
    Default candidate buffer; 3 003 rows within the k-th distance of the hot query exceed the sort buffer of k = 10 (1 024 slots) and
    k = 257 (2 048), so the select pins the cut down by key bytes first -- over keys whose top bytes are 0xFF, 0x80, 0x7F, 0x00.
    ``tiny``: the one-launch search (option tiny_rows at its default) runs the same select.
    """
    engine = world.engine
    b = oc.mixed_batch(name, 3)
    t = world.table(name)
    opts = dict(speculate=0, select_wide_from=wide_from)
    if tiny == "scan":
        opts["tiny_rows"] = 0
    with engine.options(**opts):
        got, delta = _counted(engine, lambda: t.search(b.q, None, k))
    _same(got, world.expect(name, "select", b, k), f"{name} {tiny} k={k} wide_from={wide_from}")
    if COUNTERS:
        assert delta["fallback_queries"] == 0 and delta["self_retries"] == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# (e) several segments
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [3, 9])
@pytest.mark.parametrize("path", TWO_PATHS)
@pytest.mark.parametrize("name,segs", [("nphd_one", 1), ("nphd_two", 2)])
def test_nphd_segments_that_overflow_are_fixed_before_the_merge(world, name, segs, path, nq):
    """
    Hot queries of 8, 16 and 32 bytes, each with 300 rows within its k-th distance in the 16-byte segment (and, second table, in the
    32-byte segment too): cap = 64 with levels and 256 in the single pass (k = 4), 160 for the range-limited search (k = 10).
    """
    engine = world.engine
    b = oc.mixed_batch(name, nq)
    t = world.table(name)
    with engine.options(**BASE, **PATHS[path]):
        got, delta = _counted(engine, lambda: t.search(b.q, b.qn, 4))
        got_w, delta_w = _counted(engine, lambda: t.search_within(b.q, b.qn, 10, 9))
    _same(got, world.expect(name, ("mixed", nq), b, 4), f"{name} {path} nq={nq} top-4")
    _same(got_w, world.expect(name, ("mixed", nq), b, 10, 9), f"{name} {path} nq={nq} within 9")
    if COUNTERS:
        assert delta["fallback_queries"] == 3 * segs and delta_w["fallback_queries"] == 3 * segs


# ---------------------------------------------------------------------------------------------------------------------------------
# (f) the callers
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", TWO_PATHS)
def test_search_many_reruns_its_overflowed_requests_in_either_order(world, path):
    engine = world.engine
    single = oc.SINGLE_PASS[path]
    big, small, third = "scan_b16k2", "healthy", "scan_b8k1"
    b1 = oc.scan_batch(big, 9, oc.cap_of(oc.CANDIDATE_CAP, 4, single))
    b2 = oc.scan_batch(big, 3, oc.cap_of(oc.CANDIDATE_CAP, 10, False))
    b4 = oc.scan_batch(third, 8, oc.cap_of(oc.CANDIDATE_CAP, 10, single))
    healthy = oc.case(small)
    q3 = healthy.words[:4].copy()
    plan = [
        (big, b1.q, 4, None, world.expect(big, ("scan", 9, oc.cap_of(oc.CANDIDATE_CAP, 4, single), False), b1, 4)),            # overflows
        (big, b2.q, 10, 9, world.expect(big, ("scan", 3, 160, False), b2, 10, 9)),                                              # range-limited, overflows
        (small, q3, 7, None, oc.expect_topk(healthy.keys, healthy.words, None, healthy.metric, 8, q3, None, 7)),                # healthy
        (third, b4.q, 10, None, world.expect(third, ("scan", 8, oc.cap_of(oc.CANDIDATE_CAP, 10, single), False), b4, 10)),      # overflows, another table
    ]
    hot = len(b1.hot_at) + len(b2.hot_at) + len(b4.hot_at)
    for order in (plan, plan[::-1]):
        with engine.options(**BASE, **PATHS[path]):
            got, delta = _counted(engine, lambda: engine.search_many([(world.table(n), q, None, k, r) for n, q, k, r, _ in order]))
        for i, ((n, _, k, r, exp), g) in enumerate(zip(order, got)):
            _same(g, exp, f"{path} request {i} ({n}, k={k}, radius={r})")
        if COUNTERS:
            assert delta["fallback_queries"] >= hot


@pytest.mark.parametrize("path", TWO_PATHS)
def test_search_device_fixes_its_lists_inside_the_call(world, path):
    """The synchronous device search: ``finish()`` without ``queue_results``; the records are read back from the caller's block."""
    from test_gpu_device_lists import _assert_records, _search

    engine, name = world.engine, "scan_b16k2"
    single = oc.SINGLE_PASS[path]
    b = oc.scan_batch(name, 9, oc.cap_of(oc.CANDIDATE_CAP, 4, single))
    bw = oc.scan_batch(name, 3, 160)
    t = world.table(name)
    with engine.options(**BASE, **PATHS[path]):
        (rec, cnt), delta = _counted(engine, lambda: _search(t, b.q, None, 4))
        (rec_w, cnt_w), delta_w = _counted(engine, lambda: _search(t, bw.q, None, 10, r=9))
    _assert_records(rec, cnt, world.expect(name, ("scan", 9, oc.cap_of(oc.CANDIDATE_CAP, 4, single), False), b, 4), 2, f"{path} top-4:")
    _assert_records(rec_w, cnt_w, world.expect(name, ("scan", 3, 160, False), bw, 10, 9), 2, f"{path} within 9:")
    if COUNTERS:
        assert delta["fallback_queries"] == len(b.hot_at) and delta_w["fallback_queries"] >= len(bw.hot_at)


@pytest.mark.parametrize("path", TWO_PATHS)
def test_asynchronous_search_marks_overflow_and_the_marker_survives_the_merge(world, path):
    """
    Two half-tables (alternate rows, 16-byte codes, 128-bit keys), each searched asynchronously into its part of one device block,
    then ``merge_device`` behind the stream: a query whose list overflows in either half carries ``COUNT_OVERFLOW``, every other one
    -- hot queries whose halves fit among them -- equals the oracle over all rows.
    """
    import torch

    from iscc_search_amd.sharded import block_bytes

    engine, c, k = world.engine, oc.case("scan_b16k2"), 4
    cap = oc.cap_of(oc.CANDIDATE_CAP, k, oc.SINGLE_PASS[path])
    b = oc.mixed_batch("scan_b16k2", 9)
    must = {p for p, h in b.hot_at.items() if h in oc.async_flagged(c, k, cap)}
    assert must and len(must) < len(b.hot_at)
    exp = world.expect("scan_b16k2", ("mixed", 9), b, k)
    rec_bytes, blk = block_bytes(b.nq, k)
    buf = torch.zeros(2 * blk, dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    tables = []
    try:
        for keys, words in oc.halves(c):
            tables.append(engine.open_table(c.metric, c.key_words, c.max_bytes))
            tables[-1].add(keys, words)
        with engine.options(**BASE, **PATHS[path]):
            for i, t in enumerate(tables):
                t.search_device(b.q, None, k, buf.data_ptr() + i * blk, buf.data_ptr() + i * blk + rec_bytes, consumer_stream=stream)
            merged = engine.merge_device(2, b.nq, k, 2, buf.data_ptr(), buf.data_ptr() + rec_bytes, blk, blk, after_stream=stream)
    finally:
        for t in tables:
            t.drop()
    marked = {i for i in range(b.nq) if merged[3][i] == _lib.COUNT_OVERFLOW}
    assert must <= marked <= set(b.hot_at), "a list that outgrows the buffer in one half is marked; no quiet query is"
    if COUNTERS:
        assert marked == must
    for i in range(b.nq):
        if i in marked:
            assert not merged[0][i].any() and not merged[1][i].any()
        else:
            for g, e, name in zip(merged, exp, NAMES):
                np.testing.assert_array_equal(g[i], e[i], err_msg=f"{path} query {i}: {name}")


# ---------------------------------------------------------------------------------------------------------------------------------
# (g) document frequency
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", TWO_PATHS)
@pytest.mark.parametrize("name", list(oc.DOCFREQ_TABLES))
def test_document_frequency_of_a_code_with_more_collisions_than_the_buffer(world, name, path):
    """
    The collision scan asks for dup_limit rows within radius 0: cap = max(64, 16 x dup_limit) = 400 | 16 000 against 450 | 17 000 equal
    rows.  Expected: distinct first key words among the first dup_limit equal rows by ascending key; ``distinct_kernel`` is queued
    again behind the fix.
    """
    engine, c, dup_limit = world.engine, oc.case(name), oc.DOCFREQ_LIMIT[name]
    b = oc.mixed_batch(name, 3)
    q = b.q.copy()
    stored = int(np.setdiff1d(np.arange(c.n), c.class_of(0)["tie_rows"])[5])
    q[1] = c.words[stored]                                       # a stored code outside the class: one row, one asset
    want = [oc.doc_freq_of(c, q[i], dup_limit) for i in range(3)]
    assert want[0][1] == dup_limit and want[1] == (1, 1) and want[2] == (0, 0)
    t = world.table(name)
    with engine.options(**BASE, **PATHS[path]):
        freq, delta = _counted(engine, lambda: t.doc_freq(q, None, dup_limit))
        (freq_c, coll), delta_c = _counted(engine, lambda: t.doc_freq_counted(q, None, dup_limit))
        row = int(c.class_of(0)["tie_rows"][7])
        col = t.get_freq(c.keys[[row, stored]], dup_limit)
    assert freq.tolist() == [w[0] for w in want] and freq_c.tolist() == freq.tolist()
    assert coll.tolist() == [w[1] for w in want]
    assert col.tolist() == [want[0][0], 1]
    if COUNTERS:
        assert delta["fallback_queries"] == 1 and delta_c["fallback_queries"] == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# (h) simprint scoring over overflowing lists
# ---------------------------------------------------------------------------------------------------------------------------------
SP_LIMIT, SP_THRESHOLD, SP_OVERSAMPLING = oc.SIMPRINT_LIMIT, oc.SIMPRINT_THRESHOLD, oc.SIMPRINT_OVERSAMPLING
# count = 20 x 2 = 40: cap = max(64, 16 x 40) = 640, max(640, 64 x 40) = 2 560 in the single pass
assert DOC_FREQ_DUP_LIMIT == oc.SIMPRINT_DUP_LIMIT


class SimprintWorld:
    """
    A device index and its ``OracleEngine`` twin over one corpus of tests/overflow_cases.py (``SimprintCorpus``: ``hot`` simprints
    stored in thousands of chunks, ``pool`` the ordinary ones; tests/test_overflow_cases.py counts its rows).  Expected answers come
    from the twin: its neighbour lists and stored vectors, ``np_within`` over its rows for the document frequencies, ``score_lists``
    for the scores; ``search_exact`` of the twin for the hard-boundary search.
    """

    def __init__(self, engine, kind):
        self.corpus = c = oc.simprint_corpus(kind)
        self.ndim, self.nb, self.hot, self.pool, self.total_assets = c.ndim, c.nb, c.hot, c.pool, c.total_assets
        self.rows = len(c.keys)
        self.index = HipSimprintIndex(engine, ndim=c.ndim, oversampling_factor=SP_OVERSAMPLING)
        self.twin = HipSimprintIndex(OracleEngine(), ndim=c.ndim, oversampling_factor=SP_OVERSAMPLING)
        vecs = list(c.vecs)
        self.index.add_raw(c.keys, vecs)
        self.twin.add_raw(c.keys, vecs)
        assert self.index.size == self.twin.size == self.rows
        self.t_keys, self.t_words, _ = self.twin._index._table._arrays()
        self.cache = {}

    def equal_rows(self, simprint):
        q = np.frombuffer(simprint.ljust(8 * self.t_words.shape[1], b"\0"), dtype=">u8").astype(np.uint64)
        return int((self.t_words == q).all(axis=1).sum())

    def _freq(self, simprint):
        q = np.frombuffer(simprint.ljust(8 * self.t_words.shape[1], b"\0"), dtype=">u8").astype(np.uint64)
        kk, _, _ = np_within(self.t_words, self.nb, self.t_keys, q, self.nb, DOC_FREQ_DUP_LIMIT, 0)
        return len(np.unique(kk[:, 0]))

    def want(self, simprints, device_doc_freq):
        """(asset, score, matches, chunks) per result by the checker, and the longest neighbour list."""
        key = (tuple(simprints), device_doc_freq)
        if key not in self.cache:
            count = SP_LIMIT * SP_OVERSAMPLING
            batch = self.twin._index.search(np.stack([np.frombuffer(s, dtype=np.uint8) for s in simprints]), count=count)
            lists = [[(bytes(k), int(h)) for k, h in zip(batch[q].keys, batch[q].hamming)] for q in range(len(simprints))]
            stored = lambda k: (lambda v: None if v is None else v.tobytes())(self.twin._index.get(k))
            scored = score_lists(simprints, lists, self.ndim, SP_LIMIT, SP_THRESHOLD, stored, self._freq if device_doc_freq else None, self.total_assets)
            self.cache[key] = (scored, max(len(l) for l in lists))
        return self.cache[key]

    def want_exact(self, given, limit, dup_limit):
        key = ("exact", tuple(given), limit, dup_limit)
        if key not in self.cache:
            self.cache[key] = self.twin.search_exact(given, limit=limit, threshold=0.0, detailed=True, dup_limit=dup_limit)
        return self.cache[key]

    def close(self):
        self.index.close()


def _assert_scored(got, want, simprints, detailed, what):
    assert [r.iscc_id_body for r in got] == [w[0] for w in want], f"{what}: assets and their order"
    for r, (asset, score, matches, chunks) in zip(got, want):
        assert r.score == score, (what, asset.hex(), r.score, score)
        assert r.matches == matches and r.queried == len(simprints)
        if detailed:
            assert [(c.query, c.match, c.score, c.offset, c.size, c.freq) for c in r.chunks] == \
                   [(simprints[qi], match, sim, offset, size, f) for qi, match, sim, offset, size, f in chunks], (what, asset.hex())
        else:
            assert r.chunks is None


@pytest.fixture(scope="module")
def simprint_worlds(hip_engine):
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = SimprintWorld(hip_engine, kind)
        return made[kind]

    try:
        yield get
    finally:
        for w in made.values():
            w.close()


@pytest.mark.parametrize("detailed", [True, False], ids=["detailed", "plain"])
@pytest.mark.parametrize("device_doc_freq", [True, False], ids=["devfreq", "freq1"])
@pytest.mark.parametrize("path", TWO_PATHS)
@pytest.mark.parametrize("ndim", [64, 128, 256])
def test_simprint_requests_with_hot_simprints_equal_the_checker(simprint_worlds, ndim, path, device_doc_freq, detailed):
    """
    ``search_raw`` (isccsearch_simprint_score) with the hot simprints first, last and in the middle of 30 ordinary ones, and
    ``search_raw_many`` (_score_many) with hot and ordinary requests in one round.  Both hot lists outgrow the buffer -- 2 700 rows
    tie at distance 0, 30 + 2 970 lie within distance 5, against 640 | 2 560 -- so the batch is marked and compacted a second time
    behind the fix, from the same entry base.  The first hot simprint's whole list is at distance 0 and count = 40 < dup_limit: its
    own document frequency comes from the collision scan (the ``unknown`` path).
    """
    w = simprint_worlds(ndim)
    engine = w.index._index._table.engine
    assert w.equal_rows(w.hot[0]) == 2700 > oc.cap_of(oc.CANDIDATE_CAP, 40, True) and w.equal_rows(w.hot[1]) == 30
    requests = w.corpus.raw_requests()
    kw = dict(limit=SP_LIMIT, threshold=SP_THRESHOLD, detailed=detailed, total_assets=w.total_assets, device_doc_freq=device_doc_freq)
    with engine.options(**BASE, **PATHS[path]):
        singles = []
        for i, simprints in enumerate(requests):
            got, delta = _counted(engine, lambda: w.index.search_raw(simprints, **kw))
            want, longest = w.want(simprints, device_doc_freq)
            assert len(want) == SP_LIMIT
            _assert_scored(got, want, simprints, detailed, f"{path} request {i}")
            singles.append(got)
            if COUNTERS:
                assert delta["fallback_queries"] >= 2, "both hot lists take the exact fallback"
        queries = np.stack([np.frombuffer(s, dtype=np.uint8) for s in requests[0]])
        info = w.index._index.score_assets(queries, SP_LIMIT * SP_OVERSAMPLING, None, SP_THRESHOLD, SP_LIMIT, w.total_assets,
                                           DOC_FREQ_DUP_LIMIT if device_doc_freq else 0, detailed)[3]
        assert info[0] == SP_LIMIT and info[2] == w.want(requests[0], device_doc_freq)[1] == SP_LIMIT * SP_OVERSAMPLING
        many = w.corpus.many_requests()
        got_many, delta = _counted(engine, lambda: w.index.search_raw_many(many, **kw))
        each = [w.index.search_raw(r, **kw) for r in many]
    assert got_many == each, "one round of many requests equals the requests asked one by one"
    for i, (r, got) in enumerate(zip(many, got_many)):
        _assert_scored(got, w.want(r, device_doc_freq)[0], r, detailed, f"{path} many, request {i}")
    if COUNTERS:
        assert delta["fallback_queries"] >= 3


@pytest.mark.parametrize("dup_limit", [25, 1000])
@pytest.mark.parametrize("path", TWO_PATHS)
@pytest.mark.parametrize("ndim", [64, 128, 256])
def test_hard_boundary_search_over_overflowing_collision_lists_equals_the_twin(simprint_worlds, ndim, path, dup_limit):
    """
    ``_search_exact_device`` (isccsearch_simprint_exact) against ``search_exact`` of the oracle-backed twin: hot simprints repeated
    among the simprints given, once with every lookup in one batch (hits and offsets are prepared behind the select -- and again
    behind the fix) and once with 1 102 distinct lookups (two batches; prepared after the search).  dup_limit = 25: cap = 400 against
    2 700 equal rows; dup_limit = 1 000: cap = 16 000 holds every list of this corpus, the select's own radix cuts the 2 700 rows.
    """
    w = simprint_worlds(ndim)
    engine = w.index._index._table.engine
    for what in ("one batch", "two batches"):
        given = w.corpus.exact_given(what)
        distinct = list(dict.fromkeys(given))
        assert (len(distinct) > 1024) == (what == "two batches")
        want = w.want_exact(given, 30, dup_limit)
        assert len(want) == 30
        with engine.options(**BASE, **PATHS[path]):
            got, delta = _counted(engine, lambda: w.index._search_exact_device(given, distinct, 30, 0.0, True, dup_limit))
            plain = w.index._search_exact_device(given, distinct, 30, 0.0, False, dup_limit)
        assert got == want, f"{path} {what} dup_limit={dup_limit}"
        assert [(r.iscc_id_body, r.score, r.matches, r.queried) for r in plain] == [(r.iscc_id_body, r.score, r.matches, r.queried) for r in want]
        assert all(r.chunks is None for r in plain)
        if COUNTERS:
            assert delta["fallback_queries"] == (1 if oc.cap_of(oc.CANDIDATE_CAP, dup_limit, False) < 2700 else 0)


@pytest.mark.parametrize("detailed", [True, False], ids=["detailed", "plain"])
@pytest.mark.parametrize("path", TWO_PATHS)
def test_a_simprint_whose_own_collision_scan_overflows(simprint_worlds, path, detailed):
    """
    17 003 chunks hold one simprint.  Its neighbour list (count = 40) lies wholly at distance 0, so its document frequency is asked of
    the collision scan -- whose list of dup_limit = 1 000 rows overflows its buffer of 16 000 in turn.  The hard-boundary search of the
    same simprint at dup_limit = 1 000 overflows alike.
    """
    w = simprint_worlds("big")
    engine = w.index._index._table.engine
    (hot,) = w.hot
    assert w.equal_rows(hot) == 17_003 > oc.cap_of(oc.CANDIDATE_CAP, DOC_FREQ_DUP_LIMIT, False)
    (simprints,) = w.corpus.raw_requests()
    with engine.options(**BASE, **PATHS[path]):
        got, delta = _counted(engine, lambda: w.index.search_raw(simprints, limit=SP_LIMIT, threshold=SP_THRESHOLD, detailed=detailed,
                                                                 total_assets=w.total_assets, device_doc_freq=True))
        given = w.corpus.exact_given("one batch")
        exact, delta_e = _counted(engine, lambda: w.index._search_exact_device(given, list(dict.fromkeys(given)), 30, 0.0, detailed, 1000))
    want, _ = w.want(simprints, True)
    assert w._freq(hot) == 200, "1 000 rows by ascending key, five chunks per asset"
    _assert_scored(got, want, simprints, detailed, f"{path} unknown frequency")
    want_e = w.want_exact(given, 30, 1000)
    assert [(r.iscc_id_body, r.score, r.matches, r.queried) for r in exact] == [(r.iscc_id_body, r.score, r.matches, r.queried) for r in want_e]
    if detailed:
        assert exact == want_e
    if COUNTERS:
        assert delta["fallback_queries"] >= 2, "the neighbour search and the collision scan behind it"
        assert delta_e["fallback_queries"] == 1
