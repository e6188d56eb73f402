"""
The thresholds and candidate lists of the search against the host model of tests/threshold_model.py.

The parity tests cannot see this code go wrong: a bootstrap cut one bin high, a sample tail that misses the rows of its last trip or a
pick that keeps entries above its new threshold all return the oracle's bits -- later, or by way of a retry.  Under option
``count_candidates`` the engine reports how many candidates a one-segment batch listed; here that count is held to what the model
derives from the table and the queries ("What a threshold may be").  Every expected value is an integer: none is a tolerance.

Every case runs with the one-launch search off (``tiny_rows=0``), asserts that the counter saw exactly the batches of the call, that
no query took the fallback or the retry with levels, that the intended kernels ran -- and that the same call returned the oracle's
results, so that no query can sit below its floor.  The model's precondition (every list fits the buffer) is asserted first.

Paths: XOR + popcount with levels (8 and 16 queries per pass), matrix cores with levels, matrix cores in one self-tightening pass; on
the matrix cores the unpacked kernel (longer codes, masked codes, 64-bit codes with an all-zero query in the batch),
``mfma_pack_kernel`` (64-bit codes, <= 128 queries) and ``mfma_pack3_kernel`` (64-bit codes, >= 129 queries).

Run with ``-s`` to see every observed count beside its floor and ceiling.
"""

import numpy as np
import pytest

import threshold_model as tm
from oracle import oracle_topk

pytestmark = pytest.mark.gpu

METRIC_HAMMING, METRIC_NPHD = 0, 1

COMMON = dict(count_candidates=1, speculate=0, tiny_rows=0)
_MATRIX = dict(mfma=1, mfma_pack=1, mfma_pack3=1, mfma_min_queries=1, mfma_min_rows=1)
PATHS = {
    "xor8": dict(mfma=0, queries_per_pass=8),
    "xor16": dict(mfma=0, queries_per_pass=16),
    "mfma_levels": dict(_MATRIX, self_tighten=0),
    "mfma_single": dict(_MATRIX, self_tighten=1),
}
LEVEL_PATHS = ["xor8", "xor16", "mfma_levels"]
ALL_PATHS = list(PATHS)

# name -> (rows, code bytes, key words, metric, clustered); NPHD tables hold rows of that length and are asked with 8-byte queries
TABLES = {
    "r100": (100, 8, 1, METRIC_HAMMING, False),
    "r4096": (4096, 8, 1, METRIC_HAMMING, False),
    "r4097": (4097, 8, 1, METRIC_HAMMING, False),
    "r4097x16": (4097, 16, 1, METRIC_HAMMING, False),
    "r5003x20": (5003, 20, 1, METRIC_HAMMING, False),          # no multiple of 64, 128 or 192 rows
    "r5003x16": (5003, 16, 1, METRIC_HAMMING, False),
    "r12289": (4096 + 8 * 1024 + 1, 8, 1, METRIC_HAMMING, False),      # one row into the second trip of a 1 024-thread block's tail
    "r12289x13": (4096 + 8 * 1024 + 1, 13, 1, METRIC_HAMMING, False),
    "c12289": (4096 + 8 * 1024 + 1, 8, 1, METRIC_HAMMING, True),
    "r30001nphd": (30_001, 32, 1, METRIC_NPHD, False),
    "r60000": (60_000, 8, 1, METRIC_HAMMING, False),
    "r60000x24": (60_000, 24, 1, METRIC_HAMMING, False),
    "r60000x32k2": (60_000, 32, 2, METRIC_HAMMING, False),
    "r65536": (65_536, 8, 1, METRIC_HAMMING, False),
    "r65536x32": (65_536, 32, 1, METRIC_HAMMING, False),
    "r40000": (40_000, 8, 1, METRIC_HAMMING, False),
    "r40000x13": (40_000, 13, 1, METRIC_HAMMING, False),
    "r40000x16": (40_000, 16, 1, METRIC_HAMMING, False),
    "r65537": (65_537, 8, 1, METRIC_HAMMING, False),
    "r70001": (70_001, 8, 1, METRIC_HAMMING, False),
    "r70001x16": (70_001, 16, 1, METRIC_HAMMING, False),
    "r100003": (100_003, 8, 1, METRIC_HAMMING, False),
    "r200001": (200_001, 8, 1, METRIC_HAMMING, False),
    "c200001": (200_001, 8, 1, METRIC_HAMMING, True),
}
NPHD_QUERY_BYTES = 8


def _seed(*parts):
    return [sum(ord(c) for c in str(p)) + 1000 * i for i, p in enumerate(parts)]


def _flip(rng, words, bits, prefix_bits):
    """Flip ``bits[i]`` random bits of row i within the first ``prefix_bits`` bits (big-endian packed: bit 0 is the top of word 0)."""
    for i, nb in enumerate(bits):
        for b in rng.choice(prefix_bits, size=int(nb), replace=False):
            words[i, b // 64] ^= np.uint64(1) << np.uint64(63 - b % 64)


def _flip_two(rng, words, prefix_bits):
    """Flip two distinct random bits of every row within the first ``prefix_bits`` bits."""
    n = len(words)
    first = rng.integers(0, prefix_bits, size=n)
    for b in (first, (first + rng.integers(1, prefix_bits, size=n)) % prefix_bits):
        words[np.arange(n), b // 64] ^= np.uint64(1) << (63 - b % 64).astype(np.uint64)


class World:
    """Host data, device tables, queries, distances and oracle results, each made once and shared by the cases that name them."""

    def __init__(self, engine):
        self.engine = engine
        self.host, self.tables, self.query_sets, self.dists, self.oracles = {}, {}, {}, {}, {}

    def data(self, name):
        """(keys, words, row lengths or None) of a table."""
        if name not in self.host:
            n, nbytes, key_words, metric, clustered = TABLES[name]
            rng = np.random.default_rng(_seed("rows", name))
            W = (nbytes + 7) // 8
            masks = tm.prefix_masks(nbytes, W)
            if clustered:
                # a pool of 64 codes, two random bits flipped per row: every cut falls inside a large tie class
                pool = rng.integers(0, 2**64, size=(64, W), dtype=np.uint64) & masks
                words = pool[rng.integers(0, 64, size=n)]
                _flip_two(rng, words, 8 * nbytes)
            else:
                words = rng.integers(0, 2**64, size=(n, W), dtype=np.uint64) & masks
            if key_words == 2:
                keys = np.stack([rng.integers(1, 300, size=n).astype(np.uint64), rng.permutation(n).astype(np.uint64)], axis=1)
            else:
                keys = rng.permutation(n).astype(np.uint64) + np.uint64(7)
            self.host[name] = (keys, words, np.full(n, nbytes, dtype=np.uint8) if metric == METRIC_NPHD else None)
        return self.host[name]

    def open(self, name):
        """A new device table of that data (the caller drops it): a hint is kept per table, so speculation cases start fresh."""
        _, nbytes, key_words, metric, _ = TABLES[name]
        keys, words, lens = self.data(name)
        t = self.engine.open_table(metric, key_words, nbytes)
        t.add(keys, words, lens)
        assert t.segments() == {nbytes: len(keys)}, "the counter only counts one-segment batches"
        return t

    def table(self, name):
        if name not in self.tables:
            self.tables[name] = self.open(name)
        return self.tables[name]

    def pbytes(self, name):
        return NPHD_QUERY_BYTES if TABLES[name][3] == METRIC_NPHD else TABLES[name][1]

    def queries(self, name, nq, zero=False):
        """
        (words, lengths or None): a third random, a third near-duplicates of rows at 0..14 flipped bits (thresholds spread over a
        batch), a third rows of the table's own distribution.  ``zero``: query 1 is all zeros, which keeps 64-bit batches off the
        packed kernels; no other query is.
        """
        key = (name, nq, zero)
        if key not in self.query_sets:
            _, nbytes, _, metric, clustered = TABLES[name]
            _, words, _ = self.data(name)
            rng = np.random.default_rng(_seed("queries", name, nq, zero))
            pb = self.pbytes(name)
            W = words.shape[1]
            masks = tm.prefix_masks(pb, W)
            q = words[rng.integers(0, len(words), size=nq)] & masks
            kind = np.arange(nq) % 3 if nq > 1 else np.array([1])
            _flip(rng, q, np.where(kind == 1, rng.integers(0, 15, size=nq), np.where(kind == 2, 2 if clustered else 0, 0)), 8 * pb)
            if not clustered:
                rnd = rng.integers(0, 2**64, size=(nq, W), dtype=np.uint64) & masks
                q[kind == 0] = rnd[kind == 0]
            q[~q.any(axis=1), 0] = np.uint64(1) << np.uint64(63)
            if zero:
                q[1] = 0
            self.query_sets[key] = (q, np.full(nq, pb, dtype=np.uint8) if metric == METRIC_NPHD else None)
        return self.query_sets[key]

    def dist(self, name, nq, zero=False):
        key = (name, nq, zero)
        if key not in self.dists:
            d = tm.distances(self.data(name)[1], self.queries(name, nq, zero)[0], self.pbytes(name))
            d.setflags(write=False)
            self.dists[key] = d
        return self.dists[key]

    def oracle(self, name, nq, k, zero=False):
        key = (name, nq, k, zero)
        if key not in self.oracles:
            _, nbytes, _, metric, _ = TABLES[name]
            keys, words, lens = self.data(name)
            q, qn = self.queries(name, nq, zero)
            self.oracles[key] = oracle_topk(metric, keys, words, lens, q, qn, k, fixed_nbytes=0 if metric == METRIC_NPHD else nbytes)
        return self.oracles[key]

    def close(self):
        for t in self.tables.values():
            t.drop()
        self.tables.clear()


@pytest.fixture(scope="module")
def world(hip_engine):
    w = World(hip_engine)
    yield w
    w.close()


def _assert_results(got, exp, what):
    for g, e, name in zip(got, exp, ("keys", "hamming", "prefix_bits", "count")):
        np.testing.assert_array_equal(g, e, err_msg=f"{what}: {name}")


def _packed(world, name, zero):
    """Whether a matrix-core launch over this table runs the packed kernels: one compared word, no all-zero query of 64 bits."""
    return world.pbytes(name) <= 8 and not zero


def _counted(engine, call, path, packed, batches=1):
    """Run ``call`` once; (its results, the candidates counted for it) after the assertions every case shares."""
    before = engine.stats()
    got = call()
    after = engine.stats()
    delta = {name: after[name] - before[name] for name in after}
    assert delta["candidate_batches"] == batches, "the counter must see exactly the batches of this call"
    assert delta["fallback_queries"] == 0 and delta["self_retries"] == 0, "a list overflowed: the count is not the scan's"
    if path.startswith("xor"):
        assert delta["mfma_launches"] == 0, "the batch was to stay on the XOR + popcount kernels"
    else:
        assert delta["mfma_launches"] > 0, "the batch was to run on the matrix cores"
        if packed:
            assert delta["mfma_pack_launches"] == delta["mfma_launches"], "the batch was to run on the packed kernels"
        else:
            assert delta["mfma_pack_launches"] == 0, "the batch was to run on the unpacked kernel"
    return got, int(delta["candidates"]), delta


def _check(engine, case, observed, what):
    print(f"\n[thresholds] {what}: observed {observed}, floor {case.lo}, ceiling {case.hi} ({case.kind})", end="")
    tm.check_candidates(observed, case)


def _fits(engine, case):
    assert case.per_query < engine.get_option("candidate_cap"), "model precondition: every list must fit the candidate buffer"


def _s0(engine, path, n, k):
    if path == "mfma_single":
        return tm.s0_single(n, k, engine.get_option("self_boot_rows"), engine.get_option("self_boot_per_k"))
    return tm.s0_levels(n)


def _topk(world, path, name, k, nq, zero=False, extra=None, expect_kind=None, twice=False):
    engine = world.engine
    t = world.table(name)
    q, qn = world.queries(name, nq, zero)
    dist = world.dist(name, nq, zero)
    with engine.options(**COMMON, **PATHS[path], **(extra or {})):
        case = tm.topk_case(dist, k, _s0(engine, path, dist.shape[1], k), pruned=path != "mfma_single")
        if expect_kind:
            assert case.kind == expect_kind, f"the case was built to be '{expect_kind}'"
        _fits(engine, case)
        got, observed, _ = _counted(engine, lambda: t.search(q, qn, k), path, _packed(world, name, zero))
        _assert_results(got, world.oracle(name, nq, k, zero), f"{name} {path}")
        _check(engine, case, observed, f"{path} {name} k={k} nq={nq}{' zero-query' if zero else ''} {extra or ''}")
        if twice:
            _, again, _ = _counted(engine, lambda: t.search(q, qn, k), path, _packed(world, name, zero))
            assert again == observed, "two identical calls of the level design must list the same candidates"


# ---------------------------------------------------------------------------------------------------------------------------------
# the sample is the whole segment: floor and ceiling coincide, on every path the count is sum_q N(q, d_k(q, all)) exactly
# ---------------------------------------------------------------------------------------------------------------------------------
EXACT = [
    # table, k, queries, all-zero query
    ("r4096", 10, 5, False),            # no tail
    ("r4097", 10, 64, False),           # boot_kernel at its largest batch: the tail sees one row
    ("r4097x16", 1, 65, False),         # boot_multi_kernel with padding queries: the tail sees one row
    ("r12289", 10, 160, False),         # boot_multi_kernel: one row into a second trip; mfma_pack3_kernel
    ("r12289", 10, 65, True),           # ... with an all-zero query: the unpacked kernel on 64-bit codes
    ("r12289x13", 10, 1, False),        # boot_kernel: one row into a second trip, masked last word
    ("c12289", 10, 64, False),          # every cut inside a large tie class
    ("r5003x20", 10, 65, False),
    ("r5003x16", 10, 160, False),
    ("r60000", 1024, 5, False),         # k * 4 == 4 096: the last k whose sample keeps a tail
    ("r60000", 1025, 5, False),         # ... and the first whose whole sample stays exact
    ("r60000x24", 1024, 65, False),
    ("r60000x32k2", 1025, 65, False),   # 128-bit keys
    ("r65536", 1, 1, False),
    ("r65536x32", 10, 160, False),
    ("r100", 150, 5, False),            # k >= n
    ("r30001nphd", 10, 64, False),      # NPHD: 32-byte rows asked with 8-byte queries
]


@pytest.mark.parametrize("name,k,nq,zero", EXACT, ids=[f"{n}-k{k}-q{q}{'-zero' if z else ''}" for n, k, q, z in EXACT])
@pytest.mark.parametrize("path", ALL_PATHS)
def test_exact_when_the_sample_is_the_segment(world, path, name, k, nq, zero):
    # (a session that lowers self_boot_rows makes the single pass's sample shorter than some of these tables: the model follows)
    default_sample = path != "mfma_single" or world.engine.get_option("self_boot_rows") >= TABLES[name][0]
    _topk(world, path, name, k, nq, zero, expect_kind="exact" if default_sample else None)


# ---------------------------------------------------------------------------------------------------------------------------------
# the sample is shorter than the segment
# ---------------------------------------------------------------------------------------------------------------------------------
SINGLE = [
    # table, k, queries, all-zero query, sample rows
    ("r40000", 3, 40, False, 3072),         # mfma_pack_kernel
    ("r40000", 10, 160, False, 5000),       # mfma_pack3_kernel
    ("r40000", 3, 40, True, 3072),          # unpacked kernel, 64-bit codes
    ("r40000x16", 3, 40, False, 3072),      # unpacked kernel
    ("r40000x16", 10, 160, False, 5000),
    ("r40000x13", 10, 160, False, 5000),    # ... masked last word
]


@pytest.mark.parametrize("name,k,nq,zero,s0", SINGLE, ids=[f"{n}-k{k}-q{q}{'-zero' if z else ''}" for n, k, q, z, _ in SINGLE])
def test_single_pass_between_floor_and_bootstrap_ceiling(world, name, k, nq, zero, s0):
    assert tm.s0_single(TABLES[name][0], k, 256, world.engine.get_option("self_boot_per_k")) == s0
    _topk(world, "mfma_single", name, k, nq, zero, extra=dict(self_boot_rows=256), expect_kind="interval")


def test_single_pass_samples_at_least_k_rows(hip_engine):
    """
    A sample shorter than k bounds nothing: with the first 256 rows equal to a query, ``self_boot_rows=256`` and k = 300 over 2 000
    rows (n / 8 < k) a 256-row sample ends at distance 0 and the pass lists 256 rows for that query -- fewer than it must return.
    """
    rng = np.random.default_rng(300)
    n, k, nq = 2_000, 300, 5
    words = rng.integers(0, 2**64, size=(n, 1), dtype=np.uint64)
    q = rng.integers(1, 2**64, size=(nq, 1), dtype=np.uint64)
    words[:256] = q[0]
    keys = rng.permutation(n).astype(np.uint64) + np.uint64(7)
    dist = tm.distances(words, q, 8)
    t = hip_engine.open_table(METRIC_HAMMING, 1, 8)
    try:
        t.add(keys, words)
        with hip_engine.options(**COMMON, **PATHS["mfma_single"], self_boot_rows=256):
            s0 = tm.s0_single(n, k, 256, hip_engine.get_option("self_boot_per_k"))
            assert s0 == k
            case = tm.topk_case(dist, k, s0)
            _fits(hip_engine, case)
            got, observed, _ = _counted(hip_engine, lambda: t.search(q, None, k), "mfma_single", True)
            np.testing.assert_array_equal(got[3], np.full(nq, k))
            _assert_results(got, oracle_topk(METRIC_HAMMING, keys, words, None, q, None, k, fixed_nbytes=8), "short sample")
            _check(hip_engine, case, observed, f"mfma_single planted rows k={k} nq={nq} self_boot_rows=256")
    finally:
        t.drop()


LEVELS = [
    # table, k, queries, options, kind
    ("r65537", 10, 1, {}, "one_tau"),       # the sample is one row short of the table; no levels
    ("r65537", 10, 24, {}, "interval"),
    ("r200001", 10, 1, {}, "one_tau"),
    ("r200001", 100, 1, {}, "one_tau"),
    ("r200001", 10, 24, {}, "interval"),
    ("r200001", 10, 24, {"stretch_mb": 1}, "interval"),      # the collect pass in stretches, a pick between them
    ("c200001", 10, 1, {}, "one_tau"),
    ("c200001", 10, 24, {}, "interval"),
    ("c200001", 10, 24, {"stretch_mb": 1}, "interval"),
]


@pytest.mark.parametrize("name,k,nq,extra,kind", LEVELS, ids=[f"{n}-k{k}-q{q}{'-stretch' if e else ''}" for n, k, q, e, _ in LEVELS])
@pytest.mark.parametrize("path", LEVEL_PATHS)
def test_levels_end_at_one_threshold_between_floor_and_ceiling(world, path, name, k, nq, extra, kind):
    _topk(world, path, name, k, nq, extra=extra, expect_kind=kind, twice=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# fixed radius: one scan launch under the given threshold, no sample
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nq,zero", [("r70001", 5, False), ("r70001", 40, False), ("r70001", 40, True), ("r70001", 160, False),
                                          ("r70001x16", 24, False)])
@pytest.mark.parametrize("radius", [0, 12, 20])
@pytest.mark.parametrize("path", ALL_PATHS)
def test_fixed_radius_lists_exactly_the_rows_within_it(world, path, radius, name, nq, zero):
    engine = world.engine
    t = world.table(name)
    q, qn = world.queries(name, nq, zero)
    dist = world.dist(name, nq, zero)
    case = tm.radius_case(dist, radius)
    within = tm.count_within(dist, radius)
    k = max(1, int(within.max()))             # the ceiling of the list lengths: every list comes back whole
    with engine.options(**COMMON, **PATHS[path]):
        _fits(engine, case)
        got, observed, delta = _counted(engine, lambda: t.search_within(q, qn, k, radius), path, _packed(world, name, zero))
        assert delta["scan_launches"] == 1 and delta["level_launches"] == 0
        _check(engine, case, observed, f"{path} {name} radius={radius} nq={nq}{' zero-query' if zero else ''}")
    np.testing.assert_array_equal(got[3], within)
    ek, eh, ep, _ = world.oracle(name, nq, k, zero)
    for i in range(nq):
        c = int(within[i])
        np.testing.assert_array_equal(got[0][i, :c], ek[i, :c])
        np.testing.assert_array_equal(got[1][i, :c], eh[i, :c])
        assert not got[0][i, c:].any() and not got[1][i, c:].any()


# ---------------------------------------------------------------------------------------------------------------------------------
# hints: the second identical call starts where the first ended
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["xor8", "mfma_levels", "mfma_single"])
def test_speculative_pass_lists_under_one_radius_above_the_worst_kth(world, path):
    """The first call seeds the hint, the second is ONE range-limited pass under worst + margin (one or two bits, either accepted)."""
    engine, name, k, nq = world.engine, "r100003", 10, 8
    q, qn = world.queries(name, nq)
    dist = world.dist(name, nq)
    exp = world.oracle(name, nq, k)
    t = world.open(name)
    try:
        with engine.options(**dict(COMMON, speculate=1), **PATHS[path], spec_max_queries=128):
            first = tm.topk_case(dist, k, _s0(engine, path, dist.shape[1], k), pruned=path != "mfma_single")
            case = tm.speculative_case(dist, k)
            _fits(engine, first)
            _fits(engine, case)
            got, observed, delta = _counted(engine, lambda: t.search(q, qn, k), path, True)
            assert delta["spec_hits"] == 0 and delta["spec_misses"] == 0, "a new table has no hint"
            _assert_results(got, exp, "seeding call")
            _check(engine, first, observed, f"{path} {name} seeding call k={k} nq={nq}")
            got, observed, delta = _counted(engine, lambda: t.search(q, qn, k), path, True)
            assert delta["spec_hits"] == 1 and delta["spec_misses"] == 0
            assert delta["scan_launches"] == 1 and delta["level_launches"] == 0
            _assert_results(got, exp, "speculative call")
            _check(engine, case, observed, f"{path} {name} speculative call k={k} nq={nq}")
    finally:
        t.drop()


def test_self_hint_starts_the_single_pass_under_the_hint(world):
    """Batches above ``spec_max_queries`` keep their single pass; the second identical one starts it under the hint, without a sample."""
    engine, name, k, nq, path = world.engine, "r100003", 10, 40, "mfma_single"
    q, qn = world.queries(name, nq)
    dist = world.dist(name, nq)
    exp = world.oracle(name, nq, k)
    t = world.open(name)
    try:
        with engine.options(**dict(COMMON, speculate=1), **PATHS[path], spec_max_queries=0, self_hint=1):
            first = tm.topk_case(dist, k, _s0(engine, path, dist.shape[1], k))
            case = tm.self_hint_case(dist, k)
            _fits(engine, first)
            _fits(engine, case)
            got, observed, delta = _counted(engine, lambda: t.search(q, qn, k), path, True)
            assert delta["spec_hits"] == 0 and delta["spec_misses"] == 0, "a new table has no hint"
            _assert_results(got, exp, "seeding call")
            _check(engine, first, observed, f"{path} {name} seeding call k={k} nq={nq}")
            got, observed, delta = _counted(engine, lambda: t.search(q, qn, k), path, True)
            assert delta["spec_hits"] == 1 and delta["spec_misses"] == 0
            assert delta["scan_launches"] == 1 and delta["level_launches"] == 0
            _assert_results(got, exp, "hinted call")
            _check(engine, case, observed, f"{path} {name} hinted call k={k} nq={nq}")
    finally:
        t.drop()
