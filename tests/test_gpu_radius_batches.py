"""
Large hinted batches of 64-bit codes as ONE fixed-radius pass with repair (option ``radius_batches``; search_locked, ``Spec::tight``).

A batch above ``spec_max_queries`` whose pass would run ``mfma_pack3_kernel`` is asked under one radius r for all its queries,
r = hint - margin (+ a compile-time slack of 0 or 1 bits); 1 ... 32 queries that find fewer than k rows there are asked again under
the whole hint, more of them send the batch through the hinted single pass, and a query beyond the hint is a miss as before.

The data makes every k-th distance known.  One table of 100 000 random 64-bit rows that lie >= 9 bits from every query used; for
query i exactly k planted rows at distance exactly d_i, each with its own set of flipped bits, and nothing nearer.  Queries are
random, >= 16 bits apart, so that another query's plants lie >= 10 bits away.  k = 10: the hint's margin is 2, a seeding batch of
all d_i = 3 leaves the hint at 5 and r at 3 or 4.  Before the engine is touched every batch is held to the oracle: d_k(q_i) = d_i,
d_1(q_i) = d_i, and the (k + 1)-th nearest row is >= 9 bits away.  Every answer is compared with the oracle's, every step's
``(spec_hits, spec_misses, spec_repairs, scan_launches, level_launches)`` with what the path must do.
"""

import numpy as np
import pytest

import threshold_model as tm
from oracle import oracle_topk

pytestmark = pytest.mark.gpu

K = 10
BASE_ROWS = 100_000
FAR = 9             # base rows lie at least this far from every query
APART = 16          # queries lie at least this far from one another
NQS = [160, 256]    # 5 and 8 query groups: the odd and the even instantiation of mfma_pack3_kernel
# the path under test, whatever options the session runs under (an ISCC_HIP_OPTS rerun sets radius_batches=0 or mfma=0)
ON = dict(mfma=1, mfma_pack=1, mfma_pack3=1, mfma_min_queries=17, mfma_min_rows=65536, self_tighten=1, self_hint=1, speculate=1,
          spec_max_queries=128, radius_batches=1, tiny_rows=16384, candidate_cap=16384, count_candidates=0)
STEP = ("spec_hits", "spec_misses", "spec_repairs", "scan_launches", "level_launches")


def _pairwise(a, b):
    """Hamming distance of every row of a to every row of b: int64 [len(a), len(b)]."""
    return np.bitwise_count(a[:, None, :] ^ b[None, :, :]).sum(axis=2, dtype=np.int64)


class World:
    """The base rows of one code length and a pool of queries that are far from them and from one another."""

    def __init__(self, nbytes, rows, pool, seed):
        rng = np.random.default_rng(seed)
        self.nbytes, self.W = nbytes, nbytes // 8
        self.words = rng.integers(0, 2**64, size=(rows, self.W), dtype=np.uint64)
        self.keys = rng.permutation(rows).astype(np.uint64) + np.uint64(1)
        q = rng.integers(1, 2**64, size=(pool + pool // 4, self.W), dtype=np.uint64)
        nearest = oracle_topk(0, self.keys, self.words, None, q, None, 1, fixed_nbytes=nbytes)[1][:, 0]
        q = q[nearest >= FAR]
        close = _pairwise(q, q) < APART
        np.fill_diagonal(close, False)
        q = q[~close.any(axis=1)]
        assert len(q) >= pool, "the pool lost more queries than it was oversized by"
        self.pool = q[:pool]
        self.pool.setflags(write=False)
        self.words.setflags(write=False)
        self.keys.setflags(write=False)


@pytest.fixture(scope="module")
def world():
    return World(8, BASE_ROWS, 4 * 256 + 8, 20240)


def _plants(rng, q, d, bits):
    """K rows per query at distance exactly d[i] from it, each with its own set of flipped bits: uint64 [len(q) * K, W]."""
    out = np.repeat(q, K, axis=0)
    for i in range(len(q)):
        seen = set()
        while len(seen) < K:
            seen.add(tuple(sorted(rng.choice(bits, size=int(d[i]), replace=False).tolist())))
        for j, flips in enumerate(sorted(seen)):
            for b in flips:
                out[i * K + j, b // 64] ^= np.uint64(1) << np.uint64(63 - b % 64)
    return out


class Case:
    """One table: the world's base rows and the plants of every batch of the case.  ``batches``: one array of d_i per batch."""

    def __init__(self, engine, world, batches, seed):
        rng = np.random.default_rng(seed)
        self.engine, self.world = engine, world
        self.queries, at = [], 0
        for d in batches:
            self.queries.append(np.ascontiguousarray(world.pool[at : at + len(d)]))
            at += len(d)
        assert at <= len(world.pool)
        planted = np.concatenate([_plants(rng, q, d, 8 * world.nbytes) for q, d in zip(self.queries, batches)])
        self.words = np.concatenate([world.words, planted])
        self.keys = np.concatenate([world.keys, rng.permutation(len(planted)).astype(np.uint64) + np.uint64(len(world.keys) + 1)])
        # the data has the k-th distances it was built for: d_1 = d_k = d_i, and the next row is a base row or another query's plant
        self.expected = []
        for q, d in zip(self.queries, batches):
            ek, eh, ep, _ = oracle_topk(0, self.keys, self.words, None, q, None, K + 1, fixed_nbytes=world.nbytes)
            np.testing.assert_array_equal(eh[:, 0], d)
            np.testing.assert_array_equal(eh[:, K - 1], d)
            assert int(eh[:, K].min()) >= FAR
            self.expected.append((ek[:, :K], eh[:, :K], ep[:, :K], np.full(len(q), K, dtype=np.uint32)))
        self.table = engine.open_table(0, 1, world.nbytes)
        self.table.add(self.keys, self.words)

    def ask(self, b, what):
        """Batch b against the oracle; the step's deltas of STEP (+ candidates)."""
        before = self.engine.stats()
        got = self.table.search(self.queries[b], None, K)
        after = self.engine.stats()
        for g, e, name in zip(got, self.expected[b], ("keys", "hamming", "prefix_bits", "count")):
            np.testing.assert_array_equal(g, e, err_msg=f"{what}: {name}")
        self.last = {name: int(after[name] - before[name]) for name in after if name not in ("scan_ms", "level_ms")}
        return tuple(self.last[name] for name in STEP)

    def close(self):
        self.table.drop()


def _d(nq, d=3, at=(), other=5):
    out = np.full(nq, d, dtype=np.int64)
    out[list(at)] = other
    return out


def _run(engine, world, batches, seed, body, **options):
    with engine.options(**dict(ON, **options)):
        case = Case(engine, world, batches, seed)
        try:
            body(case)
        finally:
            case.close()


@pytest.mark.parametrize("nq", NQS)
def test_every_query_within_the_radius_is_one_pass(hip_engine, world, nq):
    """Case 1: all d_i = 3 -> one collect launch, and its lists hold sum_q N(q, r) rows -- the k plants of every query for r = 3 and r = 4 alike."""

    def body(case):
        assert case.ask(0, "seeding") == (0, 0, 0, 1, 0)
        assert case.ask(1, "all within r") == (1, 0, 0, 1, 0)
        assert case.last["candidate_batches"] == 1 and case.last["fallback_queries"] == 0 and case.last["self_retries"] == 0
        dist = tm.distances(case.words, case.queries[1], 8)
        np.testing.assert_array_equal(tm.count_within(dist, 3), tm.count_within(dist, 4))
        assert case.last["candidates"] == int(tm.count_within(dist, 3).sum())
        assert case.last["mfma_pack_launches"] == 1

    _run(hip_engine, world, [_d(nq), _d(nq)], 1, body, count_candidates=1)


@pytest.mark.parametrize("where", ["first", "last", "middle"])
@pytest.mark.parametrize("nq", NQS)
def test_one_short_query_is_repaired(hip_engine, world, nq, where):
    """Case 2: one query at d = 5, the hint itself -- short under r = 3 and r = 4 -- is asked again alone; two launches, one hit."""
    at = {"first": 0, "last": nq - 1, "middle": 32 * (nq // 64)}[where]

    def body(case):
        assert case.ask(0, "seeding") == (0, 0, 0, 1, 0)
        assert case.ask(1, f"one short query at {at}") == (1, 0, 1, 2, 0)
        assert case.last["candidates"] == K * nq, "both passes are counted: k plants per query, the short one's in the second"
        assert case.last["scan_mfma_launches"] == 2 and case.last["mfma_pack_launches"] == 2, "the repair stays on the matrix cores"

    _run(hip_engine, world, [_d(nq), _d(nq, at=[at])], 2, body, count_candidates=1)


@pytest.mark.parametrize("nq", NQS)
def test_a_query_group_of_short_queries_is_repaired(hip_engine, world, nq):
    """Case 3: 32 queries at d = 5, spread over all groups: still one repair pass."""
    at = [i * nq // 32 for i in range(32)]
    assert len({i // 32 for i in at}) == nq // 32

    def body(case):
        assert case.ask(0, "seeding") == (0, 0, 0, 1, 0)
        assert case.ask(1, "32 short queries") == (1, 0, 32, 2, 0)

    _run(hip_engine, world, [_d(nq), _d(nq, at=at)], 3, body)


@pytest.mark.parametrize("nq", NQS)
def test_more_short_queries_take_the_hinted_single_pass(hip_engine, world, nq):
    """Case 4: 33 queries at d = 5: no repair, the hinted single pass answers the whole batch and holds."""
    at = [i * nq // 33 for i in range(33)]
    assert len(set(at)) == 33

    def body(case):
        assert case.ask(0, "seeding") == (0, 0, 0, 1, 0)
        hits, misses, repairs, _, levels = case.ask(1, "33 short queries")
        assert (hits, misses, repairs, levels) == (1, 0, 0, 0)

    _run(hip_engine, world, [_d(nq), _d(nq, at=at)], 4, body)


@pytest.mark.parametrize("nq", NQS)
def test_a_query_beyond_the_hint_is_a_miss(hip_engine, world, nq):
    """Case 5: one query at d = 6, beyond the hint of 5: the repair leaves it short, the ordinary path answers; the next batch hits again."""

    def body(case):
        assert case.ask(0, "seeding") == (0, 0, 0, 1, 0)
        assert case.ask(1, "one query beyond the hint")[:3] == (0, 1, 0)
        assert case.ask(2, "after the miss") == (1, 0, 0, 1, 0)

    _run(hip_engine, world, [_d(nq), _d(nq, at=[nq // 2], other=6), _d(nq)], 5, body)


@pytest.mark.parametrize("nq", NQS)
def test_the_option_turns_the_path_off(hip_engine, world, nq):
    """Case 6: ``radius_batches = 0``: the same batches as one hinted single pass each, nothing repaired; ``self_hint = 0``: no speculation."""

    def body(case):
        assert case.ask(0, "seeding") == (0, 0, 0, 1, 0)
        assert case.ask(1, "all within the hint") == (1, 0, 0, 1, 0)
        assert case.ask(2, "one query at the hint") == (1, 0, 0, 1, 0)
        with case.engine.options(radius_batches=1, self_hint=0):
            assert case.ask(3, "self_hint = 0") == (0, 0, 0, 1, 0)

    _run(hip_engine, world, [_d(nq), _d(nq), _d(nq, at=[7]), _d(nq)], 6, body, radius_batches=0)


@pytest.mark.parametrize("nq", NQS)
def test_a_repair_leaves_the_small_classes_hints_alone(hip_engine, world, nq):
    """Case 7: a one-query search twice before and once after a repaired step: the same verdict and the same candidates."""

    def body(case):
        def one(what):
            step = case.ask(2, what)
            return step, case.last["candidates"]

        assert one("one query, seeding")[0][:3] == (0, 0, 0)
        before = one("one query, under its hint")
        assert before[0] == (1, 0, 0, 1, 0)
        assert case.ask(0, "seeding") == (0, 0, 0, 1, 0)
        assert case.ask(1, "one short query") == (1, 0, 1, 2, 0)
        assert one("one query, after the repair") == before

    _run(hip_engine, world, [_d(nq), _d(nq, at=[nq // 3]), _d(1)], 7, body, count_candidates=1)


@pytest.mark.parametrize("nq,options,packed", [(128, {}, 1), (40, dict(spec_max_queries=0), 1)])
def test_smaller_chunks_keep_their_paths(hip_engine, world, nq, options, packed):
    """
    Case 8: 128 queries are a small batch (one range-limited pass under the whole hint), 40 queries above ``spec_max_queries`` a chunk of
    two groups on ``mfma_pack_kernel`` (the hinted single pass): a query at the hint is within either, one launch and no repair.
    """

    def body(case):
        assert case.ask(0, "seeding") == (0, 0, 0, 1, 0)
        assert case.ask(1, "one query at the hint") == (1, 0, 0, 1, 0)
        assert case.last["mfma_pack_launches"] == packed and case.last["mfma_launches"] == 1

    _run(hip_engine, world, [_d(nq), _d(nq, at=[nq // 2])], 8, body, **options)


def test_longer_codes_keep_the_hinted_single_pass(hip_engine):
    """Case 8, 128-bit codes (nq = 160): their fold compares per-query thresholds, so they keep the hinted single pass on the unpacked kernel."""
    nq = 160
    wide = World(16, 70_000, 2 * nq, 20241)

    def body(case):
        assert case.ask(0, "seeding") == (0, 0, 0, 1, 0)
        assert case.ask(1, "one query at the hint") == (1, 0, 0, 1, 0)
        assert case.last["mfma_pack_launches"] == 0 and case.last["mfma_launches"] == 1

    _run(hip_engine, wide, [_d(nq), _d(nq, at=[nq // 2])], 9, body)
