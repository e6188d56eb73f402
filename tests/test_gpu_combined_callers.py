"""
The combining front of ``isccsearch_search`` (csrc/search_api.hip.h: the queue in ``isccsearch_search`` and ``run_combined``) against
the oracle, at small shapes.

Searches that arrive from several threads are not answered one by one: the first caller leads a round, takes every request that
waits on the handle, groups them by (table, k), runs each group as ONE batch and copies every caller's slice back.  The full-size
concurrency tests (test_gpu_fullsize.py) send one or two 64-bit queries per caller over 100 M rows.  Here a crowd of Python threads
(tests/crowd.py) meets inside the library over tables of 20 011 rows -- just above ``tiny_rows``, so the ordinary pipeline runs --
and every caller's four arrays are held to ``oracle.oracle_topk`` over the table's host copy, bit for bit:

  * 64-bit codes and keys, 128-bit codes and keys (the ``k * KW`` strides of the copy-back), NPHD with four segments where every
    caller mixes lengths (``search_locked`` reorders the combined batch by length, so callers interleave inside it);
  * callers of 1..40 queries, so that combined totals fall on every side of 8/9, 16/17, 128 and -- twelve callers of 100 --
    ``QB_MAX`` = 1 024; under the session's options, with every round on the matrix cores, and with the matrix cores off;
  * several groups in one round: k = 10, 1, 512 and 4 096, and a second table small enough for the one-launch search;
  * five waves of one crowd over 300 007 rows, later ones under the hints that earlier combined rounds recorded, then a crowd
    whose queries miss them;
  * callers that must fail alone (query length, dropped table, count), each reading its own message on its own thread;
  * ``search_within``, ``search_many``, ``doc_freq``, ``stats`` and a writer beside the front on one mutex, with rows arriving in
    the searched table: every answer is the oracle's for one of the table's states, never an older one than the thread saw before;
  * a table dropped while its callers wait.

Combining is made to happen, not left to chance: a blocker (one long ``search_within`` over a synthetic table of its own) takes
the engine's mutex just before the barrier opens, the first caller leads a round of one and waits for the mutex, the others pile
up behind it.  ``test_callers_behind_a_long_call_are_combined`` reads from the statistics that this is so; the parity tests do not
depend on it -- the expected answer of a request is the same whichever round serves it.

Measured on an MI355X (run with ``-s`` to see each crowd's own figures):
  * a crowd of 12 to 28 members takes 0.3-1.6 ms from the barrier to its last member's call;
  * the blocker holds the mutex for 24-28 ms: 131 072 queries over 8 000 003 rows on the matrix cores, 32 768 queries with them
    off (26-27 ms).  That is fifteen times the slowest start-up seen and forty times the usual one; every crowd's last member made
    its call 23 ms or more before the blocker returned;
  * the same requests asked one after the other on one thread take 1-9 ms (24 callers of 1..40 queries) and 2-27 ms (the crowd of
    several groups), the first call of a kind being the slow one; a crowd, threads and blocker included, returns within 25-35 ms.
    The crowd beside the other entry points runs for 2.0 s, which its writer's 1 600 add + remove pairs set.  ``crowd.TIMEOUT_S``
    = 60 s is thirty times that and over a thousand times any other crowd;
  * ``test_callers_behind_a_long_call_are_combined``: 24 requests of 284 queries grew ``candidate_batches`` by 2.
"""

import functools
import os
import threading

import numpy as np
import pytest

import crowd
from crowd import Request, assert_exact, make_queries, make_table, run_crowd, same
from iscc_search_amd import _lib
from iscc_search_amd.engine import _alloc_out
from oracle import np_within

pytestmark = pytest.mark.gpu

ROWS = 20_011                   # just above tiny_rows = 16 384
TINY_ROWS = 3_000               # the one-launch search under default tiny_rows
SIZES = (1, 2, 3, 5, 8, 9, 16, 17, 40)
KINDS = ("h64", "h128", "nphd")
MFMA_ON = "mfma=0" not in os.environ.get("ISCC_HIP_OPTS", "")
PATHS = {
    "session": {},
    "matrix": dict(mfma=1, mfma_min_queries=1, mfma_min_rows=1),       # matrix cores for every round
    "xor": dict(mfma=0),
}


def _path(name):
    marks = [] if name != "matrix" else [pytest.mark.skipif(not MFMA_ON, reason="forces the matrix cores; the session runs with them off")]
    return pytest.param(name, marks=marks, id=name)


class World:
    """The tables, the blocker and the crowds' requests with the oracle's answers: each made once, shared, and left unchanged."""

    def __init__(self, engine):
        self.engine = engine
        self.blocker = crowd.Blocker(engine)
        self.tables = {kind: make_table(engine, np.random.default_rng(100 + i), kind, ROWS) for i, kind in enumerate(KINDS)}
        self.tiny = make_table(engine, np.random.default_rng(200), "h64", TINY_ROWS)
        self._requests = {}

    def block(self):
        """The blocker's call, sized for the options in force now (read before the crowd starts, not inside it)."""
        return functools.partial(self.blocker, self.blocker.queries())

    def requests(self, name, make):
        if name not in self._requests:
            self._requests[name] = make()
        return self._requests[name]

    def sizes(self, kind):
        """24 callers of one k whose numbers of queries are drawn from SIZES (every one of them at least once)."""
        def make():
            rng = np.random.default_rng([1, KINDS.index(kind)])
            nqs = list(SIZES) + list(rng.choice(SIZES, size=24 - len(SIZES)))
            rng.shuffle(nqs)
            return [Request(self.tables[kind], *make_queries(rng, self.tables[kind], int(nq)), 10) for nq in nqs]
        return self.requests(("sizes", kind), make)

    def groups(self, kind):
        """Several (table, k) groups for one round: k = 10, 1, 512, 4 096 on one table, k = 10 on the one-launch table."""
        def make():
            rng = np.random.default_rng([2, KINDS.index(kind)])
            t = self.tables[kind]
            plan = [(t, 10, int(nq)) for nq in rng.choice(SIZES, size=8)] + [(t, 1, int(nq)) for nq in rng.choice(SIZES, size=8)]
            plan += [(t, 512, int(nq)) for nq in (1, 3, 9, 17)] + [(t, 4096, 1)] * 2 + [(self.tiny, 10, int(nq)) for nq in rng.choice(SIZES, size=6)]
            order = rng.permutation(len(plan))
            return [Request(plan[i][0], *make_queries(rng, plan[i][0], plan[i][2]), plan[i][1]) for i in order]
        return self.requests(("groups", kind), make)

    def close(self):
        for t in list(self.tables.values()) + [self.tiny, self.blocker]:
            t.drop()


@pytest.fixture(scope="module")
def world(hip_engine):
    w = World(hip_engine)
    yield w
    w.close()


def _run_exact(world, requests, what, extra=()):
    """The requests (and ``extra`` members) as one crowd behind the blocker; every request's answer is the oracle's."""
    run = run_crowd(list(requests) + list(extra), blocker=world.block())
    print(f"\n{what}: {run.describe()}")
    for i, (req, out) in enumerate(zip(requests, run.outcomes)):
        assert out.error is None, f"{what}: caller {i} ({len(req.q)} queries, k={req.k}) raised {out.error!r}"
        req.check(out.value, f"{what}: caller {i} ({len(req.q)} queries, k={req.k})")
    return run


def test_callers_behind_a_long_call_are_combined(world):
    """
    On a one-segment Hamming table under ``count_candidates=1, speculate=0, tiny_rows=0`` every LockedBatch counts once in
    ``candidate_batches`` (test_gpu_thresholds.py relies on it): 24 callers answered one by one would add 24.  The blocker is a
    call of the same kind, so what it adds alone is measured first and taken off.
    """
    engine = world.engine
    requests = world.sizes("h64")
    with engine.options(count_candidates=1, speculate=0, tiny_rows=0):
        block = world.block()
        s0 = engine.stats()
        block()
        s1 = engine.stats()
        run = run_crowd(requests, blocker=block)
        s2 = engine.stats()
    alone = {name: s1[name] - s0[name] for name in ("searches", "queries", "candidate_batches")}
    delta = {name: s2[name] - s1[name] - alone[name] for name in alone}
    print(f"\n{run.describe()}; {len(requests)} requests -> {delta}; the blocker alone {alone}")
    for i, (req, out) in enumerate(zip(requests, run.outcomes)):
        assert out.error is None, out.error
        req.check(out.value, f"caller {i}")
    assert alone["searches"] == 1 and alone["candidate_batches"] >= 1
    assert delta["searches"] == len(requests)
    assert delta["queries"] == sum(len(r.q) for r in requests)
    assert 1 <= delta["candidate_batches"] < len(requests), "no round held more than one caller"


@pytest.mark.parametrize("path", [_path(p) for p in ("session", "matrix", "xor")])
@pytest.mark.parametrize("kind", KINDS)
def test_callers_of_many_sizes(world, kind, path):
    with world.engine.options(**PATHS[path]):
        _run_exact(world, world.sizes(kind), f"sizes {kind} {path}")


@pytest.mark.parametrize("path", [_path(p) for p in ("session", "matrix", "xor")])
def test_combined_batch_beyond_qb_max(world, path):
    """12 callers x 100 queries: 1 200 > QB_MAX, so one combined group is split over several pipeline runs."""
    def make():
        rng = np.random.default_rng(3)
        return [Request(world.tables["h64"], *make_queries(rng, world.tables["h64"], 100), 10) for _ in range(12)]
    with world.engine.options(**PATHS[path]):
        _run_exact(world, world.requests("qb_max", make), f"12 x 100 {path}")


@pytest.mark.parametrize("path", [_path(p) for p in ("session", "matrix")])
@pytest.mark.parametrize("kind", KINDS)
def test_several_groups_in_one_round(world, kind, path):
    with world.engine.options(**PATHS[path]):
        _run_exact(world, world.groups(kind), f"groups {kind} {path}")


def test_waves_under_recorded_hints(world):
    """
    The same crowd five times over 300 007 rows under the session's ``speculate``, ``self_hint`` and ``radius_batches``: which callers
    share a round differs from wave to wave, so later rounds start under hints that combined batches of other sizes left (a
    range-limited pass, a hinted single pass, a fixed-radius pass with repair).  Then queries far from every planted row: the hints miss.
    """
    engine = world.engine
    rng = np.random.default_rng(5)
    table = make_table(engine, rng, "h64", 300_007)
    try:
        nqs = list(SIZES) + list(rng.integers(1, 41, size=24 - len(SIZES)))
        near = [Request(table, *make_queries(rng, table, int(nq)), 10) for nq in nqs]
        far = [Request(table, *make_queries(rng, table, int(nq), far=True), 10) for nq in nqs]
        for wave, requests in enumerate([near] * 5 + [far]):
            before = engine.stats()
            _run_exact(world, requests, f"wave {wave}")
            after = engine.stats()
            print(f"wave {wave}: spec_hits + spec_misses grew by {after['spec_hits'] - before['spec_hits']} + {after['spec_misses'] - before['spec_misses']},"
                  f" spec_repairs by {after['spec_repairs'] - before['spec_repairs']}")
    finally:
        table.drop()


def _raw_search(dev, q, qn, k):
    """``isccsearch_search`` without the wrapper's checks: (return code, the calling thread's last error)."""
    out, addr = _alloc_out(len(q), k, dev.key_words)
    rc = dev.engine._lib.isccsearch_search(dev.engine.handle, dev.id, len(q), _lib.ptr(q), _lib.ptr(qn), k, *addr)
    return rc, _lib.last_error()


def _raising(fn, *args):
    """The exception ``fn`` raises and the calling thread's last error right after it."""
    try:
        fn(*args)
    except Exception as e:  # noqa: BLE001
        return e, _lib.last_error()
    return None, _lib.last_error()


def _answer_or_error(request):
    """The request's answer, or the exception it raised with the calling thread's last error."""
    try:
        return request(), None
    except Exception as e:  # noqa: BLE001
        return e, _lib.last_error()


def test_bad_callers_fail_alone(world):
    engine = world.engine
    h64, nphd = world.tables["h64"], world.tables["nphd"]
    rng = np.random.default_rng(6)
    good = [Request(t, *make_queries(rng, t, int(nq)), 10) for t in (h64, nphd) for nq in rng.choice(SIZES, size=6)]
    again = [Request(t, *make_queries(rng, t, int(nq)), 10) for t in (h64, nphd) for nq in rng.choice(SIZES, size=6)]
    q64, _ = make_queries(rng, h64, 3)
    q256, qn = make_queries(rng, nphd, 5)
    too_long = qn.copy()
    too_long[3] = 33
    wrong_bytes = np.array([8, 7, 8], dtype=np.uint8)
    # nothing is opened between this drop and the end of the test: the library gives a dropped id to the next table
    dropped = engine.open_table(0, 1, 8)
    dropped.add(h64.keys[:100], h64.words[:100])
    dropped.drop()
    bad = [
        functools.partial(_raising, h64.dev.search, np.zeros((3, 2), dtype=np.uint64), None, 10),       # two words per 64-bit query
        functools.partial(_raw_search, nphd.dev, q256, too_long, 10),           # in the good NPHD callers' own group
        functools.partial(_raw_search, h64.dev, q64, wrong_bytes, 10),          # in the good Hamming callers' own group
        functools.partial(_raising, dropped.search, q64, None, 10),
        functools.partial(_raising, h64.dev.search, q64, None, 4097),
    ]
    run = _run_exact(world, good, "errors", extra=bad)
    words, length, nbytes, table, count = (o.value for o in run.outcomes[len(good):])
    for o in run.outcomes[len(good):]:
        assert o.error is None, o.error
    assert isinstance(words[0], ValueError) and "code words" in str(words[0]), words            # (the wrapper's own check)
    assert length[0] == -22 and "query 3 length 33 outside 1..32" in length[1], length
    assert nbytes[0] == -22 and "query 1 has 7 bytes" in nbytes[1], nbytes
    assert isinstance(table[0], LookupError) and f"table {dropped.id} is not open" in str(table[0]) and f"table {dropped.id} is not open" in table[1], table
    assert isinstance(count[0], ValueError) and "count 4097 exceeds" in str(count[0]) and "count 4097 exceeds" in count[1], count
    # the front came back with leader_active clear: the next crowd on the handle is served, and exactly
    _run_exact(world, again, "after the errors")


class Reader:
    """
    A thread's repeated call while rows arrive in the searched table.  ``expects[s]`` is the oracle's answer once s batches have
    arrived.  Every answer must be one of them; an answer that came back before the first batch was sent is ``expects[0]``; and the
    states a thread's answers show never go backwards.
    """

    def __init__(self, call, expects, equal, state, max_passes):
        self.call, self.expects, self.equal, self.state, self.max_passes = call, expects, equal, state, max_passes

    def __call__(self):
        seen, passes, last = 0, 0, False
        while passes < self.max_passes:
            # (one more pass after the writer has finished: that one must show the last state)
            last = self.state["done"].is_set()
            got = self.call()
            adding = self.state["adding"].is_set()
            matches = [s for s, e in enumerate(self.expects) if s >= seen and self.equal(got, e)]
            assert matches, f"pass {passes}: the answer is the oracle's for no state from {seen} on (any state: {[s for s, e in enumerate(self.expects) if self.equal(got, e)]})"
            seen = matches[0]
            assert adding or seen == 0, f"pass {passes}: the answer shows state {seen} before any batch was sent"
            passes += 1
            if last:
                final = len(self.expects) - 1
                assert final in matches, f"the answer after the last batch shows states {matches}"
                break
        return passes, seen


def _within_equal(got, expect):
    """(keys, hamming, prefix_bits, count) of ``search_within`` against [np_within's (keys, hamming, prefix_bits) per query]."""
    gk, gh, gp, gc = got
    for i, (ek, eh, ep) in enumerate(expect):
        c = len(eh)
        if int(gc[i]) != c or not (np.array_equal(gk[i, :c], ek) and np.array_equal(gh[i, :c], eh) and np.array_equal(gp[i, :c], ep)):
            return False
    return True


def test_other_entry_points_beside_the_front(world):
    """
    8 ``search`` callers on A, 2 ``search_within`` (radius 0 and 12), 2 ``search_many`` over A and B, ``doc_freq``, ``stats`` and a
    writer share ``h->mu``.  First the writer adds rows to and removes them from C only; then it sends five batches of 50 exact
    copies of one query's code to A, under keys above every key of A.
    """
    engine = world.engine
    rng = np.random.default_rng(7)
    BATCHES, COPIES, K_WIDE = 5, 50, 300
    FIRST_HALF, BETWEEN = 800, 160      # the writer's add + remove pairs on C before the first batch and after each: about 1 ms a pair
    A = make_table(engine, rng, "h64", ROWS)
    B = make_table(engine, rng, "h128", 5_003)
    C = engine.open_table(0, 1, 8)
    try:
        x = make_queries(rng, A, 1, far=True)[0]                           # the code the writer copies: no row of A holds it
        new_keys = np.uint64(A.keys.max()) + np.arange(1, BATCHES * COPIES + 1, dtype=np.uint64)
        A.keys = np.concatenate([A.keys, new_keys])
        A.words = np.concatenate([A.words, np.repeat(x, BATCHES * COPIES, axis=0)])
        states = [ROWS + COPIES * s for s in range(BATCHES + 1)]
        state = {"adding": threading.Event(), "done": threading.Event()}
        MAX_PASSES = 20_000                # no thread loops without a bound; the writer's own passes set the length of the run

        def with_x(nq):
            q = make_queries(rng, A, nq)[0]
            q[nq // 2] = x[0]
            return q

        def reader(call, expects, equal=same):
            return Reader(call, expects, equal, state, MAX_PASSES)

        members = []
        # k = 300 shows how many batches have arrived (1 + 50 s rows at distance 0 ... ), k = 10 only whether any has
        for i in range(8):
            q, k = with_x((1, 2, 3, 5, 8, 9, 16, 17)[i]), (K_WIDE, 10)[i % 2]
            members.append(reader(functools.partial(A.dev.search, q, None, k), [A.oracle(q, None, k, rows) for rows in states]))
        for radius in (0, 12):
            q = with_x(4)
            expects = [[np_within(A.words[:rows], 8, A.keys[:rows], q[i], 8, K_WIDE, radius) for i in range(len(q))] for rows in states]
            members.append(reader(functools.partial(A.dev.search_within, q, None, K_WIDE, radius), expects, _within_equal))
        for i in range(2):
            qa, qb, qa2 = with_x(3), make_queries(rng, B, 2 + i)[0], with_x(20)
            call = functools.partial(engine.search_many, [(A.dev, qa, None, K_WIDE, None), (B.dev, qb, None, 10, None), (A.dev, qa2, None, 10, 12)])
            eb = B.oracle(qb, None, 10)
            expects = [(A.oracle(qa, None, K_WIDE, rows), eb, [np_within(A.words[:rows], 8, A.keys[:rows], qa2[j], 8, 10, 12) for j in range(len(qa2))])
                       for rows in states]
            # one call holds the mutex throughout: its three answers show ONE state
            members.append(reader(call, expects, lambda got, e: same(got[0], e[0]) and same(got[1], e[1]) and _within_equal(got[2], e[2])))
        # 64-bit keys: the document frequency of a code is the number of rows that hold it, up to dup_limit
        qf = np.concatenate([x, A.words[A.dup_row : A.dup_row + 1], A.words[17:18]])
        freq = lambda rows, dup: np.minimum([(A.words[:rows, 0] == c).sum() for c in qf[:, 0]], dup).astype(np.uint32)
        members.append(reader(functools.partial(A.dev.doc_freq, qf, None, 120), [freq(rows, 120) for rows in states], np.array_equal))

        def stats():
            passes, searches = 0, 0
            while not state["done"].is_set() and passes < MAX_PASSES:
                now = engine.stats()["searches"]
                assert now >= searches, "the statistics went backwards"
                searches, passes = now, passes + 1
            return passes, 0

        def writer():
            churned = iter(range(10**6))

            def churn(n):
                for _ in range(n):
                    keys = np.uint64(1000 * next(churned)) + np.arange(1, 201, dtype=np.uint64)
                    C.add(keys, rng.integers(0, 2**64, size=(200, 1), dtype=np.uint64))
                    assert C.remove(keys[:150]) == 150
            try:
                churn(FIRST_HALF)
                state["adding"].set()
                for b in range(BATCHES):
                    rows = slice(states[b], states[b + 1])
                    A.dev.add(A.keys[rows], A.words[rows])
                    churn(BETWEEN)
            finally:
                state["adding"].set()
                state["done"].set()
            return BATCHES, BATCHES

        run = run_crowd(members + [stats, writer], blocker=world.block())
        print(f"\nentry points: {run.describe()}; (passes, last state seen) per thread: {[o.value for o in run.outcomes]}")
        for i, o in enumerate(run.outcomes):
            assert o.error is None, f"member {i}: {o.error!r}"
        assert all(o.value[0] >= 2 for o in run.outcomes[:-1]), "a thread made fewer than two passes"
        assert A.dev.size == states[-1]
        q = with_x(9)
        assert_exact(A.dev.search(q, None, K_WIDE), A.oracle(q, None, K_WIDE), "serial search over the final table")
        np.testing.assert_array_equal(A.dev.doc_freq(qf, None, 1000), freq(states[-1], 1000))
        assert C.size == 50 * (FIRST_HALF + BETWEEN * BATCHES)
    finally:
        for t in (A, B, C):
            t.drop()


def test_table_dropped_under_its_callers(world):
    """Callers of D wait behind the blocker and so does the call that drops D: each gets the oracle's answer or the unknown-table error."""
    engine = world.engine
    rng = np.random.default_rng(8)
    D = make_table(engine, rng, "h64", ROWS)
    try:
        on_a = [Request(world.tables["h64"], *make_queries(rng, world.tables["h64"], int(nq)), 10) for nq in rng.choice(SIZES, size=8)]
        on_d = [Request(D, *make_queries(rng, D, int(nq)), 10) for nq in rng.choice(SIZES, size=8)]
        callers = [functools.partial(_answer_or_error, r) for r in on_d]
        run = _run_exact(world, on_a, "drop", extra=callers[:4] + [D.drop] + callers[4:])
        outcomes = run.outcomes[len(on_a):]
        assert outcomes[4].error is None, f"the drop itself failed: {outcomes[4].error!r}"
        answered = 0
        for i, (req, o) in enumerate(zip(on_d, outcomes[:4] + outcomes[5:])):
            assert o.error is None, o.error
            error, message = o.value
            if message is None:
                req.check(error, f"caller {i} of the dropped table")
                answered += 1
                continue
            assert isinstance(error, LookupError) and f"table {D.dev.id} is not open" in str(error) and f"table {D.dev.id} is not open" in message, (i, error, message)
        print(f"drop: {answered} of {len(on_d)} callers of the dropped table were answered before it went")
    finally:
        D.drop()
