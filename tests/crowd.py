"""
A crowd of caller threads for ``test_gpu_combined_callers.py``: the data they ask about, the oracle's answers, and the harness that
lets them into the library together behind one long call that holds the engine's mutex.

Nothing here computes an expected answer with the library: every expectation is ``oracle.oracle_topk`` / ``oracle.np_within`` over
the host copy of a table, made before a crowd starts.
"""

import threading
import time

import numpy as np
import pytest

from oracle import oracle_topk

METRIC_HAMMING, METRIC_NPHD = 0, 1
NAMES = ("keys", "hamming", "prefix_bits", "count")

# A crowd's threads are joined under ONE deadline.  Asked one after the other on one thread, the requests of a crowd take 1-27 ms on
# an MI355X, and a crowd with its blocker returns within 35 ms; the one crowd that runs for a set time takes 2.0 s (the module
# docstring of test_gpu_combined_callers.py lists the figures).  60 s is thirty times the longest: a thread alive then is not slow.
TIMEOUT_S = 60.0


class HostTable:
    """Host copy of a table (keys, words, row lengths) beside its device table; ``oracle`` answers a request from the host copy."""

    def __init__(self, engine, metric, key_words, max_bytes, keys, words, lens=None, dup_row=0):
        self.engine, self.metric, self.key_words, self.max_bytes = engine, metric, key_words, max_bytes
        self.keys, self.words, self.lens = keys, words, lens
        self.dup_row = dup_row          # a row of the block of exact duplicates
        self.dev = engine.open_table(metric, key_words, max_bytes)
        self.dev.add(keys, words, lens)

    def oracle(self, q, qn, k, rows=None):
        """The oracle's (keys, hamming, prefix_bits, count) over the host copy (``rows``: over its first rows only)."""
        keys, words, lens = (a if a is None or rows is None else a[:rows] for a in (self.keys, self.words, self.lens))
        return oracle_topk(self.metric, keys, words, lens, q, qn, k, fixed_nbytes=0 if self.metric == METRIC_NPHD else self.max_bytes)

    def drop(self):
        self.dev.drop()


def _mask_to(words, lens):
    """Zero every byte of row i beyond ``lens[i]`` (big-endian packing: byte 0 is the top of word 0)."""
    for w in range(words.shape[1]):
        inside = np.clip(lens.astype(np.int64) - 8 * w, 0, 8).astype(np.uint64)
        mask = np.where(inside == 8, np.uint64(0xFFFFFFFFFFFFFFFF), ~(np.uint64(0xFFFFFFFFFFFFFFFF) >> (inside * np.uint64(8))))
        words[:, w] &= np.where(inside == 0, np.uint64(0), mask)


def make_table(engine, rng, kind, n):
    """
    ``kind``: "h64" (64-bit Hamming, 64-bit keys), "h128" (128-bit Hamming, 128-bit keys) or "nphd" (``max_bytes=32``, rows of 8,
    16, 24 and 32 bytes, 64-bit keys).  Random codes and a block of 40 exact duplicates of one code under scattered keys.
    """
    metric, key_words, max_bytes = {"h64": (METRIC_HAMMING, 1, 8), "h128": (METRIC_HAMMING, 2, 16), "nphd": (METRIC_NPHD, 1, 32)}[kind]
    W = max_bytes // 8
    words = rng.integers(0, 2**64, size=(n, W), dtype=np.uint64)
    lens = None
    if metric == METRIC_NPHD:
        lens = rng.choice(np.array([8, 16, 24, 32], dtype=np.uint8), size=n)
        lens[:4] = (8, 16, 24, 32)
    dup = rng.choice(n, size=40, replace=False)
    words[dup] = words[dup[0]]
    if lens is not None:
        lens[dup] = lens[dup[0]]
        _mask_to(words, lens)
    if key_words == 2:
        # few distinct first words: the second word decides most ties
        keys = np.stack([rng.integers(1, 300, size=n).astype(np.uint64), rng.permutation(n).astype(np.uint64)], axis=1)
    else:
        keys = rng.permutation(n).astype(np.uint64) + np.uint64(5)
    return HostTable(engine, metric, key_words, max_bytes, keys, words, lens, int(dup[0]))


def make_queries(rng, table, nq, far=False):
    """
    ``nq`` queries of ``table``: (words, lengths or None).  Half are random; the others copy a row and flip 0..14 bits of its first
    64, so thresholds and ties differ per query; every fifth of those copies a row of the block of exact duplicates (its forty
    rows tie, and the keys decide).  On an NPHD table every query has a length of its own among 8, 16, 24 and 32
    bytes.  ``far``: random queries only.
    """
    W = table.words.shape[1]
    q = rng.integers(0, 2**64, size=(nq, W), dtype=np.uint64)
    if not far:
        src = rng.integers(0, len(table.words), size=nq)
        src[::10] = table.dup_row
        for i in range(0, nq, 2):
            row = table.words[src[i]].copy()
            if table.lens is not None:
                # a shorter row leaves the query's own random words beyond its length
                keep = int(table.lens[src[i]]) // 8
                row[keep:] = q[i, keep:]
            for b in rng.choice(64, size=(i // 2) % 15, replace=False):
                row[0] ^= np.uint64(1) << np.uint64(int(b))
            q[i] = row
    qn = None
    if table.metric == METRIC_NPHD:
        qn = rng.choice(np.array([8, 16, 24, 32], dtype=np.uint8), size=nq)
        if nq >= 4:
            qn[rng.choice(nq, size=4, replace=False)] = (8, 16, 24, 32)
        _mask_to(q, qn)
    return q, qn


class Request:
    """One caller's search and the oracle's answer to it."""

    def __init__(self, table, q, qn, k, rows=None):
        self.table, self.q, self.qn, self.k = table, q, qn, k
        self.expect = table.oracle(q, qn, k, rows)

    def __call__(self):
        return self.table.dev.search(self.q, self.qn, self.k)

    def check(self, got, what):
        assert_exact(got, self.expect, what)


def assert_exact(got, expect, what):
    for g, e, name in zip(got, expect, NAMES):
        np.testing.assert_array_equal(g, e, err_msg=f"{what}: {name}")


def same(got, expect):
    return all(np.array_equal(g, e) for g, e in zip(got, expect))


class Blocker:
    """
    One long call that holds the engine's mutex while a crowd arrives: a range-limited search (radius 0, k = 1) of many random
    queries over a synthetic table of its own.  Random 64-bit queries collide with no row, so the call is the scans and nothing
    else, under whatever options the engine runs with.  With the matrix cores off a pass takes 16 queries and not 1 024, so the call
    is sized by its number of queries: 131 072 hold the mutex for 24-28 ms on the matrix cores of an MI355X, 32 768 for 26-27 ms
    without them.  A crowd needs 0.3-1.6 ms from its barrier to its last member's call.
    """

    ROWS = 8_000_003
    QUERIES_MATRIX, QUERIES_XOR = 131_072, 32_768

    def __init__(self, engine):
        self.engine = engine
        self.table = engine.open_table(METRIC_HAMMING, 1, 8)
        self.table.add_synthetic(8, self.ROWS, seed=20_251, first_row=0, key_base=1)
        self.q = np.random.default_rng(77).integers(0, 2**64, size=(self.QUERIES_MATRIX, 1), dtype=np.uint64)

    def queries(self):
        return self.QUERIES_MATRIX if self.engine.get_option("mfma") else self.QUERIES_XOR

    def __call__(self, nq=None):
        self.table.search_within(self.q[: nq or self.queries()], None, 1, 0)

    def drop(self):
        self.table.drop()


class Outcome:
    """What one member of a crowd came back with: ``value`` or ``error``, and when it left the barrier (``entered``)."""

    __slots__ = ("value", "error", "entered", "left")

    def __init__(self):
        self.value = self.error = None
        self.entered = self.left = 0.0


class CrowdRun:
    """The outcomes of a crowd in the members' order, and what the harness measured."""

    def __init__(self, outcomes, startup_s, blocker_s, held_s, wall_s):
        self.outcomes = outcomes
        self.startup_s = startup_s      # barrier release -> the last member's call
        self.blocker_s = blocker_s      # how long the blocker's call took (None without a blocker)
        self.held_s = held_s            # the last member's call -> the blocker's return: > 0 when everyone queued behind it
        self.wall_s = wall_s

    def __iter__(self):
        return iter(self.outcomes)

    def describe(self):
        if self.blocker_s is None:
            return f"crowd of {len(self.outcomes)}: start-up {1e3 * self.startup_s:.2f} ms, {1e3 * self.wall_s:.1f} ms in all"
        return (f"crowd of {len(self.outcomes)}: start-up {1e3 * self.startup_s:.2f} ms, blocker {1e3 * self.blocker_s:.1f} ms "
                f"(returned {1e3 * self.held_s:.1f} ms after the last member's call), {1e3 * self.wall_s:.1f} ms in all")


def run_crowd(members, blocker=None, timeout=TIMEOUT_S):
    """
    Run every callable of ``members`` on a thread of its own; they pass a barrier together.  With ``blocker`` (a callable), that call
    is started on one more thread just before the barrier opens, so that it holds the engine's mutex while the members arrive: the
    first member then leads a round of one and waits for the mutex, and the others queue up behind it.

    Threads are daemons and are joined under one deadline.  One still alive then holds the engine's mutex or its queue, and every
    later call of the session would wait behind it: the session ends there (``pytest.exit``), and nothing more is started on the
    GPU.  A crowd is never run a second time.
    """
    outcomes = [Outcome() for _ in members]
    barrier = threading.Barrier(len(members) + 1)
    about_to_block = threading.Event()
    blocker_times = []

    def member(i):
        out = outcomes[i]
        try:
            barrier.wait(timeout)
            out.entered = time.perf_counter()
            out.value = members[i]()
        except BaseException as e:  # noqa: BLE001 -- handed to the test, which decides what each member may raise
            out.error = e
        out.left = time.perf_counter()

    def block():
        about_to_block.set()
        t0 = time.perf_counter()
        try:
            blocker()
        except BaseException as e:  # noqa: BLE001 -- raised again on the test's thread below
            blocker_times.append(e)
        blocker_times.extend((t0, time.perf_counter()))

    threads = [threading.Thread(target=member, args=(i,), daemon=True, name=f"crowd-{i}") for i in range(len(members))]
    for th in threads:
        th.start()
    deadline = time.monotonic() + timeout
    if blocker is not None:
        bt = threading.Thread(target=block, daemon=True, name="crowd-blocker")
        bt.start()
        threads.append(bt)
        # the blocker's thread keeps the interpreter until its call has entered the library (which then lets go of it)
        assert about_to_block.wait(timeout), "the blocker's thread did not start"
    t_open = time.perf_counter()
    barrier.wait(timeout)
    for th in threads:
        th.join(max(0.0, deadline - time.monotonic()))
        if th.is_alive():
            pytest.exit(f"{th.name} did not return within {timeout:.0f} s: a caller hangs in the library; nothing more is started", returncode=1)
    wall = time.perf_counter() - t_open
    release = min(o.entered for o in outcomes if o.entered)
    last = max(o.entered for o in outcomes)
    if blocker is None:
        return CrowdRun(outcomes, last - release, None, None, wall)
    if len(blocker_times) != 2:
        raise blocker_times[0]
    return CrowdRun(outcomes, last - release, blocker_times[1] - blocker_times[0], blocker_times[1] - last, wall)
