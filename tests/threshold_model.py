"""
Host model of how many candidates a search may list (numpy only; nothing of the engine is imported here).

Every search of the engine is exact whatever its thresholds are: a threshold that is too loose still contains the top k and the
select sorts the excess away.  What a threshold costs shows only in the length of the candidate lists, which the engine counts
under option ``count_candidates``.  For one Hamming / NPHD segment this module derives, from the table and the queries alone,
the lengths those lists may have ("What a threshold may be"):

    h(q, r)     distance of query q to row r over the compared prefix
    d_k(q, R)   k-th smallest distance over the rows R (the largest when R holds fewer than k rows)
    N(q, t)     rows of the WHOLE segment with h(q, r) <= t

    floor       N(q, d_k(q, all)): every row at or under the k-th distance lies within any valid threshold
    ceiling     N(q, tau0(q)), tau0(q) = d_min(k, s0)(q, rows [0, s0)): no path loosens the threshold of its bootstrap sample
                (a sample shorter than both k and the segment cannot bound the k-th distance: the ceiling is then every row)

A ``Case`` holds what one batch may count, ``check_candidates`` decides.  tests/test_threshold_model.py holds this file to a
brute-force loop, tests/test_gpu_thresholds.py holds the engine to this file.
"""

import numpy as np

BOOT_ROWS = 65536  # rows of the level design's bootstrap sample
HINT_MARGIN_MAX = 2  # a hint lies at most this many bits above the worst k-th distance it was taken from

_POP16 = np.array([bin(i).count("1") for i in range(1 << 16)], dtype=np.uint8)


def prefix_masks(pbytes, max_words):
    # type: (int, int) -> np.ndarray
    """uint64 [max_words]: the bits of every big-endian packed word that lie inside a compared prefix of ``pbytes`` bytes."""
    masks = np.zeros(max_words, dtype=np.uint64)
    for w in range(max_words):
        inside = min(8, max(0, pbytes - 8 * w))
        if inside:
            masks[w] = np.uint64((0xFFFFFFFFFFFFFFFF << (8 * (8 - inside))) & 0xFFFFFFFFFFFFFFFF)
    return masks


def distances(words, q_words, pbytes):
    # type: (np.ndarray, np.ndarray, int) -> np.ndarray
    """
    h(q, r) for every query and row: int32 [nq, n].

    :param words: uint64 [n, max_words] rows, big-endian packed
    :param q_words: uint64 [nq, max_words] queries, packed alike
    :param pbytes: compared prefix in bytes (Hamming: the table's code length; NPHD: min(query length, row length))
    """
    words = np.ascontiguousarray(words, dtype=np.uint64)
    q_words = np.ascontiguousarray(q_words, dtype=np.uint64)
    n, max_words = words.shape
    masks = prefix_masks(pbytes, max_words)
    out = np.zeros((q_words.shape[0], n), dtype=np.int32)
    for qi in range(q_words.shape[0]):
        for w in range(max_words):
            if not masks[w]:
                continue
            x = np.ascontiguousarray((words[:, w] ^ q_words[qi, w]) & masks[w])
            out[qi] += _POP16[x.view(np.uint16).reshape(n, 4)].sum(axis=1, dtype=np.int32)
    return out


def kth_distance(dist, k):
    # type: (np.ndarray, int) -> np.ndarray
    """d_k per query over the rows given: int64 [nq]; with fewer than k rows the largest distance among them."""
    nq, n = dist.shape
    if n == 0:
        raise ValueError("d_k over no rows")
    kk = min(k, n)
    return np.partition(dist, kk - 1, axis=1)[:, kk - 1].astype(np.int64)


def count_within(dist, t):
    # type: (np.ndarray, np.ndarray | int) -> np.ndarray
    """N(q, t) per query: int64 [nq]; ``t`` one threshold or one per query."""
    t = np.broadcast_to(np.asarray(t, dtype=np.int64), (dist.shape[0],))
    return (dist <= t[:, None]).sum(axis=1, dtype=np.int64)


def s0_single(n, k, self_boot_rows, self_boot_per_k):
    # type: (int, int, int, int) -> int
    """
    Rows of the bootstrap sample of the single self-tightening pass (options ``self_boot_rows`` / ``self_boot_per_k``); never fewer
    than k of them, whose worst would bound nothing (the two agree wherever k <= self_boot_rows).
    """
    return min(n, max(self_boot_rows, k, min(self_boot_per_k * k, n // 8)))


def s0_levels(n):
    # type: (int) -> int
    """Rows of the bootstrap sample of the level design."""
    return min(n, BOOT_ROWS)


class Case:
    """
    What one batch's candidate count may be.

    kind        "exact"     one value (floor and ceiling coincide, or the threshold is given)
                "interval"  anything from ``lo`` to ``hi``
                "one_tau"   ONE query whose list was pruned to one integer threshold tau, d_k <= tau <= tau0: N(q, tau) for one of them
                "one_r"     every query listed under ONE radius r, worst <= r <= worst + 2: sum_q N(q, r) for one of them
    lo, hi      smallest and largest admissible count
    allowed     the admissible counts when they are a set ("exact", "one_tau", "one_r"), else None
    per_query   largest list a single query of the batch may hold (the model's precondition: it must stay below the buffer)
    """

    def __init__(self, kind, lo, hi, allowed, per_query):
        self.kind, self.lo, self.hi, self.per_query = kind, int(lo), int(hi), int(per_query)
        self.allowed = None if allowed is None else frozenset(int(a) for a in allowed)
        if self.lo > self.hi:
            raise ValueError(f"floor {self.lo} above ceiling {self.hi}")
        if self.allowed is not None and (min(self.allowed) != self.lo or max(self.allowed) != self.hi):
            raise ValueError("admissible set and bounds disagree")

    def admits(self, observed):
        # type: (int) -> bool
        if self.allowed is not None:
            return int(observed) in self.allowed
        return self.lo <= int(observed) <= self.hi

    def __repr__(self):
        what = sorted(self.allowed) if self.allowed is not None and len(self.allowed) <= 8 else f"[{self.lo}, {self.hi}]"
        return f"Case({self.kind}, {what})"


def floor_counts(dist, k):
    # type: (np.ndarray, int) -> np.ndarray
    """N(q, d_k(q, all)) per query."""
    return count_within(dist, kth_distance(dist, k))


def boot_thresholds(dist, k, s0):
    # type: (np.ndarray, int, int) -> np.ndarray
    """
    tau0(q) = d_min(k, s0)(q, rows [0, s0)).  A sample of fewer than k rows that is not the whole segment bounds nothing -- the
    k-th row may lie anywhere beyond its worst -- so no valid threshold cuts there: every row stays within it.
    """
    if not 1 <= s0 <= dist.shape[1]:
        raise ValueError(f"sample of {s0} rows outside 1..{dist.shape[1]}")
    if s0 < min(k, dist.shape[1]):
        return dist.max(axis=1).astype(np.int64)
    return kth_distance(dist[:, :s0], k)


def ceiling_counts(dist, k, s0):
    # type: (np.ndarray, int, int) -> np.ndarray
    """N(q, tau0(q)) per query."""
    return count_within(dist, boot_thresholds(dist, k, s0))


def one_tau_counts(dist, k, s0):
    # type: (np.ndarray, int, int) -> list
    """ONE query: N(q, tau) for every integer tau from d_k(q, all) to tau0(q)."""
    if dist.shape[0] != 1:
        raise ValueError("the admissible thresholds of a list are known for a batch of one query only")
    lo, hi = int(kth_distance(dist, k)[0]), int(boot_thresholds(dist, k, s0)[0])
    return [int(count_within(dist, t)[0]) for t in range(lo, hi + 1)]


def topk_case(dist, k, s0, pruned=False):
    # type: (np.ndarray, int, int, bool) -> Case
    """
    A top-k batch that took a bootstrap sample of ``s0`` rows.

    ``pruned``: the level design, whose lists are pruned to the threshold after every pick -- a batch of ONE query then counts
    N(q, tau) for one integer tau ("one_tau"); the single pass never prunes and several queries only bound each other's sum.
    """
    lo, hi = floor_counts(dist, k), ceiling_counts(dist, k, s0)
    if s0 == dist.shape[1]:
        return Case("exact", lo.sum(), hi.sum(), [lo.sum()], hi.max())      # (the sample is the segment: tau0 = d_k)
    if pruned and dist.shape[0] == 1:
        return Case("one_tau", lo.sum(), hi.sum(), one_tau_counts(dist, k, s0), hi.max())
    return Case("interval", lo.sum(), hi.sum(), None, hi.max())


def radius_case(dist, radius):
    # type: (np.ndarray, int) -> Case
    """``search_within``: one scan under the given radius, no sample."""
    c = count_within(dist, radius)
    return Case("exact", c.sum(), c.sum(), [c.sum()], c.max())


def worst_kth(dist, k):
    # type: (np.ndarray, int) -> int
    """max_q d_k(q, all): where the lists of a batch end, and what the next batch's hint is taken from."""
    return int(kth_distance(dist, k).max())


def speculative_case(dist, k):
    # type: (np.ndarray, int) -> Case
    """The second identical small batch: ONE range-limited pass under r = worst + margin, the margin one or two bits."""
    worst = worst_kth(dist, k)
    sums = [count_within(dist, r) for r in range(worst, worst + HINT_MARGIN_MAX + 1)]
    return Case("one_r", sums[0].sum(), sums[-1].sum(), [s.sum() for s in sums], sums[-1].max())


def self_hint_case(dist, k):
    # type: (np.ndarray, int) -> Case
    """The second identical larger batch: its single pass starts under the hint and tightens every query's threshold from there."""
    hi = count_within(dist, worst_kth(dist, k) + HINT_MARGIN_MAX)
    return Case("interval", floor_counts(dist, k).sum(), hi.sum(), None, hi.max())


def check_candidates(observed, case):
    # type: (int, Case) -> None
    """AssertionError unless ``observed`` (candidates the engine counted for the batch) is a count ``case`` admits."""
    if case.admits(observed):
        return
    where = "below the floor" if observed < case.lo else "above the ceiling" if observed > case.hi else "between two admissible counts"
    raise AssertionError(f"{observed} candidates are {where} of {case!r}: floor {case.lo}, ceiling {case.hi}")
