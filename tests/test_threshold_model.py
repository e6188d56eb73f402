"""
tests/threshold_model.py against a brute-force loop over Python integers, on inputs small enough to enumerate, and the decisions of
its checker: every admissible count passes, a count one off the admissible set does not.
"""

import numpy as np
import pytest

import threshold_model as tm


def _pack(codes, max_words):
    """Byte strings -> big-endian packed, zero-padded uint64 words."""
    buf = np.zeros((len(codes), max_words * 8), dtype=np.uint8)
    for i, c in enumerate(codes):
        buf[i, : len(c)] = np.frombuffer(c, dtype=np.uint8)
    return buf.view(">u8").astype(np.uint64).reshape(len(codes), max_words)


def _brute_distance(a, b, pbytes):
    return bin(int.from_bytes(a[:pbytes], "big") ^ int.from_bytes(b[:pbytes], "big")).count("1")


def _brute(rows, queries, pbytes):
    return [[_brute_distance(q, r, pbytes) for r in rows] for q in queries]


def _brute_kth(ds, k):
    return sorted(ds)[min(k, len(ds)) - 1]


def _brute_tau0(ds, k, s0):
    """The bootstrap threshold; a sample shorter than both k and the segment bounds nothing."""
    return max(ds) if s0 < min(k, len(ds)) else _brute_kth(ds[:s0], k)


def _brute_within(ds, t):
    return sum(1 for d in ds if d <= t)


def _random_codes(rng, n, nbytes, pool=0):
    """Random codes; with ``pool`` they are drawn from that many codes with two random bits flipped (large tie classes)."""
    if not pool:
        return [rng.integers(0, 256, size=nbytes, dtype=np.uint8).tobytes() for _ in range(n)]
    base = rng.integers(0, 256, size=(pool, nbytes), dtype=np.uint8)
    out = []
    for _ in range(n):
        c = base[rng.integers(0, pool)].copy()
        for bit in rng.integers(0, 8 * nbytes, size=2):
            c[bit // 8] ^= np.uint8(1 << (bit % 8))
        out.append(c.tobytes())
    return out


@pytest.mark.parametrize("row_bytes,query_bytes,pbytes", [(8, 8, 8), (13, 13, 13), (3, 3, 3), (16, 16, 16), (20, 20, 20), (32, 32, 32),
                                                          (32, 8, 8), (32, 13, 13), (9, 32, 9)])
def test_distances_match_the_loop(row_bytes, query_bytes, pbytes):
    """Masked last words (odd byte counts) and NPHD prefixes min(len_q, len_row); bits past the prefix must not count."""
    rng = np.random.default_rng(row_bytes * 100 + query_bytes)
    rows, queries = _random_codes(rng, 37, row_bytes), _random_codes(rng, 5, query_bytes)
    queries[0] = rows[3][:query_bytes].ljust(query_bytes, b"\xff")        # a distance of zero over the prefix, all ones behind it
    max_words = (max(row_bytes, query_bytes) + 7) // 8
    got = tm.distances(_pack(rows, max_words), _pack(queries, max_words), pbytes)
    assert got.tolist() == _brute(rows, queries, pbytes)
    assert got[0, 3] == 0


def test_prefix_masks():
    assert [hex(int(m)) for m in tm.prefix_masks(13, 4)] == ["0xffffffffffffffff", "0xffffffffff000000", "0x0", "0x0"]
    assert [hex(int(m)) for m in tm.prefix_masks(8, 1)] == ["0xffffffffffffffff"]
    assert [hex(int(m)) for m in tm.prefix_masks(1, 1)] == ["0xff00000000000000"]


@pytest.mark.parametrize("pool", [0, 4])
@pytest.mark.parametrize("n,k,s0", [(50, 1, 7), (50, 5, 16), (50, 5, 50), (50, 49, 20), (50, 50, 50), (50, 80, 10), (9, 20, 9), (64, 10, 1)])
def test_floor_ceiling_and_thresholds_match_the_loop(pool, n, k, s0):
    """d_k, tau0, N, floor, ceiling and the admissible single-query counts; pool = 4 puts every cut inside a large tie class."""
    rng = np.random.default_rng(n * 1000 + k * 10 + s0 + pool)
    rows, queries = _random_codes(rng, n, 8, pool), _random_codes(rng, 3, 8, pool)
    dist = tm.distances(_pack(rows, 1), _pack(queries, 1), 8)
    brute = _brute(rows, queries, 8)
    dk = [_brute_kth(ds, k) for ds in brute]
    tau0 = [_brute_tau0(ds, k, s0) for ds in brute]
    floor = [_brute_within(ds, t) for ds, t in zip(brute, dk)]
    ceiling = [_brute_within(ds, t) for ds, t in zip(brute, tau0)]
    assert tm.kth_distance(dist, k).tolist() == dk
    assert tm.boot_thresholds(dist, k, s0).tolist() == tau0
    assert tm.floor_counts(dist, k).tolist() == floor
    assert tm.ceiling_counts(dist, k, s0).tolist() == ceiling
    assert all(f >= min(k, n) for f in floor)                     # ties at the cut only ever add rows
    assert all(f <= c for f, c in zip(floor, ceiling))
    if pool:
        assert any(f > min(k, n) for f in floor) or k >= n, "the pooled codes were to put ties at the cut"
    if s0 < min(k, n):
        assert ceiling == [n] * 3                                 # (50, 80, 10): ten rows say nothing about the 50th
    if k >= n:
        assert floor == [n] * 3 == ceiling                        # every row is wanted: nothing to cut
    case = tm.topk_case(dist, k, s0)
    assert (case.lo, case.hi) == (sum(floor), sum(ceiling))
    assert case.per_query == max(ceiling)
    if s0 == n:
        assert floor == ceiling and case.kind == "exact" and case.allowed == {sum(floor)}
    else:
        assert case.kind == "interval" and case.allowed is None
    for q in range(3):
        one = tm.topk_case(dist[q : q + 1], k, s0, pruned=True)
        expect = sorted({_brute_within(brute[q], t) for t in range(dk[q], tau0[q] + 1)})
        assert sorted(one.allowed) == expect
        assert one.kind == ("exact" if s0 == n else "one_tau")
        assert (one.lo, one.hi) == (floor[q], ceiling[q])


def test_floor_never_above_ceiling():
    rng = np.random.default_rng(99)
    for trial in range(60):
        n, nbytes = int(rng.integers(1, 90)), int(rng.integers(1, 33))
        k, s0 = int(rng.integers(1, 2 * n + 1)), int(rng.integers(1, n + 1))
        rows, queries = _random_codes(rng, n, nbytes, pool=trial % 3 * 3), _random_codes(rng, 2, nbytes)
        W = (nbytes + 7) // 8
        dist = tm.distances(_pack(rows, W), _pack(queries, W), nbytes)
        lo, hi = tm.floor_counts(dist, k), tm.ceiling_counts(dist, k, s0)
        assert (lo <= hi).all(), (n, nbytes, k, s0)
        assert (tm.boot_thresholds(dist, k, s0) >= tm.kth_distance(dist, k)).all()


def test_sample_rows():
    # the single pass: min(n, max(self_boot_rows, k, min(self_boot_per_k * k, n // 8)))
    assert tm.s0_single(40_000, 3, 256, 1024) == 3072
    assert tm.s0_single(40_000, 10, 256, 1024) == 5000
    assert tm.s0_single(40_000, 10, 65536, 1024) == 40_000
    assert tm.s0_single(100, 150, 65536, 1024) == 100
    assert tm.s0_single(1_000_000, 10, 65536, 1024) == 65536
    assert tm.s0_single(100_000_000, 512, 65536, 1024) == 512 * 1024
    assert tm.s0_single(2_000, 300, 256, 1024) == 300           # never fewer than k rows
    # the level design
    assert [tm.s0_levels(n) for n in (100, 65536, 65537, 200_001)] == [100, 65536, 65536, 65536]


def _world():
    rng = np.random.default_rng(4)
    rows, queries = _random_codes(rng, 400, 8, pool=8), _random_codes(rng, 4, 8, pool=8)
    return rows, queries, tm.distances(_pack(rows, 1), _pack(queries, 1), 8), _brute(rows, queries, 8)


def _rejects(observed, case):
    with pytest.raises(AssertionError):
        tm.check_candidates(observed, case)


def test_checker_exact():
    _, _, dist, brute = _world()
    case = tm.topk_case(dist, 5, dist.shape[1])
    want = sum(_brute_within(ds, _brute_kth(ds, 5)) for ds in brute)
    assert case.kind == "exact" and case.allowed == {want}
    tm.check_candidates(want, case)
    _rejects(want - 1, case)
    _rejects(want + 1, case)
    radius = tm.radius_case(dist, 20)
    want = sum(_brute_within(ds, 20) for ds in brute)
    tm.check_candidates(want, radius)
    _rejects(want - 1, radius)
    _rejects(want + 1, radius)
    nothing = tm.radius_case(dist, -1 + min(min(ds) for ds in brute))
    tm.check_candidates(0, nothing)
    _rejects(1, nothing)


def test_checker_interval():
    _, _, dist, brute = _world()
    case = tm.topk_case(dist, 5, 40)
    lo = sum(_brute_within(ds, _brute_kth(ds, 5)) for ds in brute)
    hi = sum(_brute_within(ds, _brute_kth(ds[:40], 5)) for ds in brute)
    assert case.kind == "interval" and lo < hi and (case.lo, case.hi) == (lo, hi)
    for observed in range(lo, hi + 1):
        tm.check_candidates(observed, case)
    _rejects(lo - 1, case)
    _rejects(hi + 1, case)


def test_checker_one_tau():
    _, _, dist, brute = _world()
    found_gap = False
    for q in range(4):
        case = tm.topk_case(dist[q : q + 1], 5, 25, pruned=True)
        dk, tau0 = _brute_kth(brute[q], 5), _brute_kth(brute[q][:25], 5)
        allowed = {_brute_within(brute[q], t) for t in range(dk, tau0 + 1)}
        assert case.kind == "one_tau" and case.allowed == allowed
        for observed in range(min(allowed) - 1, max(allowed) + 2):
            if observed in allowed:
                tm.check_candidates(observed, case)
            else:
                _rejects(observed, case)
                found_gap = found_gap or min(allowed) < observed < max(allowed)
    assert found_gap, "no case had a count between two admissible ones: the rejection inside the bounds went untested"


def test_checker_one_r():
    _, _, dist, brute = _world()
    k = 5
    worst = max(_brute_kth(ds, k) for ds in brute)
    allowed = {sum(_brute_within(ds, r) for ds in brute) for r in (worst, worst + 1, worst + 2)}
    case = tm.speculative_case(dist, k)
    assert case.kind == "one_r" and case.allowed == allowed and tm.worst_kth(dist, k) == worst
    assert len(allowed) == 3
    for observed in range(min(allowed) - 1, max(allowed) + 2):
        if observed in allowed:
            tm.check_candidates(observed, case)
        else:
            _rejects(observed, case)
    # the self-hint: every query's own threshold may end anywhere from its k-th distance to the hint
    hinted = tm.self_hint_case(dist, k)
    lo = sum(_brute_within(ds, _brute_kth(ds, k)) for ds in brute)
    assert hinted.kind == "interval" and (hinted.lo, hinted.hi) == (lo, max(allowed))
    tm.check_candidates(lo, hinted)
    tm.check_candidates(max(allowed), hinted)
    _rejects(lo - 1, hinted)
    _rejects(max(allowed) + 1, hinted)


def test_case_refuses_inconsistent_bounds():
    with pytest.raises(ValueError):
        tm.Case("interval", 5, 4, None, 1)
    with pytest.raises(ValueError):
        tm.Case("exact", 5, 6, [5], 1)
    with pytest.raises(ValueError):
        tm.one_tau_counts(np.zeros((2, 3), dtype=np.int32), 1, 1)
