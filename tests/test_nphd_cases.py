"""
tests/nphd_cases.py held to the oracle and to its own claims (no GPU): the exact model equals ``oracle_topk`` and ``np_within`` on
the constructed tables, the sweep table is the arithmetic it is said to be, the clustered table's lists interleave the code lengths,
and the hint scenarios end where the rule of the ratio speculation changes its verdict.
"""

from fractions import Fraction

import numpy as np
import pytest

import nphd_cases as nc
from oracle import np_within, oracle_topk

NAMES = ("keys", "hamming", "prefix_bits", "count")
METRIC_NPHD = 1


def _same(got, exp, what):
    for g, e, name in zip(got, exp, NAMES):
        np.testing.assert_array_equal(g, e, err_msg=f"{what}: {name}")


def test_model_rank_orders_as_the_fractions_do():
    pairs = [(p, h) for p in range(1, 33) for h in range(8 * p + 1)]
    by_rank = sorted(pairs, key=lambda ph: nc.model_rank(*ph))
    for (p0, h0), (p1, h1) in zip(by_rank, by_rank[1:]):
        f0, f1, r0, r1 = Fraction(h0, 8 * p0), Fraction(h1, 8 * p1), nc.model_rank(p0, h0), nc.model_rank(p1, h1)
        assert (f0 == f1 and r0 == r1) or (f0 < f1 and r1 == r0 + 1), ((p0, h0), (p1, h1))
    assert nc.model_rank(1, 0) == nc.model_rank(32, 0) == 0
    assert nc.model_rank(3, 3) == nc.model_rank(8, 8) == nc.model_rank(13, 13) == nc.model_rank(32, 32)      # 1/8 at every length
    assert nc.model_rank(32, 256) == nc.model_rank(1, 8) == len({Fraction(h, 8 * p) for p, h in pairs}) - 1
    with pytest.raises(ValueError):
        nc.model_rank(3, 25)


@pytest.mark.parametrize("key_words", [1, 2])
def test_sweep_table_is_the_arithmetic_it_claims(key_words):
    sw = nc.sweep_table(key_words)
    n = len(sw.lens)
    assert n == nc.SWEEP_ROWS == 2144 and sorted(set(sw.lens.tolist())) == list(range(1, 33))
    assert sorted(zip(sw.p.tolist(), sw.h.tolist())) == [(p, h) for p in range(1, 33) for h in range(4 * p + 1)]
    np.testing.assert_array_equal(sw.lens, sw.p)
    rows = nc.to_bytes(sw.words)
    assert all(not rows[i, sw.p[i]:].any() for i in range(n)), "bits beyond a row's length"
    # against Q, row (p, h) is at distance h over 8p bits; against ~Q at 8p - h
    h, p = nc.prefix_distances(sw.words, sw.lens, sw.Q, 32)
    np.testing.assert_array_equal(h, sw.h)
    np.testing.assert_array_equal(p, sw.p)
    h_inv, _ = nc.prefix_distances(sw.words, sw.lens, ~sw.Q, 32)
    np.testing.assert_array_equal(h_inv, 8 * sw.p - sw.h)
    # Q reaches the lower half of every row of the rank table, ~Q the upper half
    assert {(int(a), int(b)) for a, b in zip(p, h)} | {(int(a), int(b)) for a, b in zip(p, h_inv)} == {(q, x) for q in range(1, 33) for x in range(8 * q + 1)}
    # ratio < 1/8 is h < p: 528 rows; ratio == 1/8 is one row per length: k = 544 cuts that class in the middle, by key alone
    ratio = [Fraction(int(a), 8 * int(b)) for a, b in zip(sw.h, sw.p)]
    below = [i for i in range(n) if ratio[i] < Fraction(1, 8)]
    at = [i for i in range(n) if ratio[i] == Fraction(1, 8)]
    assert len(below) == 528 == sum(range(1, 33)) and all(sw.h[i] < sw.p[i] for i in below)
    assert sorted(int(sw.p[i]) for i in at) == list(range(1, 33))
    top = nc.model_topk(sw.keys, sw.words, sw.lens, nc.to_words(sw.Q[None, :]), 32, 544)
    assert top[3][0] == 544 and all(Fraction(int(a), int(b)) == Fraction(1, 8) for a, b in zip(top[1][0, 528:], top[2][0, 528:]))
    ints = nc.keys_as_ints(sw.keys)
    assert nc.keys_as_ints(top[0][0, 528:]) == sorted(ints[i] for i in at)[:16]
    assert len(set((top[2][0, 528:] // 8).tolist())) > 8, "the kept half of the class spans many lengths"
    # the keys: distinct, unrelated to (p, h), both ends of the range
    lo = np.asarray(sw.keys).reshape(n, -1)[:, -1]
    assert len(set(ints)) == n and lo.min() == 0 and lo.max() == np.uint64(0xFFFFFFFFFFFFFFFF)
    assert (lo >= np.uint64(1 << 63)).sum() > n // 3 and abs(np.corrcoef(lo.astype(np.float64), np.array([float(r) for r in ratio]))[0, 1]) < 0.1
    if key_words == 2:
        hi = np.asarray(sw.keys)[:, 0]
        assert len(np.unique(hi)) == 4 and min(np.unique(hi, return_counts=True)[1]) > 400, "a hi word is shared by many rows"


@pytest.mark.parametrize("key_words", [1, 2])
@pytest.mark.parametrize("k", [1, 544, 2144])
def test_model_equals_the_oracle_on_the_sweep_table(key_words, k):
    sw = nc.sweep_table(key_words)
    q, ql = nc.sweep_queries(sw.Q)
    assert ql.tolist() == [32, 32, 4, 8, 13, 16, 24, 32, 32]
    _same(nc.model_topk(sw.keys, sw.words, sw.lens, q, ql, k), oracle_topk(METRIC_NPHD, sw.keys, sw.words, sw.lens, q, ql, k), f"sweep k={k}")
    for nbytes in (32, 13):
        q, ql = nc.sweep_queries_many(sw.Q, 20, nbytes)
        _same(nc.model_topk(sw.keys, sw.words, sw.lens, q, ql, k), oracle_topk(METRIC_NPHD, sw.keys, sw.words, sw.lens, q, ql, k), f"sweep x20 k={k}")


@pytest.mark.parametrize("key_words", [1, 2])
def test_model_equals_the_oracle_on_the_clustered_table(key_words):
    t = nc.clustered_table(key_words)
    assert {int(b): int((t.lens == b).sum()) for b in nc.CLUSTER_LENGTHS} == {b: 2500 for b in nc.CLUSTER_LENGTHS}
    q, ql = nc.clustered_queries(t, 60)
    assert set(ql.tolist()) == set(nc.CLUSTER_QUERY_LENGTHS)
    for k in (10, 100):
        _same(nc.model_topk(t.keys, t.words, t.lens, q, ql, k), oracle_topk(METRIC_NPHD, t.keys, t.words, t.lens, q, ql, k), f"clustered k={k}")


@pytest.mark.parametrize("radius", [0, 3, 256])
def test_model_equals_np_within(radius):
    for name, t, (q, ql) in (("sweep", nc.sweep_table(2), nc.sweep_queries(nc.sweep_table(2).Q)),
                             ("clustered", nc.clustered_table(1), nc.clustered_queries(nc.clustered_table(1), 24))):
        k = 300
        got = nc.model_topk(t.keys, t.words, t.lens, q, ql, k, radius=radius)
        for i in range(len(ql)):
            ek, eh, ep = np_within(t.words, t.lens, t.keys, q[i], int(ql[i]), k, radius)
            c = int(got[3][i])
            assert c == len(eh), f"{name} radius {radius} query {i}: count"
            np.testing.assert_array_equal(got[0][i, :c], ek, err_msg=f"{name} radius {radius} query {i}: keys")
            np.testing.assert_array_equal(got[1][i, :c], eh, err_msg=f"{name} radius {radius} query {i}: hamming")
            np.testing.assert_array_equal(got[2][i, :c], ep, err_msg=f"{name} radius {radius} query {i}: prefix_bits")
            assert not got[1][i, c:].any() and not got[2][i, c:].any()
        if radius == 256:
            assert (got[3] == k).all()
        if radius == 0 and name == "sweep":
            assert got[3][0] == 32 and got[3][1] == 0     # Q: the row h = 0 of every length; ~Q: none


@pytest.mark.parametrize("nq", [60, 200])
@pytest.mark.parametrize("k", [10, 100])
def test_clustered_lists_interleave_the_lengths(nq, k):
    """Conditions on the INPUTS (the model's own lists), which the GPU tests rely on; a builder that misses them is to be changed."""
    t = nc.clustered_table(1)
    q, ql = nc.clustered_queries(t, nq)
    keys, ham, pbits, cnt = nc.model_topk(t.keys, t.words, t.lens, q, ql, k + 1)
    assert (cnt == k + 1).all()
    # a query of b bytes meets the compared prefixes min(b, row bytes): two for 4 bytes, three for 8 and 13, four or more from 16 on.
    # Every query that can holds rows of at least 4 distinct prefix lengths in its k nearest.
    for i in range(nq):
        reachable = len({min(int(ql[i]), b) for b in nc.CLUSTER_LENGTHS})
        if reachable >= 4:
            assert len(set(pbits[i, :k].tolist())) >= 4, f"query {i} of {ql[i]} bytes: prefixes {sorted(set(pbits[i, :k].tolist()))}"
    assert sum(1 for b in ql if b >= 16) >= nq * 3 // 4
    assert (pbits[:, :k] >= 128).mean() >= 0.25
    tied = [i for i in range(nq) if Fraction(int(ham[i, k - 1]), int(pbits[i, k - 1])) == Fraction(int(ham[i, k]), int(pbits[i, k])) and pbits[i, k - 1] != pbits[i, k]]
    assert tied, "no query whose k-th and (k + 1)-th rows tie across two prefix lengths"


@pytest.mark.parametrize("qlen", [32, 13])
@pytest.mark.parametrize("m", [1, 5, 160])
def test_hint_scenarios_are_what_they_claim(qlen, m):
    """Every step's planted row IS its probe's k-th row, at the fraction the label names, and the rule gives the verdict listed."""
    sc = nc.hint_scenario(qlen)
    model = nc.MHintModel(sc.keys, sc.words, sc.lens)
    for i, ((label, probe, k, verdict), (_, _, row_bytes, h, _)) in enumerate(zip(sc.steps, nc.SCENARIO_STEPS[qlen])):
        q = nc.scenario_batch(sc, i, m)
        assert q.shape == (m, 4)
        kth = nc.kth_ratios(nc.model_topk(sc.keys, sc.words, sc.lens, q, qlen, k), k)
        if probe is not None:
            assert kth[-1] == Fraction(h, 8 * min(row_bytes, qlen)) == max(kth), label
        else:
            assert max(kth) < Fraction(1, 32), label
        before = model.hint(m, qlen).ratio
        assert model.step(q, qlen, k) == verdict, f"{label} (hint {before}, worst {max(kth)})"


def test_hint_model_backs_off_after_misses_in_a_row():
    """Two misses in a row: the next two batches of the class do not speculate (and re-seed); another class is untouched."""
    sc = nc.hint_scenario(32)
    model = nc.MHintModel(sc.keys, sc.words, sc.lens)
    far = [nc.scenario_batch(sc, i, 1) for i, s in enumerate(nc.SCENARIO_STEPS[32]) if s[1] == 10 and s[2] is not None]
    near = nc.scenario_batch(sc, 5, 1)
    assert model.step(near, 32, 10) == (0, 0)           # seeds near 0
    assert model.step(far[0], 32, 10) == (0, 1)         # 12/256 beyond it: miss, re-seeded
    assert model.step(far[4], 32, 10) == (0, 1)         # 41/256 > 12/256 + 8/256: the second miss in a row
    assert model.step(far[4], 32, 10) == (0, 0) and model.step(far[4], 32, 10) == (0, 0)
    assert model.step(far[4], 32, 10) == (1, 0)
    assert model.step(nc.scenario_batch(sc, 5, 5), 32, 10) == (0, 0)
