"""
The cases of tests/overflow_cases.py are what they claim (numpy only, no GPU).

tests/test_gpu_overflow.py asserts that lists overflowed ("fallback_queries grew") and that a list of exactly ``cap`` rows did not.
Here the rows themselves are counted: every planted class has exactly its ``near`` rows below d, its ``tie`` rows at d and every
other row beyond d; ``near + tie`` exceeds ``cap_of(...)`` wherever the GPU file expects an overflow and equals ``cap`` / ``cap + 1`` in
the two boundary pairs; the quiet queries of a batch fit the smallest buffer.  So a GPU assertion on those counters cannot fail
for a reason other than the engine.
"""

import numpy as np
import pytest

import overflow_cases as oc
import threshold_model as tm

ALL_CASES = ([f"scan_{f}" for f in oc.SCAN_FORMS] + ["boundary"] + list(oc.RADIX_TABLES) + list(oc.SELECT_TABLES) + ["nphd_one", "nphd_two", "healthy"]
             + list(oc.DOCFREQ_TABLES))


def test_cap_of_follows_the_rule_of_the_candidate_buffer():
    assert oc.cap_of(64, 4, False) == 64 and oc.cap_of(64, 10, False) == 160          # max(candidate_cap, 16 k)
    assert oc.cap_of(64, 4, True) == 256 and oc.cap_of(64, 10, True) == 640            # ... raised to 64 k in the single pass
    assert oc.cap_of(16384, 10, True) == 16384 and oc.cap_of(16384, 700, True) == 44800
    assert oc.cap_of(oc.BOUNDARY_WIDE_CAP, oc.BOUNDARY_WIDE_K, False) == oc.BOUNDARY_WIDE_CAP == 16 * oc.BOUNDARY_WIDE_K
    assert oc.cap_of(64, 25, False) == 400 and oc.cap_of(64, 1000, False) == 16000   # the collision scans of dup_limit 25 / 1 000
    assert oc.cap_of(64, 40, False) == 640 and oc.cap_of(64, 40, True) == 2560       # a simprint request of 20 x oversampling 2


@pytest.mark.parametrize("name", ALL_CASES)
def test_every_class_is_what_it_claims(name):
    c = oc.case(name)
    rb = c.row_bytes()
    assert c.n % 64 and c.n % 128 and c.n % 192, "a row count that is a multiple of no tile"
    assert len(np.unique(c.keys, axis=0)) == c.n
    # bits past a row's length are zero
    for b in c.segments():
        assert not (c.words[rb == b] & ~tm.prefix_masks(b, c.max_words)).any()
    for h in range(len(c.hot)):
        q, qb = c.hot_query(h)
        dist = c.dist(q, qb)
        mine = [cl for cl in c.classes if cl["hot"] == h]
        for b in c.segments():
            here = [cl for cl in mine if cl["seg"] == b]
            d_seg = dist[rb == b]
            if not here:
                assert (d_seg > max(cl["d"] for cl in mine)).all()
                continue
            (cl,) = here
            d = cl["d"]
            assert ((d_seg < d).sum(), (d_seg == d).sum(), (d_seg > d).sum()) == (cl["near"], cl["tie"], len(d_seg) - cl["near"] - cl["tie"])
            assert (dist[cl["near_rows"]] < d).all() and (dist[cl["near_rows"]] >= 1).all() and (dist[cl["tie_rows"]] == d).all()
            assert cl["near"] < min(oc.KS) or not cl["near"]
            tie = c.words[cl["tie_rows"]]
            p = min(b, c.qlen(qb))
            diff = (tie ^ q) & tm.prefix_masks(p, c.max_words)
            if d > 0:
                assert len(np.unique(tie, axis=0)) == cl["tie"], "the rows at d are distinct codes"
                words = (p + 7) // 8
                if d >= words:
                    assert diff[:, :words].all(), "every compared word holds one of the flipped bits"
            else:
                assert not diff.any()


@pytest.mark.parametrize("pattern,key_words", [("small", 1), ("high", 1), ("spread", 1), ("small", 2), ("high", 2), ("spread", 2), ("one_asset", 2), ("few_assets", 2)])
def test_key_patterns(pattern, key_words):
    rng = np.random.default_rng(5)
    n = 70_001
    for hi in ((oc.TOP_BIT_ASSET, oc.ALL_ONES) if pattern == "one_asset" else (None,)):
        keys = oc.make_keys(rng, n, key_words, pattern, hi)
        assert len(np.unique(keys, axis=0)) == n
        lo = keys if key_words == 1 else keys[:, 1]
        if pattern == "high" or pattern == "one_asset":
            assert ((lo >> np.uint64(24)) == np.uint64(0xFFFFFFFFFF)).all() and ((lo & np.uint64(0xFFFFFF)) < n).all()
        if pattern == "spread":
            tops = (keys if key_words == 1 else keys[:, 0]) >> np.uint64(56)
            assert set(tops.tolist()) == {0x00, 0x7F, 0x80, 0xFF}
        if pattern == "one_asset":
            assert (keys[:, 0] == np.uint64(hi)).all() and hi >> 63 == 1
        if pattern == "few_assets":
            assert set(keys[:, 0].tolist()) == {0, 1, oc.ALL_ONES - 1, oc.ALL_ONES}
            assert np.array_equal(np.sort(keys[:, 1]), np.arange(n, dtype=np.uint64) + np.uint64(1000))


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) the scan paths
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,k,zero", oc.SCAN_BATCHES)
@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("form", list(oc.SCAN_FORMS))
def test_scan_batches_overflow_at_their_hot_queries_only(form, single, nq, k, zero):
    name = f"scan_{form}"
    c = oc.case(name)
    cap = oc.cap_of(oc.CANDIDATE_CAP, k, single)
    b = oc.scan_batch(name, nq, cap, zero)
    assert sorted(b.hot_at) == oc.hot_positions(nq) and 0 in b.hot_at and nq - 1 in b.hot_at
    sizes = {c.size_of(h) for h in b.hot_at.values()}
    assert cap + 1 in sizes, "one hot query lists one row more than the buffer holds"
    if len(b.hot_at) > 1:
        assert max(sizes) >= 4 * cap + 1, "... and one several times as many"
    for p, h in b.hot_at.items():
        cl = c.class_of(h)
        assert np.array_equal(b.q[p], c.hot[h]) and cl["near"] < k <= cl["near"] + cl["tie"], "the k-th distance of a hot query is its d"
        assert cl["near"] + cl["tie"] > cap
        assert c.listed(b.q[p], int(b.qb[p]), k)[cl["seg"]] == cl["near"] + cl["tie"]
    # every other query fits the smallest buffer in every segment, whichever valid threshold its pass starts from: the sample of
    # both designs is the whole table here (5 003 rows), so the threshold is the k-th distance itself
    for i in b.quiet():
        assert max(c.listed(b.q[i], int(b.qb[i]), k).values()) <= oc.cap_of(oc.CANDIDATE_CAP, k, False)
    assert (~b.q.any(axis=1)).sum() == (1 if zero else 0)
    if c.metric == oc.METRIC_NPHD:
        assert set(b.qb.tolist()) == {16}, "one batch per call: the retry counter counts batches"


def test_hot_positions_sit_at_both_sides_of_every_group_edge():
    assert oc.hot_positions(3) == [0, 2] and oc.hot_positions(8) == [0, 7] and oc.hot_positions(9) == [0, 7, 8]
    assert oc.hot_positions(130) == [0, 7, 8, 15, 16, 31, 32, 127, 128, 129]


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) the boundary
# ---------------------------------------------------------------------------------------------------------------------------------
def test_boundary_classes_hold_cap_and_cap_plus_one_rows_within_the_radius():
    c = oc.case("boundary")
    within = [int((c.dist(*c.hot_query(h)) <= 9).sum()) for h in range(4)]
    small, wide = oc.cap_of(oc.CANDIDATE_CAP, oc.BOUNDARY_K, False), oc.cap_of(oc.BOUNDARY_WIDE_CAP, oc.BOUNDARY_WIDE_K, False)
    assert within == [small, small + 1, wide, wide + 1] == [64, 65, 1040, 1041]
    assert oc.BOUNDARY_WIDE_K >= small + 1
    # under the wide buffer the two small classes fit as well
    assert within[1] <= wide
    b = oc.mixed_batch("boundary", 7)
    for i in b.quiet():
        assert int((c.dist(b.q[i], int(b.qb[i])) <= 9).sum()) == 0, "the radius admits nothing for the quiet neighbours"


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) the key radix of the fallback: a host restatement of its loop over the keys of the tie class
# ---------------------------------------------------------------------------------------------------------------------------------
def _radix_passes(keys, need, floor=65536):
    """Passes (key bytes fixed) the loop of ``fix_query`` runs over a tie class of ``keys`` (every row ties), and the rows it collects then."""
    kb = (keys if keys.ndim == 2 else keys[:, None]).astype(">u8").view(np.uint8).reshape(len(keys), -1)
    alive = np.ones(len(keys), dtype=bool)
    less, r, d = 0, need, 0
    tie = len(keys)
    buckets = []
    while less + tie > floor and d < kb.shape[1] and r < tie:
        hist = np.bincount(kb[alive, d], minlength=256)
        below = 0
        for digit in range(256):
            if below + hist[digit] >= r:
                break
            below += hist[digit]
        less, r, tie = less + below, r - below, int(hist[digit])
        alive &= kb[:, d] == digit
        buckets.append((digit, int((hist > 0).sum())))
        d += 1
    return buckets, less + tie


@pytest.mark.parametrize("k", [1, 10, 700, 4096])
@pytest.mark.parametrize("name", list(oc.RADIX_TABLES))
def test_radix_tables_walk_the_fallback_through_the_key_bytes_they_are_built_for(name, k):
    c = oc.case(name)
    assert c.n == oc.RADIX_ROWS > 65536 and (c.dist(*c.hot_query(0)) == 9).all(), "every row ties at d = 9"
    # (k = 4 096 is the range-limited search of radius 9, whose buffer is never raised to 64 k)
    for single in (False, True) if k < 4096 else (False,):
        assert c.n > oc.cap_of(oc.CANDIDATE_CAP, k, single)
    buckets, collected = _radix_passes(c.keys, k)
    if c.key_words == 1:
        # passes d = 0 .. 5; five of them through the single bucket 0xFF
        assert buckets == [(255, 1)] * 5 + [(0, 2)]
    else:
        # passes d = 0 .. 13; eight through the one asset, five through 0xFF; the cut bucket lies in the LOW word
        asset = int(c.keys[0, 0])
        assert buckets == [((asset >> (56 - 8 * d)) & 255, 1) for d in range(8)] + [(255, 1)] * 5 + [(0, 2)]
    assert collected == 65536
    b = oc.mixed_batch(name, 3)
    assert b.hot_at == {0: 0}


# ---------------------------------------------------------------------------------------------------------------------------------
# (d) the select's own radix without an overflow
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(oc.SELECT_TABLES))
def test_select_tables_tie_beyond_the_sort_buffer_and_inside_the_default_candidate_buffer(name):
    c = oc.case(name)
    assert c.size_of(0) == 3003 > 2048 and c.n <= 16384, "less + tie exceeds the sort buffer of k = 10 (1 024) and k = 257 (2 048), never the default buffer"


# ---------------------------------------------------------------------------------------------------------------------------------
# (e) several segments
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,segs", [("nphd_one", (16,)), ("nphd_two", (16, 32))])
def test_nphd_tables_overflow_in_the_named_segments_only(name, segs):
    c = oc.case(name)
    assert c.segments() == [8, 16, 32] and sorted(c.hot_bytes.tolist()) == [8, 16, 32]
    for h in range(3):
        q, qb = c.hot_query(h)
        for k, single, radius in ((4, False, None), (4, True, None), (10, False, 9)):
            cap = oc.cap_of(oc.CANDIDATE_CAP, k, single)
            d, rb = c.dist(q, qb), c.row_bytes()
            for b in (8, 16, 32):
                rows = int((d[rb == b] <= 9).sum()) if radius is not None else c.listed(q, qb, k)[b]
                assert (rows > cap) == (b in segs), (h, k, b, rows, cap)
                if b in segs:
                    assert rows == c.size_of(h, b) == 300
    for nq in (3, 9):
        b = oc.mixed_batch(name, nq)
        assert sorted(b.hot_at.values()) == [0, 1, 2] and 0 in b.hot_at and nq - 1 in b.hot_at
        for i in b.quiet():
            assert max(c.listed(b.q[i], int(b.qb[i]), 4).values()) <= 64 and int((c.dist(b.q[i], int(b.qb[i])) <= 9).sum()) <= 64


# ---------------------------------------------------------------------------------------------------------------------------------
# (f) the halves of the asynchronous search
# ---------------------------------------------------------------------------------------------------------------------------------
def test_halves_of_the_two_word_table_overflow_for_the_large_classes_only():
    c = oc.case("scan_b16k2")
    (ka, wa), (kb, wb) = oc.halves(c)
    assert len(ka) + len(kb) == c.n
    for k, single in ((4, False), (4, True)):
        cap = oc.cap_of(oc.CANDIDATE_CAP, k, single)
        flagged = oc.async_flagged(c, k, cap)
        assert flagged and len(flagged) < len(c.hot), "some hot queries overflow a half, some fit both"
    assert oc.async_flagged(c, 4, 64) == {h for h in range(len(c.hot)) if c.size_of(h) >= 161}


# ---------------------------------------------------------------------------------------------------------------------------------
# (g) document frequency
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(oc.DOCFREQ_TABLES))
def test_docfreq_tables_collide_beyond_the_buffer_of_their_dup_limit(name):
    c = oc.case(name)
    dup_limit = oc.DOCFREQ_LIMIT[name]
    q, _ = c.hot_query(0)
    equal = int((c.words == q).all(axis=1).sum())
    assert equal == c.size_of(0) > oc.cap_of(oc.CANDIDATE_CAP, dup_limit, False)
    freq, rows = oc.doc_freq_of(c, q, dup_limit)
    assert rows == dup_limit
    # few_assets: a rare asset or two lie wholly inside the first dup_limit rows and another fills them -- the count is no trivial 1
    assert freq == 1 if "ones" in name else 2 <= freq <= 3


# ---------------------------------------------------------------------------------------------------------------------------------
# (f) the range-limited requests of search_many and search_device over the two-word table
# ---------------------------------------------------------------------------------------------------------------------------------
def test_range_limited_requests_over_the_scan_table_overflow_by_the_rows_within_their_radius():
    """k = 10, radius 9: cap = 160.  What a range-limited pass lists is every row within the radius, whatever the k-th distance is."""
    c = oc.case("scan_b16k2")
    cap = oc.cap_of(oc.CANDIDATE_CAP, 10, False)
    b = oc.scan_batch("scan_b16k2", 3, cap)
    assert cap == 160 and b.hot_at
    for p, h in b.hot_at.items():
        within = int((c.dist(b.q[p], int(b.qb[p])) <= 9).sum())
        assert within == c.size_of(h) > cap, "also for a class of equal codes: no other row lies within the radius"
    for i in b.quiet():
        assert int((c.dist(b.q[i], int(b.qb[i])) <= 9).sum()) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# (h) the simprint corpora
# ---------------------------------------------------------------------------------------------------------------------------------
CAP_LEVELS, CAP_SINGLE = oc.cap_of(oc.CANDIDATE_CAP, oc.SIMPRINT_COUNT, False), oc.cap_of(oc.CANDIDATE_CAP, oc.SIMPRINT_COUNT, True)


@pytest.mark.parametrize("kind", list(oc.SIMPRINT_CORPORA))
def test_hot_simprints_list_more_rows_than_either_buffer_within_their_40th_distance(kind):
    s = oc.simprint_corpus(kind)
    assert (CAP_LEVELS, CAP_SINGLE) == (640, 2560) and oc.SIMPRINT_COUNT == 40 < oc.SIMPRINT_DUP_LIMIT
    assert len(s.keys) % 64 and s.h_max() >= oc.HOT_FLIPS, "chunks at distance 5 pass the match threshold"
    assert {s.keys[i][:8] for i in range(len(s.keys))} >= {b"\x00" * 8, b"\xff" * 8}, "the asset ids 0 and all ones"
    for hot, (equal, away) in zip(s.hot, s.hot_plan):
        dist = s.dist(hot)
        assert ((dist == 0).sum(), (dist == oc.HOT_FLIPS).sum()) == (equal, away)
        assert ((dist > 0) & (dist <= max(s.h_max(), oc.HOT_FLIPS)) & (dist != oc.HOT_FLIPS)).sum() == 0, "no other chunk within the match threshold"
        if away:
            assert len(np.unique(s.vecs[dist == oc.HOT_FLIPS], axis=0)) == away, "the chunks at distance 5 hold distinct simprints"
        # the 40th distance d, the rows below it and at it
        d = int(np.sort(dist)[oc.SIMPRINT_COUNT - 1])
        less, tie = int((dist < d).sum()), int((dist == d).sum())
        assert d == (0 if equal >= oc.SIMPRINT_COUNT else oc.HOT_FLIPS)
        assert (less, tie, int((dist > d).sum())) == ((0, equal, len(dist) - equal) if d == 0 else (equal, away, len(dist) - equal - away))
        assert less < oc.SIMPRINT_COUNT <= less + tie and less + tie > CAP_SINGLE > CAP_LEVELS, "both passes overflow"


@pytest.mark.parametrize("kind", [64, 128, 256])
def test_requests_of_the_two_hot_corpora(kind):
    s = oc.simprint_corpus(kind)
    a, b = s.hot
    equal_a, equal_b = int((s.dist(a) == 0).sum()), int((s.dist(b) == 0).sum())
    # the first hot simprint's whole list lies at distance 0 and 40 < dup_limit: its own frequency is asked of the collision scan, which fits
    assert equal_a == 2700 >= oc.SIMPRINT_COUNT and equal_a <= oc.cap_of(oc.CANDIDATE_CAP, oc.SIMPRINT_DUP_LIMIT, False) == 16000
    # hard-boundary lookups: dup_limit 25 -> cap 400 < 2 700, and no other lookup of either list comes near it; dup_limit 1 000 -> every list fits
    assert equal_a > oc.cap_of(oc.CANDIDATE_CAP, 25, False) == 400 >= equal_b == 30
    for request in s.raw_requests():
        assert request.count(a) == 1 and request.count(b) == 1 and len(request) == 32
    assert {s.raw_requests()[0].index(a), s.raw_requests()[1].index(a), s.raw_requests()[2].index(a)} == {0, 31, 15}
    many = s.many_requests()
    assert sum(r.count(a) + r.count(b) for r in many) == 3 and sum(len(r) for r in many) <= oc.LOOKUPS_PER_BATCH
    for form, several in (("one batch", False), ("two batches", True)):
        given = s.exact_given(form)
        distinct = list(dict.fromkeys(given))
        assert (len(distinct) > oc.LOOKUPS_PER_BATCH) == several and given.count(a) == 2 and a in distinct and b in distinct
        assert max(int((s.dist(sp) == 0).sum()) for sp in distinct if sp != a) <= 400, "exactly one lookup outgrows the buffer of dup_limit 25"


def test_requests_of_the_big_corpus():
    s = oc.simprint_corpus("big")
    (hot,) = s.hot
    equal = int((s.dist(hot) == 0).sum())
    scan_cap = oc.cap_of(oc.CANDIDATE_CAP, oc.SIMPRINT_DUP_LIMIT, False)
    assert equal == 17003 > scan_cap == 16000, "the collision scan behind the unknown frequency overflows, and so does the lookup of dup_limit 1 000"
    (request,) = s.raw_requests()
    assert request.count(hot) == 1
    given = s.exact_given("one batch")
    distinct = list(dict.fromkeys(given))
    assert len(distinct) <= oc.LOOKUPS_PER_BATCH and given.count(hot) == 2
    assert max(int((s.dist(sp) == 0).sum()) for sp in distinct if sp != hot) <= scan_cap
    # the first 1 000 equal rows by ascending key hold five chunks of each of 200 assets
    first = sorted(k for k, d in zip(s.keys, s.dist(hot)) if d == 0)[: oc.SIMPRINT_DUP_LIMIT]
    assert len({k[:8] for k in first}) == 200
