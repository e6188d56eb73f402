"""
The helpers of ``tests/device_lists.py`` checked without a GPU: ``reference_merge`` against a plain ``sorted()``, the shape of
what ``make_lists`` and ``pack`` produce, and ``check_record_order`` on one good list and on lists it must reject.
"""

import numpy as np
import pytest

from device_lists import (
    POISON_PAYLOAD, SPLIT_GAP, check_record_order, make_lists, mixed_counts, pack, reference_merge, valid_counts,
)
from iscc_search_amd._lib import COUNT_OVERFLOW, RECORD_DTYPE
from iscc_search_amd.sharded import block_bytes


def _sorted_merge(lists, counts, q, k):
    """One query by Python's stable sort: [(key_hi, key_lo, hamming, prefix_bits)]."""
    rows = []
    for l in range(lists.shape[0]):
        for i in range(min(int(counts[l, q]), k)):
            r = lists[l, q, i]
            rows.append((int(r["dist_rank"]), int(r["key_hi"]), int(r["key_lo"]), l, int(r["hamming"]), int(r["prefix_bits"])))
    rows = sorted(rows, key=lambda r: r[:4])[:k]
    return [(r[1], r[2], r[4], r[5]) for r in rows]


@pytest.mark.parametrize("n_lists,nq,k,key_words", [(1, 3, 4, 1), (2, 5, 3, 2), (3, 4, 7, 1), (5, 6, 2, 2), (4, 2, 1, 1)])
def test_reference_merge_equals_sorted(n_lists, nq, k, key_words):
    rng = np.random.default_rng(n_lists * 100 + k)
    counts = mixed_counts(rng, n_lists, nq, k)
    counts[0, 0] = k + 5                                   # a raw count above k is clamped
    lists = make_lists(rng, n_lists, nq, k, key_words, counts)
    keys, ham, pbits, cnt = reference_merge(lists, counts, k, key_words)
    for q in range(nq):
        want = _sorted_merge(lists, counts, q, k)
        c = int(cnt[q])
        assert c == len(want) == min(k, int(valid_counts(counts, k)[:, q].sum()))
        got_keys = [(int(a), int(b)) for a, b in keys[q, :c]] if key_words == 2 else [(0, int(a)) for a in keys[q, :c]]
        assert got_keys == [(w[0], w[1]) for w in want]
        assert ham[q, :c].tolist() == [w[2] for w in want] and pbits[q, :c].tolist() == [w[3] for w in want]
        assert not keys[q, c:].any() and not ham[q, c:].any() and not pbits[q, c:].any()


def test_reference_merge_puts_the_lower_list_first_on_an_exact_tie_and_passes_the_overflow_marker_on():
    rng = np.random.default_rng(5)
    counts = np.full((3, 2), 4, dtype=np.uint32)
    lists = make_lists(rng, 3, 2, 4, 2, counts)
    lists["dist_rank"][0, 0, 0] = 0                        # list 0's head is the query's first record ...
    twin = lists[0, 0, 0].copy()
    twin["hamming"] = 4242
    lists[2, 0, 0] = twin                                  # ... and list 2's head has the same (rank, key) with another payload
    keys, ham, _, cnt = reference_merge(lists, counts, 4, 2)
    want = _sorted_merge(lists, counts, 0, 4)
    assert ham[0].tolist() == [w[2] for w in want]
    assert ham[0, :2].tolist() == [int(lists[0, 0, 0]["hamming"]), 4242] and (keys[0, 0] == keys[0, 1]).all()
    counts[1, 1] = COUNT_OVERFLOW
    keys, ham, pbits, cnt = reference_merge(lists, counts, 4, 2)
    assert cnt.tolist() == [4, COUNT_OVERFLOW] and not keys[1].any() and not ham[1].any() and not pbits[1].any()


@pytest.mark.parametrize("key_words", [1, 2])
def test_make_lists_are_sorted_key_distinct_and_poisoned_past_the_count(key_words):
    rng = np.random.default_rng(11)
    n_lists, nq, k = 4, 6, 9
    counts = mixed_counts(rng, n_lists, nq, k)
    counts[1, 2], counts[2, 3] = 0xFFFFFFFE, k + 5
    lists = make_lists(rng, n_lists, nq, k, key_words, counts)
    assert lists.dtype == RECORD_DTYPE and lists.shape == (n_lists, nq, k)
    valid = valid_counts(counts, k)
    assert valid[1, 2] == k and valid[2, 3] == k
    for q in range(nq):
        seen = set()
        for l in range(n_lists):
            n = int(valid[l, q])
            head, tail = lists[l, q, :n], lists[l, q, n:]
            rows = [(int(r["dist_rank"]), int(r["key_hi"]), int(r["key_lo"])) for r in head]
            assert rows == sorted(rows)
            keys = {r[1:] for r in rows}
            assert len(keys) == n and not (keys & seen) and (0, 0) not in keys
            seen |= keys
            if key_words == 1:
                assert not head["key_hi"].any()
            assert not tail["dist_rank"].any() and not tail["key_hi"].any() and not tail["key_lo"].any()
            assert (tail["hamming"] == POISON_PAYLOAD).all() and (tail["prefix_bits"] == POISON_PAYLOAD).all()
    # a small alphabet of ranks: the key decides most of the order
    assert 3 <= len(np.unique(np.concatenate([lists[l, q, : valid[l, q]]["dist_rank"] for l in range(n_lists) for q in range(nq)]))) <= 5


def test_pack_lays_out_blocks_and_split():
    rng = np.random.default_rng(2)
    n_lists, nq, k = 3, 5, 4
    counts = mixed_counts(rng, n_lists, nq, k)
    lists = make_lists(rng, n_lists, nq, k, 2, counts)
    rec_bytes, blk = block_bytes(nq, k)
    buf, rec_off, cnt_off, ls, cs = pack(lists, counts, "blocks")
    assert (rec_off, cnt_off, ls, cs, buf.size) == (0, rec_bytes, blk, blk, n_lists * blk)
    buf2, rec_off2, cnt_off2, ls2, cs2 = pack(lists, counts, "split")
    assert (ls2, cs2) == (rec_bytes + SPLIT_GAP, nq * 4) and ls2 != cs2 and ls2 % 8 == 0 and cnt_off2 == n_lists * ls2
    for b, ro, co, s, c in ((buf, rec_off, cnt_off, ls, cs), (buf2, rec_off2, cnt_off2, ls2, cs2)):
        for l in range(n_lists):
            np.testing.assert_array_equal(b[ro + l * s : ro + l * s + rec_bytes].view(RECORD_DTYPE).reshape(nq, k), lists[l])
            np.testing.assert_array_equal(b[co + l * c : co + l * c + nq * 4].view(np.uint32), counts[l])
    for l in range(n_lists):
        assert (buf2[l * ls2 + rec_bytes : (l + 1) * ls2] == 0xFF).all()          # the gaps
        assert (buf[l * blk + rec_bytes + nq * 4 : (l + 1) * blk] == 0xFF).all()  # the pad
    with pytest.raises(ValueError):
        pack(lists, counts, "rows")


def _nphd_records():
    """Six records in NPHD order: 0/64 = 0/32 < 1/64 < 1/32 = 2/64 < 3/32 (equal fractions share a rank, the key decides)."""
    rows = [(0, 64, 0, 5), (0, 32, 0, 9), (1, 64, 1, 2), (1, 32, 2, 1), (2, 64, 2, 8), (3, 32, 3, 4)]
    rec = np.zeros(len(rows), dtype=RECORD_DTYPE)
    for i, (h, p, rank, key) in enumerate(rows):
        rec[i] = (0, key, rank, h, p)
    return rec


def test_check_record_order_accepts_a_good_list():
    rec = _nphd_records()
    check_record_order(rec, len(rec), 1)
    check_record_order(rec, 0, 1)
    ham = np.zeros(4, dtype=RECORD_DTYPE)                  # a Hamming table: constant prefix, rank in the order of hamming
    ham["key_hi"], ham["key_lo"], ham["dist_rank"], ham["hamming"], ham["prefix_bits"] = [1, 1, 2, 2], [3, 4, 1, 2], [0, 0, 5, 9], [0, 0, 5, 9], 64
    check_record_order(ham, 4, 2)


def test_check_record_order_rejects_swapped_records_and_wrong_ranks():
    rec = _nphd_records()
    swapped = rec.copy()
    swapped[[2, 3]] = swapped[[3, 2]]                      # two records in the wrong order
    with pytest.raises(AssertionError, match="strictly ascending"):
        check_record_order(swapped, len(swapped), 1)
    check_record_order(swapped, 2, 1)                      # ... beyond the count: not looked at
    same_key = rec.copy()
    same_key["key_lo"][1] = same_key["key_lo"][0]          # equal (rank, key): not STRICTLY ascending
    with pytest.raises(AssertionError, match="strictly ascending"):
        check_record_order(same_key, len(same_key), 1)
    wrong_rank = rec.copy()
    wrong_rank["dist_rank"][4] = 3                         # 2/64 ranked above 1/32: ascending, but equal fractions share a rank
    wrong_rank["dist_rank"][5] = 4
    with pytest.raises(AssertionError, match="does not order as hamming / prefix_bits"):
        check_record_order(wrong_rank, len(wrong_rank), 1)
    by_hamming = rec.copy()                                # ranks that follow hamming alone, ignoring the prefix
    by_hamming["dist_rank"] = by_hamming["hamming"]
    by_hamming = by_hamming[np.lexsort((by_hamming["key_lo"], by_hamming["dist_rank"]))]
    with pytest.raises(AssertionError, match="does not order as hamming / prefix_bits"):
        check_record_order(by_hamming, len(by_hamming), 1)
    with pytest.raises(AssertionError, match="key_hi"):
        hi = rec.copy()
        hi["key_hi"][5] = 1
        check_record_order(hi, len(hi), 1)
