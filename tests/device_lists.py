"""
Synthetic ``Record`` lists and a host reference of their merge (TEST INFRASTRUCTURE).

``merge_kernel`` ranks every record of every list by binary search into the other lists; the device searches leave such lists in
caller-owned memory.  The helpers here build lists whose order is decided by every field the kernel compares, lay them out in
device memory the two ways callers do, restate the merge with ``np.lexsort`` and check raw records read back from the device.
Importable without a GPU (``upload`` alone needs torch and a device); checked by ``tests/test_device_lists_reference.py``.
"""

import numpy as np

from iscc_search_amd._lib import COUNT_OVERFLOW, RECORD_DTYPE
from iscc_search_amd.sharded import block_bytes

RECORD_BYTES = RECORD_DTYPE.itemsize
POISON_PAYLOAD = 0xFFFF
SPLIT_GAP = 64                      # bytes of 0xFF behind every record block of the "split" layout
RANK_ALPHABET = np.array([2, 7, 40, 41, 1000], dtype=np.uint32)
KEY_HI_ALPHABET = np.array([1, 2, 3, 1 << 40, (1 << 64) - 1], dtype=np.uint64)


def valid_counts(counts, k):
    """Records a list really holds per query: a raw count is clamped to k (``count_of`` in merge_kernel; COUNT_OVERFLOW too)."""
    return np.minimum(np.asarray(counts, dtype=np.uint64), np.uint64(k)).astype(np.int64)


def mixed_counts(rng, n_lists, nq, k):
    """Counts per (list, query) drawn from {0, 1, k - 1, k}."""
    return rng.choice(np.array([0, 1, max(k - 1, 0), k], dtype=np.uint32), size=(n_lists, nq)).astype(np.uint32)


def record_order(rec):
    """Indices that stable-sort a 1-D record array by (dist_rank, key_hi, key_lo)."""
    return np.lexsort((rec["key_lo"], rec["key_hi"], rec["dist_rank"]))


def make_lists(rng, n_lists, nq, k, key_words, counts, n_ranks=4):
    # type: (np.random.Generator, int, int, int, int, np.ndarray, int) -> np.ndarray
    """
    Host lists [n_lists][nq][k] of ``RECORD_DTYPE``.  Per (list, query) the first min(count, k) records are sorted by
    (dist_rank, key_hi, key_lo) with keys distinct across all lists of the query; ``dist_rank`` comes from ``n_ranks`` (3..5)
    values and, with 128-bit keys, ``key_hi`` from a handful, so that every field decides often; ``hamming`` / ``prefix_bits`` are a
    payload independent of the order.  Every record past the count is poison: rank 0, key 0, payload 0xFFFF -- a reader that
    goes beyond a list's count puts it at the head of its answer.
    """
    if not 3 <= n_ranks <= len(RANK_ALPHABET):
        raise ValueError("n_ranks must be 3..5")
    counts = np.asarray(counts, dtype=np.uint32)
    if counts.shape != (n_lists, nq):
        raise ValueError("counts must be shaped [n_lists][nq]")
    valid = valid_counts(counts, k)
    lists = np.zeros((n_lists, nq, k), dtype=RECORD_DTYPE)
    lists["hamming"] = POISON_PAYLOAD
    lists["prefix_bits"] = POISON_PAYLOAD
    for q in range(nq):
        total = int(valid[:, q].sum())
        # distinct, non-zero (zero is the poison key), spread over all 64 bits
        key_lo = (rng.permutation(3 * total + 1)[:total].astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        at = 0
        for l in range(n_lists):
            n = int(valid[l, q])
            rec = np.zeros(n, dtype=RECORD_DTYPE)
            rec["key_lo"] = key_lo[at : at + n]
            if key_words == 2:
                rec["key_hi"] = rng.choice(KEY_HI_ALPHABET, size=n)
            rec["dist_rank"] = rng.choice(RANK_ALPHABET[:n_ranks], size=n)
            rec["hamming"] = rng.integers(0, 1000, size=n)
            rec["prefix_bits"] = rng.integers(1, 1000, size=n)
            lists[l, q, :n] = rec[record_order(rec)]
            at += n
    return lists


def pack(lists, counts, layout):
    # type: (np.ndarray, np.ndarray, str) -> tuple
    """
    The bytes of ``lists`` / ``counts`` as they lie in device memory: (bytes uint8, record offset, count offset, list stride,
    count stride).  ``"blocks"``: one {records | counts | pad} block per list (``block_bytes``), both strides the block size.
    ``"split"``: every record block followed by a gap, the count arrays packed behind them all -- the strides differ.
    Everything that is neither record nor count is 0xFF.
    """
    n_lists, nq, k = lists.shape
    counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(n_lists, nq)
    rec_bytes, blk = block_bytes(nq, k)
    if layout == "blocks":
        list_stride = count_stride = blk
        rec_off, cnt_off = 0, rec_bytes
        size = n_lists * blk
    elif layout == "split":
        list_stride, count_stride = rec_bytes + SPLIT_GAP, nq * 4
        rec_off, cnt_off = 0, n_lists * list_stride
        size = cnt_off + n_lists * count_stride
    else:
        raise ValueError(f"unknown layout {layout!r}")
    buf = np.full(size, 0xFF, dtype=np.uint8)
    for l in range(n_lists):
        a = rec_off + l * list_stride
        buf[a : a + rec_bytes] = np.ascontiguousarray(lists[l]).view(np.uint8).reshape(-1)
        c = cnt_off + l * count_stride
        buf[c : c + nq * 4] = counts[l].view(np.uint8)
    return buf, rec_off, cnt_off, list_stride, count_stride


def upload(lists, counts, layout="blocks", device="cuda:0"):
    # type: (np.ndarray, np.ndarray, str, str) -> tuple
    """``pack`` on the device: (tensor -- keep it alive --, record pointer, count pointer, list stride, count stride) for ``merge_device``."""
    import torch

    buf, rec_off, cnt_off, list_stride, count_stride = pack(lists, counts, layout)
    dev = torch.from_numpy(buf).to(device)
    torch.cuda.synchronize()
    return dev, dev.data_ptr() + rec_off, dev.data_ptr() + cnt_off, list_stride, count_stride


def reference_merge(lists, counts, k, key_words):
    # type: (np.ndarray, np.ndarray, int, int) -> tuple
    """
    The merge restated: per query the first min(count, k) records of every list, stable-sorted by (dist_rank, key_hi, key_lo)
    with the list id last (the lower list first on an exact tie), cut to k.  Returns (keys, hamming, prefix_bits, count) shaped
    as ``HipEngine.merge_device`` returns them, zeros past the count; a query with COUNT_OVERFLOW in any list reports
    COUNT_OVERFLOW and zero rows.
    """
    n_lists, nq, _ = lists.shape
    counts = np.asarray(counts, dtype=np.uint32).reshape(n_lists, nq)
    valid = valid_counts(counts, k)
    keys = np.zeros((nq, k, 2) if key_words == 2 else (nq, k), dtype=np.uint64)
    ham = np.zeros((nq, k), dtype=np.uint32)
    pbits = np.zeros((nq, k), dtype=np.uint16)
    cnt = np.zeros(nq, dtype=np.uint32)
    for q in range(nq):
        if (counts[:, q] == COUNT_OVERFLOW).any():
            cnt[q] = COUNT_OVERFLOW
            continue
        rec = np.concatenate([lists[l, q, : valid[l, q]] for l in range(n_lists)])
        list_id = np.concatenate([np.full(valid[l, q], l) for l in range(n_lists)])
        order = np.lexsort((list_id, rec["key_lo"], rec["key_hi"], rec["dist_rank"]))[:k]
        rec = rec[order]
        c = len(rec)
        cnt[q] = c
        if key_words == 2:
            keys[q, :c, 0], keys[q, :c, 1] = rec["key_hi"], rec["key_lo"]
        else:
            keys[q, :c] = rec["key_lo"]
        ham[q, :c] = rec["hamming"]
        pbits[q, :c] = rec["prefix_bits"]
    return keys, ham, pbits, cnt


def check_record_order(records, count, key_words):
    # type: (np.ndarray, int, int) -> None
    """
    Raw records of ONE query as a device search left them: the first ``count`` strictly ascending in (dist_rank, key), and
    ``dist_rank`` ordering exactly as the fraction hamming / prefix_bits does -- a < b, a == b by integer cross-multiplication, for
    every pair.  (A Hamming table's prefix is constant: the rule is then the order of ``hamming``.)  Raises AssertionError.
    """
    rec = records[:count]
    rank = rec["dist_rank"].astype(np.int64)
    for i in range(1, count):
        a = (int(rank[i - 1]), int(rec["key_hi"][i - 1]), int(rec["key_lo"][i - 1]))
        b = (int(rank[i]), int(rec["key_hi"][i]), int(rec["key_lo"][i]))
        assert a < b, f"records {i - 1}, {i} are not strictly ascending in (dist_rank, key): {a} !< {b}"
    if key_words == 1:
        assert not rec["key_hi"].any(), "key_hi of a 64-bit key is not zero"
    h = rec["hamming"].astype(np.int64)
    p = rec["prefix_bits"].astype(np.int64)
    assert (p > 0).all() and (h <= p).all(), "hamming / prefix_bits of a record are not a distance over a prefix"
    lhs = h[:, None] * p[None, :]          # h_a * p_b
    rhs = h[None, :] * p[:, None]          # h_b * p_a
    less = rank[:, None] < rank[None, :]
    equal = rank[:, None] == rank[None, :]
    bad = np.argwhere((less != (lhs < rhs)) | (equal != (lhs == rhs)))
    assert len(bad) == 0, (
        f"dist_rank does not order as hamming / prefix_bits: records {bad[0].tolist()} have ranks "
        f"{rank[bad[0]].tolist()}, hamming {h[bad[0]].tolist()}, prefix_bits {p[bad[0]].tolist()}"
    )
