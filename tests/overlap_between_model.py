"""
Host model of ``isccsearch_join_overlaps_between`` (TEST INFRASTRUCTURE): the pairs (asset of table A, asset of table B) that share chunks.

Brute force over all A x B row pairs in numpy, dicts for the aggregation.  Rows, keys and codes as in ``overlap_model.py``; each table has
its own listed assets (two label spaces: the rank in its own side's ``asset_keys``) and its own document frequencies -- a row is a stop
chunk by the frequency of its code in ITS table alone.
"""

from collections import defaultdict

import numpy as np

from overlap_model import ENOSPC, OVERLAP_DTYPE, chunk_keys, doc_freq  # noqa: F401  (chunk_keys: for the tests that build tables)

INFO_NAMES = ("chunk_pairs", "records", "live_rows_a", "stop_chunks_a", "live_rows_b", "stop_chunks_b")
SKIP_SAME_ASSET = 1


def side_labels(keys, words, asset_keys, max_doc_freq, dup_limit):
    """(label per row or -1, live mask, stop mask, chunks per listed asset) of one table."""
    asset_keys = np.asarray(asset_keys, dtype=np.uint64)
    assert len(asset_keys) and bool(np.all(asset_keys[1:] > asset_keys[:-1]))
    chunks = np.zeros(len(asset_keys), dtype=np.uint32)
    n = len(keys)
    if n == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool), np.zeros(0, dtype=bool), chunks
    pos = np.searchsorted(asset_keys, keys[:, 0])
    live = (pos < len(asset_keys)) & (asset_keys[np.minimum(pos, len(asset_keys) - 1)] == keys[:, 0])
    stop = np.zeros(n, dtype=bool)
    if max_doc_freq > 0:
        stop = live & (doc_freq(keys, words, dup_limit) > max_doc_freq)
    np.add.at(chunks, pos[live], 1)
    return np.where(live & ~stop, pos, -1).astype(np.int64), live, stop, chunks


def cross_chunk_pairs(labels_a, words_a, assets_a, labels_b, words_b, assets_b, max_hamming, skip_same_asset):
    """(i, j, hamming) of every chunk pair: row i of A and row j of B, both labelled, within ``max_hamming``; not of one asset key if skipped."""
    out_i, out_j, out_h = [], [], []
    n_b = len(labels_b)
    for i0 in range(0, len(labels_a), 256):
        i1 = min(i0 + 256, len(labels_a))
        h = np.zeros((i1 - i0, n_b), dtype=np.int64)
        for w in range(words_a.shape[1]):
            h += np.bitwise_count(words_a[i0:i1, None, w] ^ words_b[None, :, w]).astype(np.int64)
        ok = (h <= max_hamming) & (labels_a[i0:i1, None] >= 0) & (labels_b[None, :] >= 0)
        if skip_same_asset:
            ok &= assets_a[i0:i1, None] != assets_b[None, :]
        ii, jj = np.nonzero(ok)
        out_i.append(ii + i0)
        out_j.append(jj)
        out_h.append(h[ii, jj])
    if not out_i:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(out_i), np.concatenate(out_j), np.concatenate(out_h)


def model_overlaps_between(keys_a, words_a, keys_b, words_b, asset_keys_a, asset_keys_b, max_hamming, max_doc_freq=0, dup_limit=1000,
                           flags=SKIP_SAME_ASSET, capacity=None):
    """
    ``(rc, records, chunks_a, chunks_b, info)`` of the C call: ``rc`` 0 or ``ENOSPC`` (then only ``info["chunk_pairs"]`` means anything),
    ``records`` an ``OVERLAP_DTYPE`` array sorted by (reserved, src, dst) -- reserved 0: src a label of side A, dst of side B; 1: the
    other way round --, ``chunks_x`` uint32 per listed asset of either side, ``info`` a dict.  ``capacity`` None: room for everything.
    """
    keys_a = np.asarray(keys_a, dtype=np.uint64).reshape(-1, 2)
    keys_b = np.asarray(keys_b, dtype=np.uint64).reshape(-1, 2)
    W = max([np.asarray(w).reshape(len(k), -1).shape[1] for k, w in ((keys_a, words_a), (keys_b, words_b)) if len(k)] or [1])
    words_a = np.asarray(words_a, dtype=np.uint64).reshape(len(keys_a), -1) if len(keys_a) else np.zeros((0, W), dtype=np.uint64)
    words_b = np.asarray(words_b, dtype=np.uint64).reshape(len(keys_b), -1) if len(keys_b) else np.zeros((0, W), dtype=np.uint64)
    labels_a, live_a, stop_a, chunks_a = side_labels(keys_a, words_a, asset_keys_a, max_doc_freq, dup_limit)
    labels_b, live_b, stop_b, chunks_b = side_labels(keys_b, words_b, asset_keys_b, max_doc_freq, dup_limit)
    ii, jj, hh = cross_chunk_pairs(labels_a, words_a, keys_a[:, 0], labels_b, words_b, keys_b[:, 0], max_hamming, bool(flags & SKIP_SAME_ASSET))
    best = {}                      # (direction, src, dst, row of src) -> smallest distance to a row of dst
    pairs = defaultdict(int)       # (direction, src, dst) -> chunk pairs
    for i, j, h in zip(ii.tolist(), jj.tolist(), hh.tolist()):
        la, lb = int(labels_a[i]), int(labels_b[j])
        for k in ((0, la, lb, i), (1, lb, la, j)):
            pairs[k[:3]] += 1
            best[k] = min(best.get(k, h), h)
    matched, sums = defaultdict(int), defaultdict(int)
    for k, h in best.items():
        matched[k[:3]] += 1
        sums[k[:3]] += h
    records = np.zeros(len(pairs), dtype=OVERLAP_DTYPE)
    for r, k in enumerate(sorted(pairs)):
        direction, src, dst = k
        records[r] = (src, dst, matched[k], direction, sums[k], pairs[k])
    info = dict(zip(INFO_NAMES, (len(ii), len(records), int(live_a.sum()), int(stop_a.sum()), int(live_b.sum()), int(stop_b.sum()))))
    if capacity is not None and len(ii) > capacity:
        return ENOSPC, None, None, None, {"chunk_pairs": len(ii)}
    return 0, records, chunks_a, chunks_b, info
