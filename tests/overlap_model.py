"""
Host model of ``isccsearch_join_overlaps`` (TEST INFRASTRUCTURE): the asset pairs that share chunks in one simprint table.

Brute force over all row pairs in numpy, dicts for the aggregation.  A row is a chunk: ``keys[i] = (asset, offset << 32 | size)``,
``words[i]`` its code (zero past ``ndim`` bits).  The stop-chunk rule models the document frequency as ``csrc/docfreq.h`` defines it:
distinct assets among the first ``dup_limit`` rows of equal code by ascending key.
"""

from collections import defaultdict

import numpy as np

OVERLAP_DTYPE = np.dtype([("src", "<u4"), ("dst", "<u4"), ("matched", "<u4"), ("reserved", "<u4"), ("sum_hamming", "<u8"), ("chunk_pairs", "<u8")])
INFO_NAMES = ("chunk_pairs", "records", "live_rows", "stop_chunks")
ENOSPC = "ENOSPC"


def chunk_keys(assets, offsets=None, sizes=None):
    """[n, 2] uint64 keys of chunks of ``assets`` (the chunk's position as its offset unless given, size 1)."""
    assets = np.asarray(assets, dtype=np.uint64)
    n = len(assets)
    offsets = np.arange(n, dtype=np.uint64) if offsets is None else np.asarray(offsets, dtype=np.uint64)
    sizes = np.ones(n, dtype=np.uint64) if sizes is None else np.asarray(sizes, dtype=np.uint64)
    return np.stack([assets, (offsets << np.uint64(32)) | sizes], axis=1)


def doc_freq(keys, words, dup_limit):
    """freq[i]: distinct assets among the first ``dup_limit`` rows (ascending key) that hold the code of row i."""
    runs = defaultdict(list)
    for i, w in enumerate(words.tolist()):
        runs[tuple(w)].append(i)
    freq = np.zeros(len(keys), dtype=np.uint32)
    for rows in runs.values():
        rows.sort(key=lambda i: (int(keys[i, 0]), int(keys[i, 1])))
        count = len({int(keys[i, 0]) for i in rows[:dup_limit]})
        freq[rows] = count
    return freq


def row_labels(keys, words, asset_keys, max_doc_freq, dup_limit):
    """(label per row or -1, live mask, stop mask): the label is the rank of the row's asset in ``asset_keys``; stop chunks have none."""
    asset_keys = np.asarray(asset_keys, dtype=np.uint64)
    assert len(asset_keys) and bool(np.all(asset_keys[1:] > asset_keys[:-1]))
    n = len(keys)
    if n == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool), np.zeros(0, dtype=bool)
    pos = np.searchsorted(asset_keys, keys[:, 0])
    live = (pos < len(asset_keys)) & (asset_keys[np.minimum(pos, len(asset_keys) - 1)] == keys[:, 0])
    stop = np.zeros(n, dtype=bool)
    if max_doc_freq > 0:
        stop = live & (doc_freq(keys, words, dup_limit) > max_doc_freq)
    labels = np.where(live & ~stop, pos, -1).astype(np.int64)
    return labels, live, stop


def chunk_pairs(labels, words, max_hamming):
    """(i, j, hamming) of every chunk pair i < j: both rows labelled, the labels different, the distance within ``max_hamming``."""
    n = len(labels)
    out_i, out_j, out_h = [], [], []
    for i0 in range(0, n, 256):
        i1 = min(i0 + 256, n)
        h = np.zeros((i1 - i0, n), dtype=np.int64)
        for w in range(words.shape[1]):
            h += np.bitwise_count(words[i0:i1, None, w] ^ words[None, :, w]).astype(np.int64)
        ok = (h <= max_hamming) & (np.arange(n)[None, :] > np.arange(i0, i1)[:, None])
        ok &= (labels[i0:i1, None] >= 0) & (labels[None, :] >= 0) & (labels[i0:i1, None] != labels[None, :])
        ii, jj = np.nonzero(ok)
        out_i.append(ii + i0)
        out_j.append(jj)
        out_h.append(h[ii, jj])
    if not out_i:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(out_i), np.concatenate(out_j), np.concatenate(out_h)


def model_overlaps(keys, words, asset_keys, max_hamming, max_doc_freq=0, dup_limit=1000, capacity=None):
    """
    ``(rc, records, chunks, info)`` of the C call: ``rc`` 0 or ``ENOSPC`` (then only ``info["chunk_pairs"]`` means anything),
    ``records`` an ``OVERLAP_DTYPE`` array sorted by (src, dst), ``chunks`` uint32 per listed asset, ``info`` a dict.
    ``capacity`` None: room for everything.
    """
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 2)
    words = np.asarray(words, dtype=np.uint64).reshape(len(keys), -1) if len(keys) else np.zeros((0, 1), dtype=np.uint64)
    labels, live, stop = row_labels(keys, words, asset_keys, max_doc_freq, dup_limit)
    chunks = np.zeros(len(asset_keys), dtype=np.uint32)
    if len(keys):
        np.add.at(chunks, np.searchsorted(np.asarray(asset_keys, dtype=np.uint64), keys[live, 0]), 1)
    ii, jj, hh = chunk_pairs(labels, words, max_hamming)
    best = {}                      # (src, dst, row of src) -> smallest distance to a row of dst
    pairs = defaultdict(int)       # (src, dst) -> chunk pairs
    for i, j, h in zip(ii.tolist(), jj.tolist(), hh.tolist()):
        for src_row, dst_row in ((i, j), (j, i)):
            src, dst = int(labels[src_row]), int(labels[dst_row])
            pairs[(src, dst)] += 1
            k = (src, dst, src_row)
            best[k] = min(best.get(k, h), h)
    matched, sums = defaultdict(int), defaultdict(int)
    for (src, dst, _), h in best.items():
        matched[(src, dst)] += 1
        sums[(src, dst)] += h
    records = np.zeros(len(pairs), dtype=OVERLAP_DTYPE)
    for r, (src, dst) in enumerate(sorted(pairs)):
        records[r] = (src, dst, matched[(src, dst)], 0, sums[(src, dst)], pairs[(src, dst)])
    info = dict(zip(INFO_NAMES, (len(ii), len(records), int(live.sum()), int(stop.sum()))))
    if capacity is not None and len(ii) > capacity:
        return ENOSPC, None, None, {"chunk_pairs": len(ii)}
    return 0, records, chunks, info
