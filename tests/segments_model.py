"""
Host model of ``isccsearch_join_segments`` (TEST INFRASTRUCTURE): where the asset pairs of one simprint table share chunks.

The overlap part is ``overlap_model.model_overlaps``; the chunk pairs are those of ``overlap_model.chunk_pairs`` (brute force over all
row pairs).  A row's ordinal is counted by its definition -- rows of the same asset with a smaller second key word -- and a segment is
grown forward from every chunk pair that has no predecessor ``(o_src - 1, o_dst - 1)`` among its asset pair's chunk pairs.
"""

from collections import defaultdict

import numpy as np

from overlap_model import ENOSPC, chunk_pairs, model_overlaps, row_labels

SEGMENT_DTYPE = np.dtype([("src", "<u4"), ("dst", "<u4"), ("first_src", "<u4"), ("first_dst", "<u4"), ("length", "<u4"), ("sum_hamming", "<u4"),
                          ("begin_src", "<u4"), ("begin_dst", "<u4"), ("end_src", "<u8"), ("end_dst", "<u8")])
INFO_NAMES = ("chunk_pairs", "records", "live_rows", "stop_chunks", "segments")


def ordinals(keys):
    """ordinal[i]: the rows with key word 0 of row i and a smaller key word 1, counted row by row."""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 2)
    out = np.zeros(len(keys), dtype=np.int64)
    for i in range(len(keys)):
        out[i] = int(np.count_nonzero((keys[:, 0] == keys[i, 0]) & (keys[:, 1] < keys[i, 1])))
    return out


def oriented_pairs(keys, words, asset_keys, max_hamming, max_doc_freq=0, dup_limit=1000):
    """{(src, dst): {(o_src, o_dst): (hamming, row_src, row_dst)}} of the chunk pairs, src < dst."""
    labels, _, _ = row_labels(keys, words, asset_keys, max_doc_freq, dup_limit)
    ords = ordinals(keys)
    out = defaultdict(dict)
    for i, j, h in zip(*(a.tolist() for a in chunk_pairs(labels, words, max_hamming))):
        if labels[i] > labels[j]:
            i, j = j, i
        out[(int(labels[i]), int(labels[j]))][(int(ords[i]), int(ords[j]))] = (h, i, j)
    return out


def model_segments(keys, words, asset_keys, max_hamming, max_doc_freq=0, dup_limit=1000, capacity=None):
    """
    ``(rc, records, chunks, info, segments)`` of the C call: the first four as ``model_overlaps`` returns them (``info`` with
    ``"segments"``), ``segments`` a ``SEGMENT_DTYPE`` array sorted by (src, dst, first_dst - first_src, first_src).
    """
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 2)
    words = np.asarray(words, dtype=np.uint64).reshape(len(keys), -1) if len(keys) else np.zeros((0, 1), dtype=np.uint64)
    rc, records, chunks, info = model_overlaps(keys, words, asset_keys, max_hamming, max_doc_freq, dup_limit, capacity)
    if rc == ENOSPC:
        return rc, None, None, info, None
    place = lambda row: (int(keys[row, 1]) >> 32, int(keys[row, 1]) & 0xFFFFFFFF)
    rows = []
    for (src, dst), pairs in oriented_pairs(keys, words, asset_keys, max_hamming, max_doc_freq, dup_limit).items():
        for (o_src, o_dst), (h, row_src, row_dst) in pairs.items():
            if (o_src - 1, o_dst - 1) in pairs:
                continue
            length, total, last = 1, h, (row_src, row_dst)
            while (o_src + length, o_dst + length) in pairs:
                h2, r_src, r_dst = pairs[(o_src + length, o_dst + length)]
                total += h2
                last = (r_src, r_dst)
                length += 1
            rows.append((src, dst, o_dst - o_src, o_src, o_dst, length, total, place(row_src)[0], place(row_dst)[0], sum(place(last[0])), sum(place(last[1]))))
    rows.sort()
    segments = np.zeros(len(rows), dtype=SEGMENT_DTYPE)
    for r, (src, dst, _, o_src, o_dst, length, total, begin_src, begin_dst, end_src, end_dst) in enumerate(rows):
        segments[r] = (src, dst, o_src, o_dst, length, total, begin_src, begin_dst, end_src, end_dst)
    return 0, records, chunks, dict(info, segments=len(segments)), segments
