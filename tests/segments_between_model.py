"""
Host model of ``isccsearch_join_segments_between`` (TEST INFRASTRUCTURE): where the assets of two simprint tables share chunks.

The overlap part is ``overlap_between_model.model_overlaps_between``; the chunk pairs are those of its ``cross_chunk_pairs`` (brute force
over all A x B row pairs) with its ``side_labels``.  A row's ordinal is counted by its definition IN ITS OWN TABLE
(``segments_model.ordinals``), and a segment is grown forward from every chunk pair that has no predecessor ``(o_a - 1, o_b - 1)`` among
its asset pair's chunk pairs.  ``src`` is always the label of the table_a asset and ``dst`` that of the table_b asset.
"""

from collections import defaultdict

import numpy as np

from overlap_between_model import ENOSPC, SKIP_SAME_ASSET, cross_chunk_pairs, model_overlaps_between, side_labels
from segments_model import SEGMENT_DTYPE, ordinals

INFO_NAMES = ("chunk_pairs", "records", "live_rows_a", "stop_chunks_a", "live_rows_b", "stop_chunks_b", "segments")


def model_segments_between(keys_a, words_a, keys_b, words_b, asset_keys_a, asset_keys_b, max_hamming, max_doc_freq=0, dup_limit=1000,
                           flags=SKIP_SAME_ASSET, capacity=None):
    """
    ``(rc, records, chunks_a, chunks_b, info, segments)`` of the C call: the first five as ``model_overlaps_between`` returns them (``info``
    with ``"segments"``), ``segments`` a ``SEGMENT_DTYPE`` array sorted by (src, dst, first_dst - first_src, first_src).
    """
    keys_a = np.asarray(keys_a, dtype=np.uint64).reshape(-1, 2)
    keys_b = np.asarray(keys_b, dtype=np.uint64).reshape(-1, 2)
    rc, records, chunks_a, chunks_b, info = model_overlaps_between(keys_a, words_a, keys_b, words_b, asset_keys_a, asset_keys_b, max_hamming,
                                                                   max_doc_freq, dup_limit, flags, capacity)
    if rc == ENOSPC:
        return rc, None, None, None, info, None
    W = max([np.asarray(w).reshape(len(k), -1).shape[1] for k, w in ((keys_a, words_a), (keys_b, words_b)) if len(k)] or [1])
    words_a = np.asarray(words_a, dtype=np.uint64).reshape(len(keys_a), -1) if len(keys_a) else np.zeros((0, W), dtype=np.uint64)
    words_b = np.asarray(words_b, dtype=np.uint64).reshape(len(keys_b), -1) if len(keys_b) else np.zeros((0, W), dtype=np.uint64)
    labels_a = side_labels(keys_a, words_a, asset_keys_a, max_doc_freq, dup_limit)[0]
    labels_b = side_labels(keys_b, words_b, asset_keys_b, max_doc_freq, dup_limit)[0]
    ords_a, ords_b = ordinals(keys_a), ordinals(keys_b)
    by_pair = defaultdict(dict)     # (label a, label b) -> {(o_a, o_b): (hamming, row of A, row of B)}
    ii, jj, hh = cross_chunk_pairs(labels_a, words_a, keys_a[:, 0], labels_b, words_b, keys_b[:, 0], max_hamming, bool(flags & SKIP_SAME_ASSET))
    for i, j, h in zip(ii.tolist(), jj.tolist(), hh.tolist()):
        by_pair[(int(labels_a[i]), int(labels_b[j]))][(int(ords_a[i]), int(ords_b[j]))] = (h, i, j)
    place = lambda keys, row: (int(keys[row, 1]) >> 32, int(keys[row, 1]) & 0xFFFFFFFF)
    rows = []
    for (src, dst), pairs in by_pair.items():
        for (o_a, o_b), (h, row_a, row_b) in pairs.items():
            if (o_a - 1, o_b - 1) in pairs:
                continue
            length, total, last = 1, h, (row_a, row_b)
            while (o_a + length, o_b + length) in pairs:
                h2, r_a, r_b = pairs[(o_a + length, o_b + length)]
                total += h2
                last = (r_a, r_b)
                length += 1
            rows.append((src, dst, o_b - o_a, o_a, o_b, length, total, place(keys_a, row_a)[0], place(keys_b, row_b)[0],
                         sum(place(keys_a, last[0])), sum(place(keys_b, last[1]))))
    rows.sort()
    segments = np.zeros(len(rows), dtype=SEGMENT_DTYPE)
    for r, (src, dst, _, o_a, o_b, length, total, begin_a, begin_b, end_a, end_b) in enumerate(rows):
        segments[r] = (src, dst, o_a, o_b, length, total, begin_a, begin_b, end_a, end_b)
    return 0, records, chunks_a, chunks_b, dict(info, segments=len(segments)), segments
