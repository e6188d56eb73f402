"""
Host model of ``isccsearch_join_components`` (``HipTable.join_components``): what the device must compute, by the slowest means.

The qualifying row pairs come from the brute force the join tests use (``test_gpu_duplicates.np_join``: every pair of distinct rows
within ``max_hamming[min(len_a, len_b)]`` bits over the common prefix); pairs with a row whose key has no label are dropped; a dict
union-find over the labels takes the links of the input forest and one link per remaining pair; the answer is the smallest label of
every label's component, and the number of remaining pairs.
"""

import numpy as np

from test_gpu_duplicates import np_join

NONE = 0xFFFFFFFF


def row_pairs(keys, words, nb, mh):
    """(keys_a, keys_b) of the qualifying row pairs; none for fewer than two rows."""
    if len(nb) < 2:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64)
    ka, kb, _, _ = np_join(np.asarray(keys, dtype=np.uint64), np.asarray(words, dtype=np.uint64), np.asarray(nb), np.asarray(mh, dtype=np.int64))
    return ka, kb


def components(n_labels, parent_in, label_pairs):
    """Smallest label per component (uint32 [n_labels]) under the input forest's links plus ``label_pairs``, by a dict union-find."""
    up = {}

    def find(x):
        while up.get(x, x) != x:
            x = up[x]
        return x

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            up[max(a, b)] = min(a, b)

    for i, p in enumerate(np.asarray(parent_in).tolist()):
        assert p <= i, "the input forest needs parent[i] <= i"
        union(i, p)
    for a, b in label_pairs:
        union(a, b)
    return np.array([find(i) for i in range(n_labels)], dtype=np.uint32)


def linked_pairs(keys, words, nb, mh, live_keys, live_labels):
    """[(label_a, label_b)] of the qualifying row pairs whose two rows have labels: the links of one call."""
    label_of = dict(zip(np.asarray(live_keys, dtype=np.uint64).tolist(), np.asarray(live_labels, dtype=np.uint32).tolist()))
    ka, kb = row_pairs(keys, words, nb, mh)
    return [(label_of[a], label_of[b]) for a, b in zip(ka.tolist(), kb.tolist()) if a in label_of and b in label_of]


def join_components(keys, words, nb, mh, live_keys, live_labels, parent_in):
    """(parent_out, links) for a table of rows (keys, words, nb) -- the model of one call."""
    linked = linked_pairs(keys, words, nb, mh, live_keys, live_labels)
    return components(len(parent_in), parent_in, linked), len(linked)
