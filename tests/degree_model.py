"""
Host model of ``isccsearch_join_degrees`` and ``isccsearch_join_within_live`` (``HipTable.join_degrees``, ``HipTable.join_within`` with
``live_keys``): what the device must compute, by the plainest means.

One dense matrix of all-pairs distances: rows i and j compare ``p = min(len_i, len_j)`` bytes -- a code is packed big-endian into 64-bit
words, so the last compared word keeps its TOP ``p % 8`` bytes, as the oracle masks it -- and are NEAR when ``hamming <=
max_hamming[p]`` (a negative entry: never).  A row is LISTED when its key is in ``live_keys``.  The degree of a listed key is the
number of other listed rows near its row (0 for a key the table does not hold), the links are the near pairs of two listed rows, and
the live pairs are those pairs as ``join_within`` writes them: key_a < key_b, sorted by (key_a, key_b).  64-bit keys; tables of a few
thousand rows at the most (the matrix is n x n).
"""

import numpy as np


def word_masks():
    """[33, 4]: the bits of word w that a prefix of p bytes compares"""
    m = np.zeros((33, 4), dtype=np.uint64)
    for p in range(1, 33):
        for w in range(4):
            nbytes = min(max(p - 8 * w, 0), 8)
            m[p, w] = np.uint64((((1 << (8 * nbytes)) - 1) << (8 * (8 - nbytes))) & 0xFFFFFFFFFFFFFFFF)
    return m


def near_matrix(words, nb, mh):
    """(near [n, n] bool, symmetric, False on the diagonal; hamming [n, n]; prefix bytes [n, n])"""
    words = np.asarray(words, dtype=np.uint64)
    nb = np.asarray(nb).astype(np.int64)
    mh = np.asarray(mh).astype(np.int64)
    n = len(nb)
    p = np.minimum(nb[:, None], nb[None, :])
    h = np.zeros((n, n), dtype=np.int64)
    masks = word_masks()
    for w in range(words.shape[1] if n else 0):
        h += np.bitwise_count((words[:, None, w] ^ words[None, :, w]) & masks[p, w]).astype(np.int64)
    near = h <= mh[p]
    near[np.arange(n), np.arange(n)] = False
    return near, h, p


def listed_near(keys, words, nb, mh, live_keys, matrix=None):
    """near_matrix (or ``matrix``, its result for the same table and thresholds) restricted to pairs of two listed rows, and the rows' listing"""
    keys = np.asarray(keys, dtype=np.uint64)
    listed = np.isin(keys, np.asarray(live_keys, dtype=np.uint64))
    near, h, p = matrix if matrix is not None else near_matrix(words, nb, mh)
    return near & listed[:, None] & listed[None, :], h, p, listed


def join_degrees(keys, words, nb, mh, live_keys, matrix=None):
    """(degrees uint32 [n_live], links) -- the model of one ``isccsearch_join_degrees`` call"""
    keys = np.asarray(keys, dtype=np.uint64)
    live_keys = np.asarray(live_keys, dtype=np.uint64)
    near, _, _, listed = listed_near(keys, words, nb, mh, live_keys, matrix)
    degrees = np.zeros(len(live_keys), dtype=np.uint32)
    degrees[np.searchsorted(live_keys, keys[listed])] = near.sum(axis=1)[listed]
    return degrees, int(near.sum()) // 2


def join_within_live(keys, words, nb, mh, live_keys, matrix=None):
    """(keys_a, keys_b, hamming, prefix_bits) -- the model of one ``isccsearch_join_within_live`` call that fits its capacity"""
    keys = np.asarray(keys, dtype=np.uint64)
    near, h, p, _ = listed_near(keys, words, nb, mh, live_keys, matrix)
    ii, jj = np.nonzero(near & (keys[:, None] < keys[None, :]))
    order = np.lexsort((keys[jj], keys[ii]))
    ii, jj = ii[order], jj[order]
    return keys[ii], keys[jj], h[ii, jj].astype(np.uint32), (8 * p[ii, jj]).astype(np.uint16)
