"""
The host model of ``isccsearch_join_segments`` (``tests/segments_model.py``) against records worked by hand, against a second
derivation written independently (group the chunk pairs of an asset pair by diagonal, sort, split where the ordinal jumps) and against
the invariant that ties it to the overlap records: the lengths of the segments of (src, dst) add up to ``chunk_pairs``.
"""

from collections import defaultdict

import numpy as np

from overlap_model import ENOSPC, chunk_keys, model_overlaps
from segments_model import SEGMENT_DTYPE, model_segments, oriented_pairs, ordinals

A, B, C, D, E, X, Y = (int(v) for v in np.random.default_rng(5).integers(0, 2**63, size=7))     # about 32 bits apart
C3 = C ^ 0b111                                  # three bits off C


def tuples(segments):
    return [tuple(int(v) for v in s) for s in segments.tolist()]


def hand_table():
    """Four assets; the rows in an order unrelated to their offsets."""
    rows = []
    rows += [(10, i * 100, 100, c) for i, c in enumerate([A, B, C, D, E])]
    rows += [(20, i * 50, 50, c) for i, c in enumerate([X, B, C3, Y, E, A])]
    rows += [(30, i * 10, 10, c) for i, c in enumerate([C, D])]
    rows += [(40, 0, 9, B), (40, 0, 5, Y ^ 1)]                        # equal offsets: the smaller size comes first
    order = np.random.default_rng(1).permutation(len(rows))
    rows = [rows[i] for i in order]
    keys = chunk_keys([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
    words = np.array([[r[3]] for r in rows], dtype=np.uint64)
    return keys, words


def test_ordinals_count_within_the_asset():
    keys, _ = hand_table()
    ords = ordinals(keys)
    for asset, size in ((10, 100), (20, 50), (30, 10)):
        mine = keys[:, 0] == asset
        assert (ords[mine] == (keys[mine, 1] >> np.uint64(32)) // size).all()
    nine = int(np.nonzero((keys[:, 0] == 40) & ((keys[:, 1] & np.uint64(0xFFFFFFFF)) == 9))[0][0])
    five = int(np.nonzero((keys[:, 0] == 40) & ((keys[:, 1] & np.uint64(0xFFFFFFFF)) == 5))[0][0])
    assert (ords[five], ords[nine]) == (0, 1)


def test_records_worked_by_hand():
    keys, words = hand_table()
    rc, records, chunks, info, segments = model_segments(keys, words, [10, 20, 30, 40], 3)
    assert rc == 0 and chunks.tolist() == [5, 6, 2, 2]
    assert tuples(segments) == [
        # 10 and 20: B, C (three bits off) on the diagonal 0, D against Y splits the run from E; A sits five chunks further on in 20
        (0, 1, 1, 1, 2, 3, 100, 50, 300, 150),
        (0, 1, 4, 4, 1, 0, 400, 200, 500, 250),
        (0, 1, 0, 5, 1, 0, 0, 250, 100, 300),
        # 10 and 30: chunks 2, 3 of 10 are chunks 0, 1 of 30 -- a negative diagonal
        (0, 2, 2, 0, 2, 0, 200, 0, 400, 20),
        # 10 and 40: B is 40's second chunk (offset 0, the larger size)
        (0, 3, 1, 1, 1, 0, 100, 0, 200, 9),
        # 20 and 30: C3 against C;  20 and 40: B;  Y against Y ^ 1 on the diagonal -3
        (1, 2, 2, 0, 1, 3, 100, 0, 150, 10),
        (1, 3, 3, 0, 1, 1, 150, 0, 200, 5),
        (1, 3, 1, 1, 1, 0, 50, 0, 100, 9),
    ]
    assert info == {"chunk_pairs": 10, "records": 10, "live_rows": 15, "stop_chunks": 0, "segments": 8}
    assert segments.dtype == SEGMENT_DTYPE and SEGMENT_DTYPE.itemsize == 48
    # the overlap part is model_overlaps', unchanged
    rc, exp_records, exp_chunks, exp_info = model_overlaps(keys, words, [10, 20, 30, 40], 3)
    assert records.tobytes() == exp_records.tobytes() and (chunks == exp_chunks).all() and {k: info[k] for k in exp_info} == exp_info
    # at radius 0 the three-bit pairs are gone: the first run shrinks to B alone
    _, _, _, _, exact = model_segments(keys, words, [10, 20, 30, 40], 0)
    assert tuples(exact)[0] == (0, 1, 1, 1, 1, 0, 100, 50, 200, 100) and len(exact) == 6


def test_unlisted_assets_and_stop_chunks():
    keys, words = hand_table()
    # without asset 20 its rows pair with nothing, and the labels close up
    _, _, chunks, info, segments = model_segments(keys, words, [10, 30, 40], 3)
    assert tuples(segments) == [(0, 1, 2, 0, 2, 0, 200, 0, 400, 20), (0, 2, 1, 1, 1, 0, 100, 0, 200, 9)] and chunks.tolist() == [5, 2, 2]
    # B is held by three assets: above a cut of 2 it is a stop chunk, which keeps its ordinal and splits nothing it is not part of
    _, _, chunks, info, segments = model_segments(keys, words, [10, 20, 30, 40], 3, max_doc_freq=2)
    assert info["stop_chunks"] == 3 and chunks.tolist() == [5, 6, 2, 2]
    assert tuples(segments)[0] == (0, 1, 2, 2, 1, 3, 200, 100, 300, 150)
    assert all(s[:2] != (0, 3) for s in tuples(segments))


def test_ends_may_pass_32_bits_and_capacity():
    keys = chunk_keys([1, 1, 2, 2], [0xFFFFFE00, 0xFFFFFF00, 0, 0xFFFFFF00], [0x100, 0x1000, 8, 0x1000])
    words = np.array([[A], [B], [A], [B]], dtype=np.uint64)
    rc, _, _, info, segments = model_segments(keys, words, [1, 2], 0)
    assert tuples(segments) == [(0, 1, 0, 0, 2, 0, 0xFFFFFE00, 0, 0x100000F00, 0x100000F00)]
    assert model_segments(keys, words, [1, 2], 0, capacity=1)[0] == ENOSPC
    assert model_segments(keys, words, [1, 2], 0, capacity=1)[3] == {"chunk_pairs": 2}
    assert model_segments(keys, words, [1, 2], 0, capacity=2)[0] == 0
    rc, records, chunks, info, segments = model_segments(np.zeros((0, 2), np.uint64), np.zeros((0, 1), np.uint64), [1, 2], 0)
    assert rc == 0 and len(segments) == 0 and info["segments"] == 0


def by_diagonals(keys, words, asset_keys, max_hamming, max_doc_freq=0):
    """The second derivation: per asset pair group the chunk pairs by diagonal, sort by o_src, split where o_src jumps."""
    out = []
    for (src, dst), pairs in sorted(oriented_pairs(keys, words, asset_keys, max_hamming, max_doc_freq).items()):
        diagonals = defaultdict(list)
        for (o_src, o_dst), (h, row_src, row_dst) in pairs.items():
            diagonals[o_dst - o_src].append((o_src, h, row_src, row_dst))
        for d in sorted(diagonals):
            run = []
            for item in sorted(diagonals[d]) + [None]:
                if run and (item is None or item[0] != run[-1][0] + 1):
                    (o, _, r_src, r_dst), (_, _, l_src, l_dst) = run[0], run[-1]
                    offset = lambda r: int(keys[r, 1]) >> 32
                    end = lambda r: offset(r) + (int(keys[r, 1]) & 0xFFFFFFFF)
                    out.append((src, dst, o, o + d, len(run), sum(x[1] for x in run), offset(r_src), offset(r_dst), end(l_src), end(l_dst)))
                    run = []
                if item is not None:
                    run.append(item)
    return out


def small_table(rng):
    """A few assets of a few chunks over a small pool of codes, with copied stretches: runs of every length, some diagonals shared."""
    n_assets = int(rng.integers(2, 6))
    pool = rng.integers(0, 2**64, size=int(rng.integers(3, 9)), dtype=np.uint64)
    assets, offsets, sizes, codes = [], [], [], []
    for a in range(n_assets):
        k = int(rng.integers(1, 9))
        seq = pool[rng.integers(0, len(pool), size=k)]
        for i in range(k):
            assets.append(7 * a + 3)
            offsets.append(int(rng.integers(0, 4)) * 1000 + i)         # clusters of offsets: ordinals differ from offsets
            sizes.append(int(rng.integers(1, 50)))
            codes.append(int(seq[i]) ^ (1 << int(rng.integers(0, 64)) if rng.random() < 0.3 else 0))
    uniq = {}
    for i, key in enumerate(zip(assets, offsets, sizes)):
        uniq[key] = i                                                  # keys are unique in a table
    rows = rng.permutation(sorted(uniq.values()))
    keys = chunk_keys(np.array(assets)[rows], np.array(offsets)[rows], np.array(sizes)[rows])
    words = np.array(codes, dtype=np.uint64)[rows][:, None]
    listed = sorted({7 * a + 3 for a in range(n_assets) if n_assets < 3 or a != 1} | {1})
    return keys, words, np.array(listed, dtype=np.uint64)


def test_two_derivations_and_the_sum_of_lengths_on_200_tables():
    rng = np.random.default_rng(77)
    with_segments = longer = 0
    for _ in range(200):
        keys, words, asset_keys = small_table(rng)
        for tau, cut in ((0, 0), (1, 0), (1, 2)):
            rc, records, chunks, info, segments = model_segments(keys, words, asset_keys, tau, max_doc_freq=cut)
            assert rc == 0
            assert tuples(segments) == by_diagonals(keys, words, asset_keys, tau, cut)
            lengths = defaultdict(int)
            for s in segments:
                assert s["src"] < s["dst"] and s["length"] >= 1
                lengths[(int(s["src"]), int(s["dst"]))] += int(s["length"])
            pairs = {(int(r["src"]), int(r["dst"])): int(r["chunk_pairs"]) for r in records if r["src"] < r["dst"]}
            assert lengths == pairs
            assert info["segments"] == len(segments) and sum(lengths.values()) == info["chunk_pairs"]
            order = [(int(s["src"]), int(s["dst"]), int(s["first_dst"]) - int(s["first_src"]), int(s["first_src"])) for s in segments]
            assert order == sorted(order) and len(set(order)) == len(order)
            with_segments += len(segments) > 0
            longer += int((segments["length"] > 1).sum())
    assert with_segments > 300 and longer > 100
