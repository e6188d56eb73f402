"""
The host model of ``isccsearch_join_segments_between`` (``tests/segments_between_model.py``) against records worked by hand, against the
one-table model (``segments_model.model_segments`` over both tables concatenated, for tables with disjoint asset keys) and against the
invariants that tie it to the overlap records: its overlap part is ``model_overlaps_between``'s, and the lengths of the segments of
(a, b) add up to ``chunk_pairs`` of the records (0, a, b) and (1, b, a).
"""

from collections import defaultdict

import numpy as np

from overlap_between_model import ENOSPC, SKIP_SAME_ASSET, chunk_keys, model_overlaps_between
from segments_between_model import INFO_NAMES, model_segments_between
from segments_model import SEGMENT_DTYPE, model_segments

A, B, C, D, E, X, Y = (int(v) for v in np.random.default_rng(5).integers(0, 2**63, size=7))     # about 32 bits apart
C3 = C ^ 0b111                                  # three bits off C


def tuples(segments):
    return [tuple(int(v) for v in s) for s in segments.tolist()]


def table(rows, seed):
    """(keys, words) of rows (asset, offset, size, code), in an order unrelated to their offsets."""
    order = np.random.default_rng(seed).permutation(len(rows))
    rows = [rows[i] for i in order]
    return chunk_keys([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]), np.array([[r[3]] for r in rows], dtype=np.uint64)


def hand_tables():
    """Table a: assets 10 (five chunks) and 50 (one).  Table b: assets 20, 30 and 40, which hold stretches of asset 10."""
    rows_a = [(10, i * 100, 100, c) for i, c in enumerate([A, B, C, D, E])] + [(50, 7, 3, Y)]
    rows_b = [(20, i * 50, 50, c) for i, c in enumerate([X, B, C3, Y, E, A])]
    rows_b += [(30, i * 10, 10, c) for i, c in enumerate([C, D])]
    rows_b += [(40, 0, 9, B), (40, 0, 5, Y ^ 1)]                      # equal offsets: the smaller size comes first
    return table(rows_a, 1), table(rows_b, 2)


def test_records_worked_by_hand():
    (ka, wa), (kb, wb) = hand_tables()
    rc, records, chunks_a, chunks_b, info, segments = model_segments_between(ka, wa, kb, wb, [10, 50], [20, 30, 40], 3)
    assert rc == 0 and chunks_a.tolist() == [5, 1] and chunks_b.tolist() == [6, 2, 2]
    assert tuples(segments) == [
        # 10 and 20: B, C (three bits off) on the diagonal 0, D against Y splits the run from E; A sits five chunks further on in 20: a
        # second diagonal of the same pair, and runs of length 1
        (0, 0, 1, 1, 2, 3, 100, 50, 300, 150),
        (0, 0, 4, 4, 1, 0, 400, 200, 500, 250),
        (0, 0, 0, 5, 1, 0, 0, 250, 100, 300),
        # 10 and 30: chunks 2, 3 of 10 are chunks 0, 1 of 30 -- a clip at another ordinal, a negative diagonal
        (0, 1, 2, 0, 2, 0, 200, 0, 400, 20),
        # 10 and 40: B is 40's SECOND chunk (offset 0, the larger size)
        (0, 2, 1, 1, 1, 0, 100, 0, 200, 9),
        # 50 and 20: src is the label of table a even where it is the larger number;  50 and 40: Y against Y ^ 1, 40's first chunk
        (1, 0, 0, 3, 1, 0, 7, 150, 10, 200),
        (1, 2, 0, 0, 1, 1, 7, 0, 10, 5),
    ]
    assert info == {"chunk_pairs": 9, "records": 10, "live_rows_a": 6, "stop_chunks_a": 0, "live_rows_b": 10, "stop_chunks_b": 0, "segments": 7}
    assert tuple(info) == INFO_NAMES and segments.dtype == SEGMENT_DTYPE
    # the overlap part is model_overlaps_between's, unchanged
    rc, exp_records, exp_a, exp_b, exp_info = model_overlaps_between(ka, wa, kb, wb, [10, 50], [20, 30, 40], 3)
    assert records.tobytes() == exp_records.tobytes() and (chunks_a == exp_a).all() and (chunks_b == exp_b).all()
    assert {k: info[k] for k in exp_info} == exp_info
    # at radius 0 the three-bit and one-bit pairs are gone: the first run shrinks to B alone
    exact = model_segments_between(ka, wa, kb, wb, [10, 50], [20, 30, 40], 0)[5]
    assert tuples(exact)[0] == (0, 0, 1, 1, 1, 0, 100, 50, 200, 100) and len(exact) == 6


def test_the_sides_exchanged_mirror_every_segment():
    (ka, wa), (kb, wb) = hand_tables()
    ab = model_segments_between(ka, wa, kb, wb, [10, 50], [20, 30, 40], 3)[5]
    ba = model_segments_between(kb, wb, ka, wa, [20, 30, 40], [10, 50], 3)[5]
    mirror = sorted((d, s, fd, fs, n, h, bd, bs, ed, es) for s, d, fs, fd, n, h, bs, bd, es, ed in tuples(ab))
    assert sorted(tuples(ba)) == mirror
    order = [(s, d, fd - fs, fs) for s, d, fs, fd, *_ in tuples(ba)]
    assert order == sorted(order)


def test_unlisted_assets_take_no_part_and_keep_no_label():
    (ka, wa), (kb, wb) = hand_tables()
    # without asset 20 its rows pair with nothing, and table b's labels close up; table a's do not move
    _, _, chunks_a, chunks_b, info, segments = model_segments_between(ka, wa, kb, wb, [10, 50], [30, 40], 3)
    assert tuples(segments) == [(0, 0, 2, 0, 2, 0, 200, 0, 400, 20), (0, 1, 1, 1, 1, 0, 100, 0, 200, 9), (1, 1, 0, 0, 1, 1, 7, 0, 10, 5)]
    assert chunks_a.tolist() == [5, 1] and chunks_b.tolist() == [2, 2] and info["live_rows_b"] == 4


def test_a_stop_chunk_in_table_a_only_splits_the_run_and_keeps_its_ordinal():
    x = [int(v) for v in np.random.default_rng(4).integers(0, 2**63, size=8)]
    rows_a = [(1, i, 4, x[i]) for i in range(8)] + [(a, 0, 4, x[3]) for a in range(3, 8)]      # x[3] is held by six assets of a
    rows_b = [(2, 10 + i, 4, x[i]) for i in range(8)]                                          # and by one of b
    (ka, wa), (kb, wb) = table(rows_a, 3), table(rows_b, 4)
    listed_a = [1, 3, 4, 5, 6, 7]
    _, _, chunks_a, _, info, seg = model_segments_between(ka, wa, kb, wb, listed_a, [2], 0, max_doc_freq=5)
    assert info["stop_chunks_a"] == 6 and info["stop_chunks_b"] == 0 and chunks_a.tolist() == [8, 1, 1, 1, 1, 1]
    # the ordinals still count the stop chunk: the second run starts at chunk 4 of either asset
    assert tuples(seg) == [(0, 0, 0, 0, 3, 0, 0, 10, 6, 16), (0, 0, 4, 4, 4, 0, 4, 14, 11, 21)]
    _, _, _, _, info, seg = model_segments_between(ka, wa, kb, wb, listed_a, [2], 0, max_doc_freq=6)
    assert info["stop_chunks_a"] == 0 and tuples(seg)[0] == (0, 0, 0, 0, 8, 0, 0, 10, 11, 21) and len(seg) == 6
    # the sides exchanged: the chunk is a stop chunk of the table that is now b
    _, _, _, _, info, seg = model_segments_between(kb, wb, ka, wa, [2], listed_a, 0, max_doc_freq=5)
    assert info["stop_chunks_b"] == 6 and tuples(seg) == [(0, 0, 0, 0, 3, 0, 10, 0, 16, 6), (0, 0, 4, 4, 4, 0, 14, 4, 21, 11)]


def test_ends_may_pass_32_bits_and_capacity():
    ka = chunk_keys([1, 1], [0xFFFFFE00, 0xFFFFFF00], [0x100, 0x1000])
    kb = chunk_keys([2, 2], [0, 0xFFFFFF00], [8, 0x2000])
    wa = wb = np.array([[A], [B]], dtype=np.uint64)
    rc, _, _, _, info, segments = model_segments_between(ka, wa, kb, wb, [1], [2], 0)
    assert rc == 0 and tuples(segments) == [(0, 0, 0, 0, 2, 0, 0xFFFFFE00, 0, 0x100000F00, 0x100001F00)]
    refused = model_segments_between(ka, wa, kb, wb, [1], [2], 0, capacity=1)
    assert refused[0] == ENOSPC and refused[4] == {"chunk_pairs": 2} and refused[5] is None
    assert model_segments_between(ka, wa, kb, wb, [1], [2], 0, capacity=2)[0] == 0
    empty = np.zeros((0, 2), np.uint64), np.zeros((0, 1), np.uint64)
    for sides in ((*empty, kb, wb), (ka, wa, *empty), (*empty, *empty)):
        rc, records, _, _, info, segments = model_segments_between(*sides, [1], [2], 0)
        assert rc == 0 and len(records) == 0 and len(segments) == 0 and info["segments"] == 0


def test_an_asset_held_by_both_tables_is_one_run_without_the_flag():
    rows = [(9, i * 10, 10, c) for i, c in enumerate([A, B, C, D, E])]
    (ka, wa), (kb, wb) = table(rows + [(3, 0, 1, X)], 5), table(rows + [(4, 0, 1, Y)], 6)
    _, _, _, _, info, seg = model_segments_between(ka, wa, kb, wb, [3, 9], [4, 9], 0, flags=0)
    assert tuples(seg) == [(1, 1, 0, 0, 5, 0, 0, 0, 50, 50)] and info["chunk_pairs"] == 5
    _, records, _, _, info, seg = model_segments_between(ka, wa, kb, wb, [3, 9], [4, 9], 0, flags=SKIP_SAME_ASSET)
    assert len(seg) == 0 and len(records) == 0 and info["chunk_pairs"] == 0 and info["live_rows_a"] == 6


def small_tables(rng, disjoint):
    """
    Two tables of a few assets of a few chunks off ONE small pool of codes, with clustered offsets (ordinals differ from offsets):
    ``(keys, words, listed)`` per side.  ``disjoint``: no asset key is in both tables; else some are, with rows of their own.
    """
    pool = rng.integers(0, 2**64, size=int(rng.integers(3, 9)), dtype=np.uint64)
    sides = []
    for side in range(2):
        n_assets = int(rng.integers(1, 5))
        rows = {}
        for a in range(n_assets):
            asset = 14 * a + 3 + (7 * side if disjoint or a % 2 else 0)
            k = int(rng.integers(1, 9))
            seq = pool[rng.integers(0, len(pool), size=k)]
            for i in range(k):
                code = int(seq[i]) ^ (1 << int(rng.integers(0, 64)) if rng.random() < 0.3 else 0)
                rows[(asset, int(rng.integers(0, 4)) * 1000 + i, int(rng.integers(1, 50)))] = code        # keys are unique in a table
        order = rng.permutation(len(rows))
        items = [list(rows.items())[i] for i in order]
        keys = chunk_keys([k[0] for k, _ in items], [k[1] for k, _ in items], [k[2] for k, _ in items])
        words = np.array([[c] for _, c in items], dtype=np.uint64)
        listed = sorted({int(k) for k in keys[:, 0].tolist() if n_assets < 3 or k != 17 + 7 * side} | {1})       # one asset unlisted
        sides.append((keys, words, np.array(listed, dtype=np.uint64)))
    return sides


def test_the_overlap_part_and_the_sum_of_lengths_on_200_pairs_of_tables():
    rng = np.random.default_rng(78)
    with_segments = longer = same_key = 0
    for _ in range(200):
        (ka, wa, la), (kb, wb, lb) = small_tables(rng, disjoint=False)
        for tau, cut, flags in ((0, 0, SKIP_SAME_ASSET), (1, 0, 0), (1, 2, SKIP_SAME_ASSET)):
            rc, records, chunks_a, chunks_b, info, segments = model_segments_between(ka, wa, kb, wb, la, lb, tau, cut, 1000, flags)
            exp = model_overlaps_between(ka, wa, kb, wb, la, lb, tau, cut, 1000, flags)
            assert rc == 0 and records.tobytes() == exp[1].tobytes() and (chunks_a == exp[2]).all() and (chunks_b == exp[3]).all()
            assert {k: v for k, v in info.items() if k != "segments"} == exp[4]
            lengths = defaultdict(int)
            for s in segments:
                assert s["length"] >= 1
                lengths[(int(s["src"]), int(s["dst"]))] += int(s["length"])
                same_key += int(la[s["src"]] == lb[s["dst"]])
            forth = {(int(r["src"]), int(r["dst"])): int(r["chunk_pairs"]) for r in records if r["reserved"] == 0}
            back = {(int(r["dst"]), int(r["src"])): int(r["chunk_pairs"]) for r in records if r["reserved"] == 1}
            assert lengths == forth == back
            assert info["segments"] == len(segments) and sum(lengths.values()) == info["chunk_pairs"]
            order = [(int(s["src"]), int(s["dst"]), int(s["first_dst"]) - int(s["first_src"]), int(s["first_src"])) for s in segments]
            assert order == sorted(order) and len(set(order)) == len(order)
            with_segments += len(segments) > 0
            longer += int((segments["length"] > 1).sum())
    assert with_segments > 300 and longer > 100 and same_key > 10


def test_disjoint_tables_equal_the_cross_pairs_of_the_one_table_model():
    """No asset key in both tables: the chunk pairs across the tables are those of the self-join of both tables' rows in one table that
    lie across, with the same ordinals; a pair whose table_a key is the larger has its sides exchanged there."""
    rng = np.random.default_rng(79)
    compared = exchanged = 0
    for _ in range(150):
        (ka, wa, la), (kb, wb, lb) = small_tables(rng, disjoint=True)
        assert not set(ka[:, 0].tolist()) & set(kb[:, 0].tolist())
        both = np.array(sorted(set(la.tolist()) | set(lb.tolist())), dtype=np.uint64)
        in_a = set(la.tolist()) - {1}                                  # (1 is listed on both sides and has no rows)
        for tau in (0, 1):
            segments = model_segments_between(ka, wa, kb, wb, la, lb, tau)[5]
            union = model_segments(np.concatenate([ka, kb]), np.concatenate([wa, wb]), both, tau)[4]
            exp = []
            for s, d, fs, fd, n, h, bs, bd, es, ed in tuples(union):
                key_s, key_d = int(both[s]), int(both[d])
                if (key_s in in_a) == (key_d in in_a):
                    continue                                           # both assets of one table
                if key_s in in_a:
                    exp.append((int(np.searchsorted(la, key_s)), int(np.searchsorted(lb, key_d)), fs, fd, n, h, bs, bd, es, ed))
                else:
                    exp.append((int(np.searchsorted(la, key_d)), int(np.searchsorted(lb, key_s)), fd, fs, n, h, bd, bs, ed, es))
                    exchanged += 1
            exp.sort(key=lambda r: (r[0], r[1], r[3] - r[2], r[2]))
            assert tuples(segments) == exp
            compared += len(exp)
    assert compared > 300 and exchanged > 50
