"""
WHERE the assets of two tables share chunks, on an MI355X: ``isccsearch_join_segments_between`` through
``HipTable.join_segments_between``, and ``find_shared_matches(segments=True)``.

Every case runs on both kernels -- ``forced(engine)`` (``mfma_join_kernel`` in its cross OVERLAP form) and ``valu(engine)``
(``join_scan_kernel``), ONE launch each, the launch counters saying which ran -- and compares records, both chunk arrays, info and
segments for exact byte equality with the host model (``tests/segments_between_model.py``) and with each other; its overlap part is also
compared with a plain ``join_overlaps_between`` of the same tables.  The tables hold planted CLIPS (``clipped_tables``): stretches of an
asset's chunk codes of one table copied into an asset of the other at another position, the rows of both inserted in shuffled order so
that a chunk's ordinal is never its row.  Row counts are those of ``test_gpu_overlaps_between``: each table is held (the one with more
rows) in one case and streamed in the other, so the labels' side bit, not the slot of a hit, has to orient a pair.
"""

import errno

import numpy as np
import pytest

from helpers import make_asset
from iscc_search_amd import _lib
from iscc_search_amd.index import HipIndex, HipOptions
from overlap_between_model import ENOSPC, SKIP_SAME_ASSET, chunk_keys
from segments_between_model import INFO_NAMES, model_segments_between
from test_gpu_join_mfma import counters, dropping, forced, valu
from test_gpu_overlaps_between import SIZES, sp_table
from test_gpu_segments import codes, copied
from test_shared_content import CT, chunks_of, library, rnd
from test_shared_match_segments import LocatedOracleEngine

pytestmark = pytest.mark.gpu

MANY = 10_000_000
GOLD = np.uint64(0x9E3779B97F4A7C15)


def raw_call(engine, ta, tb, max_hamming, keys_a, keys_b, capacity, max_doc_freq=0, dup_limit=1000, flags=SKIP_SAME_ASSET):
    """The C call itself: (rc, records, chunks_a, chunks_b, info array, segments)."""
    keys_a = np.ascontiguousarray(keys_a, dtype=np.uint64)
    keys_b = np.ascontiguousarray(keys_b, dtype=np.uint64)
    records = np.zeros(2 * capacity, dtype=_lib.OVERLAP_DTYPE)
    segments = np.zeros(capacity, dtype=_lib.SEGMENT_DTYPE)
    chunks_a, chunks_b = np.zeros(len(keys_a), dtype=np.uint32), np.zeros(len(keys_b), dtype=np.uint32)
    info = np.zeros(7, dtype=np.uint64)
    rc = engine._lib.isccsearch_join_segments_between(
        engine.handle, ta.id, tb.id, max_hamming, max_doc_freq, dup_limit, len(keys_a), _lib.ptr(keys_a), len(keys_b), _lib.ptr(keys_b), flags,
        capacity, _lib.ptr(records) if capacity else None, _lib.ptr(segments) if capacity else None, _lib.ptr(chunks_a), _lib.ptr(chunks_b),
        _lib.ptr(info))
    return rc, records, chunks_a, chunks_b, info, segments


def same_result(got, exp, what):
    (g_rec, g_a, g_b, g_info, g_seg), (e_rec, e_a, e_b, e_info, e_seg) = got, exp
    assert g_info == e_info, what
    assert g_rec.dtype == e_rec.dtype and g_rec.shape == e_rec.shape and g_rec.tobytes() == e_rec.tobytes(), what + ": records"
    assert np.array_equal(g_a, e_a) and np.array_equal(g_b, e_b), what + ": chunks"
    assert g_seg.dtype == e_seg.dtype and g_seg.shape == e_seg.shape, what + ": segments"
    if g_seg.tobytes() != e_seg.tobytes():
        bad = int(np.nonzero(g_seg != e_seg)[0][0])
        raise AssertionError(f"{what}: segment {bad} of {len(g_seg)} is {g_seg[bad]}, expected {e_seg[bad]}")


def both_kernels(engine, call, exp=None, launches=True):
    """``call()`` on the matrix cores and on the VALU kernel: equal to each other (and to ``exp``), the counters saying which ran."""
    l0, m0 = counters(engine)
    with forced(engine):
        got = call()
    l1, m1 = counters(engine)
    with valu(engine):
        ref = call()
    l2, m2 = counters(engine)
    if launches:
        assert m1 == m0 + 1 and l1 == l0 + 1, "the forced call did not make its one launch on the matrix cores"
        assert m2 == m1 and l2 == l1 + 1, "the join_mfma=0 call did not make its one launch on the VALU kernel"
    else:
        assert (l2, m2) == (l0, m0), "an empty table launched a join kernel"
    same_result(got, ref, "matrix cores against VALU")
    if exp is not None:
        same_result(got, exp, "matrix cores against the model")
    return got


def check(engine, ta, tb, side_a, side_b, max_hamming, max_doc_freq=0, dup_limit=1000, skip=True, launches=True):
    (keys_a, words_a, listed_a), (keys_b, words_b, listed_b) = side_a, side_b
    rc, *exp = model_segments_between(keys_a, words_a, keys_b, words_b, listed_a, listed_b, max_hamming, max_doc_freq, dup_limit,
                                      SKIP_SAME_ASSET if skip else 0)
    assert rc == 0
    got = both_kernels(engine, lambda: ta.join_segments_between(tb, max_hamming, listed_a, listed_b, max_doc_freq, MANY, dup_limit, skip),
                       tuple(exp), launches)
    # the overlap part is what the plain call returns
    p_rec, p_a, p_b, p_info = ta.join_overlaps_between(tb, max_hamming, listed_a, listed_b, max_doc_freq, MANY, dup_limit, skip)
    assert p_rec.tobytes() == got[0].tobytes() and np.array_equal(p_a, got[1]) and np.array_equal(p_b, got[2])
    assert p_info == {k: v for k, v in got[3].items() if k != "segments"}
    return got


def clipped_tables(rng, n_a, n_b, nbytes=8, flips=3):
    """
    ``((keys, words, listed) of A, the same of B, special)``: n_a and n_b chunks of assets that contain clips of assets of the OTHER
    table, rows shuffled.  Words are ``[n, nbytes // 8]``.  From 65 rows per side on both tables hold the core ``check_planted`` looks
    for in the model's output: X, UA (unlisted), W and S in A; Y, UB (unlisted), Z, V and S in B.  On each side the first asset that
    takes a clip takes an exact copy of chunks of a LISTED asset of the other table: a chunk pair at every radius.  Every seventh
    other asset is unlisted, and each side lists an asset (5) that has no rows.
    """
    W = nbytes // 8
    assets = ([], [])                                # per side [(codes [k, 4], places [(offset, size)] or None)]
    names = ({}, {})                                 # per side {name: index in assets}
    if n_a >= 65 and n_b >= 65:
        x, y, v = codes(rng, 12, nbytes), codes(rng, 12, nbytes), codes(rng, 4, nbytes)
        y[0:3] = copied(rng, x[0:3], nbytes, flips)             # a run that starts at ordinal 0 on both sides ...
        y[4:6] = copied(rng, x[4:6], nbytes, flips)             # ... one chunk that does not match, and a second run on the diagonal
        y[7] = x[0]                                             # a code Y holds twice: another diagonal, a run of length 1
        y[10:12] = copied(rng, x[10:12], nbytes, flips)         # a run that ends at the last chunk of both assets
        ua = copied(rng, y[1:4], nbytes, flips)                 # the unlisted asset of A, within the radius of Y's chunks
        ub = copied(rng, x[1:4], nbytes, flips)                 # the unlisted asset of B
        z = copied(rng, x[5:9], nbytes, flips)                  # B: two chunks of equal offset, the ordinals follow (offset, size)
        z[[0, 1]] = z[[1, 0]]                                   # (0, 3) sorts before (0, 9): it is x5's copy
        w = copied(rng, v, nbytes, flips)                       # A: the same against V of B
        w[[0, 1]] = w[[1, 0]]
        s = codes(rng, 5, nbytes)                               # one asset key held by both tables, identical rows
        equal = [(0, 9), (0, 3), (9, 2), (11, 4)]
        shared = [(i * 20, 20) for i in range(5)]
        for side, core in ((0, (("X", x, None), ("UA", ua, None), ("W", w, equal), ("S", s, shared))),
                           (1, (("Y", y, None), ("UB", ub, None), ("Z", z, equal), ("V", v, None), ("S", s.copy(), shared)))):
            for name, c, places in core:
                names[side][name] = len(assets[side])
                assets[side].append((c, places))
    unlisted_at = lambda side, i: i in [at for name, at in names[side].items() if name.startswith("U")] or (i >= len(names[side]) and i > 0 and (i - len(names[side])) % 7 == 3)
    left = [n_a - sum(len(a[0]) for a in assets[0]), n_b - sum(len(a[0]) for a in assets[1])]
    assert min(left) >= 0
    clips = [0, 0]
    while left[0] > 0 or left[1] > 0:
        side = 0 if left[0] * n_b >= left[1] * n_a else 1                      # the side with the larger part of its rows left
        k = min(int(rng.integers(1, 41)), left[side])
        c = codes(rng, k, nbytes)
        other = [a for i, a in enumerate(assets[1 - side]) if clips[side] or not unlisted_at(1 - side, i)]
        if other and (clips[side] == 0 or rng.random() < 0.6) and not unlisted_at(side, len(assets[side])):
            src = other[int(rng.integers(0, len(other)))][0]
            lo = int(rng.integers(0, len(src)))
            clip = copied(rng, src[lo:lo + int(rng.integers(1, 7))], nbytes, flips if clips[side] else 0)[:k]
            at = int(rng.integers(0, k - len(clip) + 1))
            c[at:at + len(clip)] = clip
            clips[side] += 1
        assets[side].append((c, None))
        left[side] -= k
    n_ids = len(assets[0]) + len(assets[1])
    ids = (rng.choice(np.arange(1, 10 * n_ids + 10, dtype=np.uint64), size=n_ids, replace=False) * GOLD).tolist()
    sides, special = [], {}
    for side, n in ((0, n_a), (1, n_b)):
        mine = [ids.pop() for _ in assets[side]]
        if "S" in names[side]:
            mine[names[side]["S"]] = special.setdefault("S", mine[names[side]["S"]])
        row_assets, offsets, sizes, words = [], [], [], []
        for a, (c, places) in zip(mine, assets[side]):
            if places is None:
                size = rng.integers(1, 1000, size=len(c))
                places = list(zip((np.cumsum(size) - size).tolist(), size.tolist()))
            row_assets += [a] * len(c)
            offsets += [p[0] for p in places]
            sizes += [p[1] for p in places]
            words.append(c)
        order = rng.permutation(n)
        keys = chunk_keys(np.array(row_assets, dtype=np.uint64)[order], np.array(offsets)[order], np.array(sizes)[order])
        words = np.concatenate(words)[order][:, :W]
        unlisted = {a for i, a in enumerate(mine) if unlisted_at(side, i)}
        listed = np.array(sorted((set(mine) - unlisted) | {5}), dtype=np.uint64)              # 5: a listed asset without rows
        special.update({name: mine[i] for name, i in names[side].items()})
        sides.append((keys, words, listed))
    return sides[0], sides[1], special


def check_planted(side_a, side_b, special, flips):
    """What every pair of tables of 65 rows or more per side has to contain, looked up in the MODEL's output: a degenerate pair fails here."""
    (ka, wa, la), (kb, wb, lb) = side_a, side_b
    rc, _, chunks_a, chunks_b, info, seg = model_segments_between(ka, wa, kb, wb, la, lb, flips)
    assert rc == 0
    label_a = {int(a): i for i, a in enumerate(la.tolist())}
    label_b = {int(a): i for i, a in enumerate(lb.tolist())}
    s = {f: seg[f].astype(np.int64) for f in seg.dtype.names}
    diagonal = s["first_dst"] - s["first_src"]
    xy = (s["src"] == label_a[special["X"]]) & (s["dst"] == label_b[special["Y"]])
    assert bool((xy & (s["first_src"] == 0) & (s["first_dst"] == 0)).any()), "no run starts at ordinal 0"
    ends = (s["first_src"] + s["length"] == chunks_a[s["src"]]) & (s["first_dst"] + s["length"] == chunks_b[s["dst"]])
    assert bool((xy & ends).any()), "no run ends at the last chunk of both assets"
    same = (s["src"][1:] == s["src"][:-1]) & (s["dst"][1:] == s["dst"][:-1]) & (diagonal[1:] == diagonal[:-1])
    assert bool((xy[1:] & same & (s["first_src"][1:] == s["first_src"][:-1] + s["length"][:-1] + 1)).any()), "no two runs one chunk apart on a diagonal"
    assert len(set(diagonal[xy].tolist())) >= 2, "X and Y do not meet on two diagonals"
    assert bool((xy & (s["length"] == 1)).any()), "no run of length 1"
    # the unlisted assets' rows are within the radius of the other table's and take no part
    for unlisted, own, (keys, words), against, (o_keys, o_words) in (("UA", label_a, (ka, wa), "Y", (kb, wb)), ("UB", label_b, (kb, wb), "X", (ka, wa))):
        assert special[unlisted] not in own
        rows_u, rows_o = words[keys[:, 0] == special[unlisted]], o_words[o_keys[:, 0] == special[against]]
        dist = np.bitwise_count(rows_u[:, None, :] ^ rows_o[None, :, :]).sum(axis=2)
        assert len(rows_u) == 3 and int((dist <= flips).sum()) >= 3, "an unlisted asset matches nothing"
    # Z of B and W of A: two chunks at offset 0; the four chunks are one run only if ordinals follow (offset, size) in their own table
    for name, keys in (("Z", kb), ("W", ka)):
        places = keys[keys[:, 0] == special[name], 1]
        assert sorted((int(p) >> 32, int(p) & 0xFFFFFFFF) for p in places.tolist())[:2] == [(0, 3), (0, 9)]
    xz = (s["src"] == label_a[special["X"]]) & (s["dst"] == label_b[special["Z"]]) & (s["length"] == 4) & (s["first_src"] == 5) & (s["first_dst"] == 0)
    wv = (s["src"] == label_a[special["W"]]) & (s["dst"] == label_b[special["V"]]) & (s["length"] == 4) & (s["first_src"] == 0) & (s["first_dst"] == 0)
    assert bool(xz.any()) and bool(wv.any()), "the chunks of equal offset are not in one run"
    # S: one asset key in both tables, identical rows -- no pair with the flag, one run of all its chunks without
    rows = lambda keys, words: sorted((int(k[1]), tuple(w)) for k, w in zip(keys[keys[:, 0] == special["S"]].tolist(), words[keys[:, 0] == special["S"]].tolist()))
    assert len(rows(ka, wa)) == 5 and rows(ka, wa) == rows(kb, wb)
    ss = (s["src"] == label_a[special["S"]]) & (s["dst"] == label_b[special["S"]])
    assert not bool(ss.any()), "the flag did not keep the shared asset from pairing with itself"
    every = model_segments_between(ka, wa, kb, wb, la, lb, flips, flags=0)[5]
    mine = every[(every["src"] == label_a[special["S"]]) & (every["dst"] == label_b[special["S"]])]
    assert [tuple(int(v) for v in r) for r in mine.tolist()] == [(label_a[special["S"]], label_b[special["S"]], 0, 0, 5, 0, 0, 0, 100, 100)]
    return info


@pytest.mark.parametrize("n_a,n_b", SIZES)
def test_simprints64(hip_engine, n_a, n_b):
    rng = np.random.default_rng(1000 * n_a + n_b)
    side_a, side_b, special = clipped_tables(rng, n_a, n_b)
    if special:
        check_planted(side_a, side_b, special, 3)
    with dropping(sp_table(hip_engine, 8, *side_a[:2]), sp_table(hip_engine, 8, *side_b[:2])) as (ta, tb):
        for tau in (0, 3):
            *_, skipped, seg = check(hip_engine, ta, tb, side_a, side_b, tau, skip=True)
            *_, every, _ = check(hip_engine, ta, tb, side_a, side_b, tau, skip=False)
            assert skipped["chunk_pairs"] >= 1 and skipped["segments"] >= 1
            if special:
                assert every["chunk_pairs"] >= skipped["chunk_pairs"] + 5 and every["segments"] > skipped["segments"]
        assert int(seg["length"].max()) >= (3 if special else 1)


@pytest.mark.parametrize("nbytes,flips", [(16, 7), (32, 9)])
def test_simprints128_and_256(hip_engine, nbytes, flips):
    rng = np.random.default_rng(nbytes)
    side_a, side_b, special = clipped_tables(rng, 3000, 2500, nbytes, flips)
    check_planted(side_a, side_b, special, flips)
    with dropping(sp_table(hip_engine, nbytes, *side_a[:2]), sp_table(hip_engine, nbytes, *side_b[:2])) as (ta, tb):
        for max_hamming in (0, flips):
            *_, info, _ = check(hip_engine, ta, tb, side_a, side_b, max_hamming)
            assert info["segments"] >= 1
        check(hip_engine, tb, ta, side_b, side_a, flips, skip=False)        # the sides exchanged: table A is the streamed one


def tuples(segments):
    return [tuple(int(v) for v in s) for s in segments.tolist()]


def table(rng, rows):
    """(keys, words) of rows (asset, offset, size, code) in shuffled order."""
    order = rng.permutation(len(rows))
    return (chunk_keys([rows[i][0] for i in order], [rows[i][1] for i in order], [rows[i][2] for i in order]),
            np.array([[rows[i][3]] for i in order], dtype=np.uint64))


def test_a_stop_chunk_of_one_table_inside_a_clip_splits_the_run(hip_engine):
    rng = np.random.default_rng(4)
    x = [int(v) for v in rng.integers(0, 2**63, size=8)]
    # x[3] is held by six assets of A and by one of B: a stop chunk in A alone
    ka, wa = table(rng, [(1, i, 4, x[i]) for i in range(8)] + [(a, 0, 4, x[3]) for a in range(3, 8)])
    kb, wb = table(rng, [(2, 10 + i, 4, x[i]) for i in range(8)])
    side_a, side_b = (ka, wa, np.array([1, 3, 4, 5, 6, 7], dtype=np.uint64)), (kb, wb, np.array([2], dtype=np.uint64))
    with dropping(sp_table(hip_engine, 8, ka, wa), sp_table(hip_engine, 8, kb, wb)) as (ta, tb):
        *_, info, seg = check(hip_engine, ta, tb, side_a, side_b, 0, max_doc_freq=5)
        assert info["stop_chunks_a"] == 6 and info["stop_chunks_b"] == 0
        # the ordinals still count the stop chunk: the second run starts at chunk 4 of either asset
        assert tuples(seg) == [(0, 0, 0, 0, 3, 0, 0, 10, 6, 16), (0, 0, 4, 4, 4, 0, 4, 14, 11, 21)]
        *_, info, seg = check(hip_engine, ta, tb, side_a, side_b, 0, max_doc_freq=6)
        assert info["stop_chunks_a"] == 0 and tuples(seg)[0] == (0, 0, 0, 0, 8, 0, 0, 10, 11, 21)
        # the sides exchanged: the chunk is a stop chunk of the table that is now B (and still the held one)
        *_, info, seg = check(hip_engine, tb, ta, side_b, side_a, 0, max_doc_freq=5)
        assert info["stop_chunks_b"] == 6 and tuples(seg) == [(0, 0, 0, 0, 3, 0, 10, 0, 16, 6), (0, 0, 4, 4, 4, 0, 14, 4, 21, 11)]


def test_removed_rows_close_the_ordinals_up_in_one_table(hip_engine):
    rng = np.random.default_rng(2)
    side_a, side_b, _ = clipped_tables(rng, 3000, 2500)
    (ka, wa, la), (kb, wb, lb) = side_a, side_b
    with dropping(sp_table(hip_engine, 8, ka, wa), sp_table(hip_engine, 8, kb, wb)) as (ta, tb):
        *_, before = check(hip_engine, ta, tb, side_a, side_b, 3)
        first = int(np.nonzero(np.isin(ka[:, 0], la))[0][0])                    # a row of a listed asset, kept to the end
        gone = rng.choice(np.setdiff1d(np.arange(3000), [first]), size=900, replace=False)      # now A is the smaller, streamed table
        assert ta.remove(ka[gone]) == 900
        keep = np.setdiff1d(np.arange(3000), gone)
        *_, info, after = check(hip_engine, ta, tb, (ka[keep], wa[keep], la), side_b, 3)
        assert info["segments"] > 0 and info["live_rows_a"] <= len(keep)
        # chunks inside clips went: runs were cut, and what lies behind a removed chunk of A moved down; B's ordinals stayed
        assert int(before["length"].sum()) > int(after["length"].sum()) and int(after["length"].max()) >= 2
        assert after.tobytes() != before[: len(after)].tobytes()
        ta.remove(ka[keep[keep != first]])                                      # one row: still a launch
        one = (ka[first:first + 1], wa[first:first + 1], la)
        rec, chunks_a, _, info, seg = check(hip_engine, ta, tb, one, side_b, 64, skip=False)
        assert info["live_rows_a"] == 1 and info["chunk_pairs"] == info["live_rows_b"] == info["segments"] and int(chunks_a.sum()) == 1
        assert bool(np.all(seg["length"] == 1)) and bool(np.all(seg["first_src"] == 0))
        ta.remove(one[0])                                                       # empty: nothing launched, chunks and info still filled
        empty = (ka[:0], wa[:0], la)
        rec, chunks_a, chunks_b, info, seg = check(hip_engine, ta, tb, empty, side_b, 64, launches=False)
        assert len(rec) == 0 and len(seg) == 0 and int(chunks_a.sum()) == 0
        assert info["chunk_pairs"] == info["segments"] == 0 and info["live_rows_a"] == 0 and info["live_rows_b"] == int(chunks_b.sum()) > 0
        rec, _, _, info, seg = check(hip_engine, tb, ta, side_b, empty, 64, max_doc_freq=5, launches=False)
        assert len(rec) == 0 and len(seg) == 0 and info["live_rows_a"] > 0 and info["live_rows_b"] == 0


def test_ends_pass_32_bits(hip_engine):
    a, b = 0x0123456789ABCDEF, 0xFEDCBA9876543210
    ka = chunk_keys([1, 1], [0xFFFFFF00, 0xFFFFFE00], [0x1000, 0x100])
    kb = chunk_keys([2, 2], [0, 0xFFFFFF00], [8, 0x2000])
    wa, wb = np.array([[b], [a]], dtype=np.uint64), np.array([[a], [b]], dtype=np.uint64)
    side_a, side_b = (ka, wa, np.array([1], dtype=np.uint64)), (kb, wb, np.array([2], dtype=np.uint64))
    with dropping(sp_table(hip_engine, 8, ka, wa), sp_table(hip_engine, 8, kb, wb)) as (ta, tb):
        *_, seg = check(hip_engine, ta, tb, side_a, side_b, 0)
        assert tuples(seg) == [(0, 0, 0, 0, 2, 0, 0xFFFFFE00, 0, 0x100000F00, 0x100001F00)]
        *_, seg = check(hip_engine, tb, ta, side_b, side_a, 0)
        assert tuples(seg) == [(0, 0, 0, 0, 2, 0, 0, 0xFFFFFE00, 0x100001F00, 0x100000F00)]


def test_capacity_is_exact_on_both_kernels(hip_engine):
    rng = np.random.default_rng(9)
    side_a, side_b, _ = clipped_tables(rng, 1500, 1100)
    (ka, wa, la), (kb, wb, lb) = side_a, side_b
    rc, *exp = model_segments_between(ka, wa, kb, wb, la, lb, 3)
    total = exp[3]["chunk_pairs"]
    assert total > 100
    assert model_segments_between(ka, wa, kb, wb, la, lb, 3, capacity=total - 1)[0] == ENOSPC
    with dropping(sp_table(hip_engine, 8, ka, wa), sp_table(hip_engine, 8, kb, wb)) as (ta, tb):
        for option in (forced, valu):
            with option(hip_engine):
                rc, _, _, _, info, _ = raw_call(hip_engine, ta, tb, 3, la, lb, total - 1)
                assert rc == -errno.ENOSPC and int(info[0]) == total
                assert "capacity" in hip_engine._lib.isccsearch_last_error().decode()
                rc, _, _, _, info, _ = raw_call(hip_engine, ta, tb, 3, la, lb, 0)
                assert rc == -errno.ENOSPC and int(info[0]) == total
                rc, rec, chunks_a, chunks_b, info, seg = raw_call(hip_engine, ta, tb, 3, la, lb, total)
                assert rc == 0
                same_result((rec[: int(info[1])], chunks_a, chunks_b, dict(zip(INFO_NAMES, info.tolist())), seg[: int(info[6])]), tuple(exp),
                            "capacity == total")
        with pytest.raises(ValueError, match="exceed max_pairs"):
            ta.join_segments_between(tb, 3, la, lb, 0, total - 1)
        same_result(ta.join_segments_between(tb, 3, la, lb, 0, total), tuple(exp), "max_pairs == total")


def test_refused_arguments_leave_the_outputs_untouched(hip_engine):
    words = np.array([[5], [5], [6]], dtype=np.uint64)
    call = hip_engine._lib.isccsearch_join_segments_between
    last_error = lambda: hip_engine._lib.isccsearch_last_error().decode()
    with dropping(sp_table(hip_engine, 8, chunk_keys([1, 2, 3]), words), sp_table(hip_engine, 8, chunk_keys([4, 5, 6]), words),
                  hip_engine.open_table(_lib.METRIC_HAMMING, 1, 8), hip_engine.open_table(_lib.METRIC_NPHD, 1, 32),
                  hip_engine.open_table(_lib.METRIC_HAMMING, 2, 16)) as (ta, tb, t_kw1, t_nphd, t_wide):
        t_kw1.add(np.array([1, 2], dtype=np.uint64), words[:2])
        good_a, good_b = np.array([1, 2, 3], dtype=np.uint64), np.array([4, 5, 6], dtype=np.uint64)
        records = np.full(16, 0xEE, dtype=np.uint8).repeat(32).view(_lib.OVERLAP_DTYPE)
        segments = np.full(8, 0xEE, dtype=np.uint8).repeat(48).view(_lib.SEGMENT_DTYPE)
        chunks_a, chunks_b = np.full(3, 0xEEEEEEEE, dtype=np.uint32), np.full(3, 0xEEEEEEEE, dtype=np.uint32)
        info = np.full(7, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
        P = _lib.ptr
        base = dict(h=hip_engine.handle, table_a=ta.id, table_b=tb.id, max_hamming=0, max_doc_freq=0, dup_limit=1000, n_assets_a=3, asset_keys_a=P(good_a),
                    n_assets_b=3, asset_keys_b=P(good_b), flags=1, capacity=4, out_pairs=P(records), out_segments=P(segments), out_chunks_a=P(chunks_a),
                    out_chunks_b=P(chunks_b), out_info=P(info))
        unsorted, repeated = np.array([1, 3, 2], dtype=np.uint64), np.array([4, 5, 5], dtype=np.uint64)
        cases = [
            (dict(h=None), -errno.EINVAL, "handle"),
            (dict(asset_keys_a=None), -errno.EINVAL, "NULL"),
            (dict(asset_keys_b=None), -errno.EINVAL, "NULL"),
            (dict(out_chunks_a=None), -errno.EINVAL, "NULL"),
            (dict(out_chunks_b=None), -errno.EINVAL, "NULL"),
            (dict(out_info=None), -errno.EINVAL, "NULL"),
            (dict(out_pairs=None), -errno.EINVAL, "out_pairs"),
            (dict(out_segments=None), -errno.EINVAL, "out_segments"),
            (dict(table_b=ta.id), -errno.EINVAL, "isccsearch_join_overlaps joins a table with itself"),
            (dict(table_a=t_kw1.id), -errno.EINVAL, f"table {t_kw1.id} has"),
            (dict(table_b=t_kw1.id), -errno.EINVAL, "key_words"),
            (dict(table_b=t_nphd.id), -errno.EINVAL, "HAMMING"),
            (dict(table_b=t_wide.id), -errno.EINVAL, "max_bytes"),
            (dict(n_assets_a=0), -errno.EINVAL, "n_assets_a"),
            (dict(n_assets_a=1 << 31), -errno.EINVAL, "n_assets_a"),
            (dict(n_assets_b=0), -errno.EINVAL, "n_assets_b"),
            (dict(n_assets_b=1 << 31), -errno.EINVAL, "n_assets_b"),
            (dict(asset_keys_a=P(unsorted)), -errno.EINVAL, "asset_keys_a[2]"),
            (dict(asset_keys_b=P(repeated)), -errno.EINVAL, "asset_keys_b[2]"),
            (dict(max_hamming=-1), -errno.EINVAL, "max_hamming"),
            (dict(max_doc_freq=11, dup_limit=10), -errno.EINVAL, "dup_limit"),
            (dict(flags=3), -errno.EINVAL, "flags"),
            (dict(capacity=1 << 31), -errno.E2BIG, "32 bits"),
        ]
        before = counters(hip_engine), hip_engine.stats()["freq_builds"]
        for change, want, word in cases:
            args = dict(base, **change)
            rc = call(*args.values())
            assert rc == want and word in last_error(), (change, rc, last_error())
            untouched = all(bool(np.all(x.view(np.uint8) == 0xEE)) for x in (records, segments, chunks_a, chunks_b, info))
            assert untouched, change
        assert (counters(hip_engine), hip_engine.stats()["freq_builds"]) == before
        with pytest.raises(ValueError, match="another engine"):
            ta.join_segments_between(object(), 0, good_a, good_b, 0, 10)
        # what is allowed: both outputs NULL with capacity 0 (here -ENOSPC: codes 5, 5, 6 on either side give 5 chunk pairs), no flag,
        # max_doc_freq == dup_limit
        assert call(*dict(base, capacity=0, out_pairs=None, out_segments=None).values()) == -errno.ENOSPC and int(info[0]) == 5
        assert call(*dict(base, capacity=8, flags=0, max_doc_freq=10, dup_limit=10).values()) == 0
        assert info.tolist() == [5, 10, 3, 0, 3, 0, 5] and chunks_a.tolist() == [1, 1, 1] and chunks_b.tolist() == [1, 1, 1]
        # every asset has one chunk: five runs of one pair, (label a, label b, ordinals 0 and 0, 1, 0, the chunk's offset and end on either side)
        assert tuples(segments[:5]) == [(0, 0, 0, 0, 1, 0, 0, 0, 1, 1), (0, 1, 0, 0, 1, 0, 0, 1, 1, 2), (1, 0, 0, 0, 1, 0, 1, 0, 2, 1),
                                        (1, 1, 0, 0, 1, 0, 1, 1, 2, 2), (2, 2, 0, 0, 1, 0, 2, 2, 3, 3)]


def test_default_dispatch_small_tables_stay_on_the_valu_kernel(hip_engine):
    rng = np.random.default_rng(22)
    side_a, side_b, special = clipped_tables(rng, 5000, 5000)
    (ka, wa, la), (kb, wb, lb) = side_a, side_b
    with dropping(sp_table(hip_engine, 8, ka, wa), sp_table(hip_engine, 8, kb, wb)) as (ta, tb):
        l0, m0 = counters(hip_engine)
        with hip_engine.options(mfma=1, join_mfma=1):
            got = ta.join_segments_between(tb, 3, la, lb, 0, MANY)
        l1, m1 = counters(hip_engine)
        assert m1 == m0 and l1 == l0 + 1
        rc, *exp = model_segments_between(ka, wa, kb, wb, la, lb, 3)
        same_result(got, tuple(exp), "default dispatch against the model")


def test_find_shared_matches_end_to_end(hip_engine):
    """Two libraries of about 300 assets and 3 000 chunks each, dealt alternately from one generated library, and a clip of ten chunks
    whose fifth chunk was replaced in the other library's copy: ``max_gap=1`` makes one segment of its two runs.  The device result on
    both kernels equals the model-backed one of ``test_shared_match_segments``."""
    rng = np.random.default_rng(31)
    assets = library(rng, 600, chunks=(4, 14))
    assets_a, assets_b = assets[0::2], assets[1::2]
    clip = [rnd(rng) for _ in range(10)]
    assets_a.append(make_asset(rng, 600, simprints={CT: chunks_of(clip)}))
    assets_b.append(make_asset(rng, 601, simprints={CT: chunks_of([rnd(rng)] + clip[:4] + [rnd(rng)] + clip[5:])}))
    cpu_engine = LocatedOracleEngine()
    cpu_a, cpu_b = HipIndex(cpu_engine, HipOptions()), HipIndex(cpu_engine, HipOptions())
    cpu_a.add_assets(assets_a)
    cpu_b.add_assets(assets_b)
    exp = cpu_a.find_shared_matches(cpu_b, max_doc_freq=0, segments=True, max_gap=1)
    a, b = HipIndex(hip_engine, HipOptions()), HipIndex(hip_engine, HipOptions())
    try:
        a.add_assets(assets_a)
        b.add_assets(assets_b)
        assert 2500 < a._sp_tables[CT].size < _lib.MAX_K and 2500 < b._sp_tables[CT].size < _lib.MAX_K
        _, m0 = counters(hip_engine)
        with forced(hip_engine):
            got = a.find_shared_matches(b, max_doc_freq=0, segments=True, max_gap=1)
        _, m1 = counters(hip_engine)
        with valu(hip_engine):
            ref = a.find_shared_matches(b, max_doc_freq=0, segments=True, max_gap=1)
        assert m1 == m0 + 1 and counters(hip_engine)[1] == m1
        assert len(got) > 100 and got == exp and ref == exp
        runs = [s for p in got for t in p.types.values() for s in t.segments]
        assert max(s.chunks for s in runs) >= 4 and any(s.span == 10 and s.chunks == 9 for s in runs)
        kwargs = dict(min_chunks=2, max_doc_freq=5, segments=True, min_segment=2)
        assert b.find_shared_matches(a, **kwargs) == cpu_b.find_shared_matches(cpu_a, **kwargs)
        # segments=False stays the call it was
        assert a.find_shared_matches(b, max_doc_freq=0) == cpu_a.find_shared_matches(cpu_b, max_doc_freq=0)
    finally:
        a.close()
        b.close()
