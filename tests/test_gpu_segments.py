"""
WHERE assets share chunks, on an MI355X: ``isccsearch_join_segments`` through ``HipTable.join_segments``, and
``find_shared_content(segments=True)``.

Every case runs on both kernels -- ``forced(engine)`` (``mfma_join_kernel``) and ``valu(engine)`` (``join_scan_kernel``), the launch
counters saying which ran -- and compares records, chunks, info and segments for exact byte equality with the host model
(``tests/segments_model.py``) and with each other; its overlap part is also compared with a plain ``join_overlaps`` of the same table.
The tables hold planted CLIPS (``clipped``): stretches of one asset's chunk codes copied into another asset at another position, the
rows inserted in shuffled order so that a chunk's ordinal is not its row.  Row counts are those of ``test_gpu_overlaps``: the shapes
at which the two emit paths change behaviour.
"""

import errno

import numpy as np
import pytest

from iscc_search_amd import _lib
from iscc_search_amd.index import HipIndex, HipOptions
from overlap_model import ENOSPC, chunk_keys
from segments_model import INFO_NAMES, model_segments
from test_gpu_duplicates import table_with
from test_gpu_join_mfma import N_TWO_BLOCKS, counters, dropping, forced, valu
from helpers import make_asset
from test_shared_content import CT, chunks_of, library, rnd
from test_shared_segments import cpu_index

pytestmark = pytest.mark.gpu

MANY = 10_000_000
GOLD = np.uint64(0x9E3779B97F4A7C15)


def sp_table(engine, nbytes, keys, words):
    return table_with(engine, _lib.METRIC_HAMMING, 2, nbytes, keys, words, None)


def raw_call(engine, t, max_hamming, asset_keys, capacity, max_doc_freq=0, dup_limit=1000):
    """The C call itself: (rc, records, chunks, info array, segments)."""
    asset_keys = np.ascontiguousarray(asset_keys, dtype=np.uint64)
    records = np.zeros(2 * capacity, dtype=_lib.OVERLAP_DTYPE)
    segments = np.zeros(capacity, dtype=_lib.SEGMENT_DTYPE)
    chunks = np.zeros(len(asset_keys), dtype=np.uint32)
    info = np.zeros(5, dtype=np.uint64)
    rc = engine._lib.isccsearch_join_segments(engine.handle, t.id, max_hamming, max_doc_freq, dup_limit, len(asset_keys), _lib.ptr(asset_keys),
                                              capacity, _lib.ptr(records) if capacity else None, _lib.ptr(segments) if capacity else None,
                                              _lib.ptr(chunks), _lib.ptr(info))
    return rc, records, chunks, info, segments


def same_result(got, exp, what):
    (g_rec, g_chunks, g_info, g_seg), (e_rec, e_chunks, e_info, e_seg) = got, exp
    assert g_info == e_info, what
    assert g_rec.dtype == e_rec.dtype and g_rec.shape == e_rec.shape and g_rec.tobytes() == e_rec.tobytes(), what + ": records"
    assert np.array_equal(g_chunks, e_chunks), what + ": chunks"
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
        assert m1 > m0 and l1 - l0 == m1 - m0, "the forced call did not run on the matrix cores alone"
        assert m2 == m1 and l2 > l1, "the join_mfma=0 call did not run on the VALU kernel alone"
    else:
        assert (l2, m2) == (l0, m0), "a table without a pair of rows launched a join kernel"
    same_result(got, ref, "matrix cores against VALU")
    if exp is not None:
        same_result(got, exp, "matrix cores against the model")
    return got


def check(engine, t, keys, words, asset_keys, max_hamming, max_doc_freq=0, dup_limit=1000, launches=True):
    rc, rec, chunks, info, segments = model_segments(keys, words, asset_keys, max_hamming, max_doc_freq, dup_limit)
    assert rc == 0
    got = both_kernels(engine, lambda: t.join_segments(max_hamming, asset_keys, max_doc_freq, MANY, dup_limit), (rec, chunks, info, segments), launches)
    # the overlap part is what the plain call returns
    p_rec, p_chunks, p_info = t.join_overlaps(max_hamming, asset_keys, max_doc_freq, MANY, dup_limit)
    assert p_rec.tobytes() == got[0].tobytes() and np.array_equal(p_chunks, got[1]) and p_info == {k: v for k, v in got[2].items() if k != "segments"}
    return got


def codes(rng, k, nbytes):
    """k random codes of nbytes bytes as [k, 4] words, zero past the code."""
    w = rng.integers(0, 2**64, size=(k, 4), dtype=np.uint64)
    w[:, (nbytes + 7) // 8:] = 0
    return w


def copied(rng, w, nbytes, flips):
    """Copies of the codes w with at most ``flips`` bits changed each."""
    w = w.copy()
    for i in range(len(w)):
        for bit in rng.choice(8 * nbytes, size=int(rng.integers(0, flips + 1)), replace=False).tolist():
            w[i, bit // 64] ^= np.uint64(1) << np.uint64(bit % 64)
    return w


def clipped(rng, n, nbytes=8, flips=3):
    """
    ``(keys, words, asset_keys, special)``: n chunks of assets that contain clips of each other, rows shuffled.  From 65 rows on the
    table holds the core assets X, Y, U (unlisted) and Z, which ``check_planted`` looks for in the model's output.
    """
    assets = []                                     # [(codes [k, 4], places [(offset, size)] or None)]
    special = {}
    if n >= 65:
        x = codes(rng, 12, nbytes)
        y = codes(rng, 12, nbytes)
        y[0:3] = copied(rng, x[0:3], nbytes, flips)             # a run that starts at ordinal 0 ...
        y[4:6] = copied(rng, x[4:6], nbytes, flips)             # ... one chunk that does not match, and a second run on the diagonal
        y[7] = x[0]                                             # a code Y holds twice: another diagonal, a run of length 1
        y[10:12] = copied(rng, x[10:12], nbytes, flips)         # a run that ends at the last chunk of both assets
        u = copied(rng, x[1:4], nbytes, flips)                  # the unlisted asset
        z = copied(rng, x[5:9], nbytes, flips)                  # two chunks of equal offset: the ordinals follow (offset, size)
        assets += [(x, None), (y, None), (u, None), (z, [(0, 9), (0, 3), (9, 2), (11, 4)])]
        z[[0, 1]] = z[[1, 0]]                                   # (0, 3) sorts before (0, 9): it is x5's copy
    elif n >= 4:
        p = codes(rng, n // 2, nbytes)
        q = codes(rng, n - n // 2, nbytes)
        q[: len(p)] = copied(rng, p, nbytes, flips)
        q[len(p) // 2] = codes(rng, 1, nbytes)[0]
        assets += [(p, None), (q, None)]
    else:
        p = codes(rng, 1, nbytes)
        assets += [(p, None)] + [(p.copy(), None) for _ in range(n - 1)]
    left = n - sum(len(a[0]) for a in assets)
    while left > 0:
        k = min(int(rng.integers(1, 41)), left)
        w = codes(rng, k, nbytes)
        if rng.random() < 0.6:
            src = assets[int(rng.integers(0, len(assets)))][0]
            lo = int(rng.integers(0, len(src)))
            clip = copied(rng, src[lo:lo + int(rng.integers(1, 7))], nbytes, flips)[:k]
            at = int(rng.integers(0, k - len(clip) + 1))
            w[at:at + len(clip)] = clip
        assets.append((w, None))
        left -= k
    ids = rng.choice(np.arange(1, 10 * len(assets) + 10, dtype=np.uint64), size=len(assets), replace=False) * GOLD
    row_assets, offsets, sizes, words = [], [], [], []
    for a, (w, places) in zip(ids.tolist(), assets):
        if places is None:
            size = rng.integers(1, 1000, size=len(w))
            places = list(zip((np.cumsum(size) - size).tolist(), size.tolist()))
        row_assets += [a] * len(w)
        offsets += [p[0] for p in places]
        sizes += [p[1] for p in places]
        words.append(w)
    order = rng.permutation(n)
    keys = chunk_keys(np.array(row_assets, dtype=np.uint64)[order], np.array(offsets)[order], np.array(sizes)[order])
    words = np.concatenate(words)[order]
    unlisted = {int(ids[2])} if n >= 65 else set()
    unlisted |= {int(a) for i, a in enumerate(ids.tolist()) if i >= 4 and i % 7 == 3}
    asset_keys = np.array(sorted((set(ids.tolist()) - unlisted) | {5}), dtype=np.uint64)      # 5: a listed asset without rows
    if n >= 65:
        special = {name: int(ids[i]) for i, name in enumerate("XYUZ")}
    return keys, words, asset_keys, special


def check_planted(keys, words, asset_keys, special, nbytes, flips):
    """What the issue wants every table of 65 rows or more to contain, looked up in the MODEL's output: a degenerate table fails here."""
    W = (nbytes + 7) // 8
    rc, _, chunks, info, seg = model_segments(keys, words[:, :W], asset_keys, flips)
    assert rc == 0
    label = {int(a): i for i, a in enumerate(asset_keys.tolist())}
    x, y, z = label[special["X"]], label[special["Y"]], label[special["Z"]]
    s = {f: seg[f].astype(np.int64) for f in seg.dtype.names}
    diagonal = s["first_dst"] - s["first_src"]
    assert bool((s["length"] == 1).any()), "no run of length 1"
    assert bool(((s["first_src"] == 0) | (s["first_dst"] == 0)).any()), "no run starts at ordinal 0"
    assert bool(((s["first_src"] + s["length"] == chunks[s["src"]]) | (s["first_dst"] + s["length"] == chunks[s["dst"]])).any()), "no run ends at a last chunk"
    same = (s["src"][1:] == s["src"][:-1]) & (s["dst"][1:] == s["dst"][:-1]) & (diagonal[1:] == diagonal[:-1])
    assert bool((same & (s["first_src"][1:] == s["first_src"][:-1] + s["length"][:-1] + 1)).any()), "no two runs one chunk apart on a diagonal"
    xy = (s["src"] == min(x, y)) & (s["dst"] == max(x, y))
    assert len(set(diagonal[xy].tolist())) >= 2, "X and Y do not meet on two diagonals"
    # the unlisted asset's rows are within the radius of X's and take no part
    assert special["U"] not in label
    rows_u, rows_x = words[keys[:, 0] == special["U"]][:, :W], words[keys[:, 0] == special["X"]][:, :W]
    dist = np.bitwise_count(rows_u[:, None, :] ^ rows_x[None, :, :]).sum(axis=2)
    assert int((dist <= flips).sum()) >= 3, "the unlisted asset matches nothing"
    # Z: two chunks at offset 0; its four chunks are one run against X's chunks 5..8 only if ordinals follow (offset, size)
    places = keys[keys[:, 0] == special["Z"], 1]
    assert sorted((int(p) >> 32, int(p) & 0xFFFFFFFF) for p in places.tolist())[:2] == [(0, 3), (0, 9)]
    xz = (s["src"] == min(x, z)) & (s["dst"] == max(x, z)) & (s["length"] == 4)
    assert bool(xz.any()), "Z's four chunks are not one run"
    return info


@pytest.mark.parametrize("n", [2, 17, 65, 1025, 2049, N_TWO_BLOCKS])
def test_simprints64(hip_engine, n):
    rng = np.random.default_rng(n)
    keys, words, asset_keys, special = clipped(rng, n)
    if n >= 65:
        check_planted(keys, words, asset_keys, special, 8, 3)
    with dropping(sp_table(hip_engine, 8, keys, words)) as (t,):
        for tau in (0, 3):
            _, _, info, segments = check(hip_engine, t, keys, words[:, :1], asset_keys, tau)
            assert info["chunk_pairs"] >= 1 and info["segments"] >= 1
        assert int(segments["length"].max()) >= min(n, 3) - 1


@pytest.mark.parametrize("nbytes,flips", [(16, 7), (32, 9)])
def test_simprints128_and_256(hip_engine, nbytes, flips):
    rng = np.random.default_rng(nbytes)
    keys, words, asset_keys, special = clipped(rng, 3000, nbytes, flips)
    check_planted(keys, words, asset_keys, special, nbytes, flips)
    with dropping(sp_table(hip_engine, nbytes, keys, words)) as (t,):
        for max_hamming in (0, flips):
            _, _, info, _ = check(hip_engine, t, keys, words[:, : nbytes // 8], asset_keys, max_hamming)
            assert info["segments"] >= 1


def test_a_stop_chunk_inside_a_clip_splits_the_run(hip_engine):
    rng = np.random.default_rng(4)
    x = codes(rng, 8, 8)
    boiler = x[3].copy()
    rows = [(1, i, x[i]) for i in range(8)] + [(2, 10 + i, x[i]) for i in range(8)]
    rows += [(a, 0, boiler) for a in range(3, 8)] + [(a, 1, codes(rng, 1, 8)[0]) for a in range(3, 8)]
    order = rng.permutation(len(rows))
    keys = chunk_keys([rows[i][0] for i in order], [rows[i][1] for i in order], [4] * len(rows))
    words = np.array([rows[i][2] for i in order], dtype=np.uint64)
    asset_keys = np.arange(1, 8, dtype=np.uint64)
    with dropping(sp_table(hip_engine, 8, keys, words)) as (t,):
        _, _, info, seg = check(hip_engine, t, keys, words[:, :1], asset_keys, 0, max_doc_freq=6)
        assert info["stop_chunks"] == 7
        # the ordinals still count the stop chunk: the second run starts at chunk 4 of either asset
        assert [tuple(int(v) for v in s) for s in seg.tolist()] == [(0, 1, 0, 0, 3, 0, 0, 10, 6, 16), (0, 1, 4, 4, 4, 0, 4, 14, 11, 21)]
        _, _, info, seg = check(hip_engine, t, keys, words[:, :1], asset_keys, 0, max_doc_freq=7)
        assert info["stop_chunks"] == 0 and tuple(int(v) for v in seg[0]) == (0, 1, 0, 0, 8, 0, 0, 10, 11, 21)
        _, _, info, seg = check(hip_engine, t, keys, words[:, :1], asset_keys, 0, max_doc_freq=0)
        assert info["stop_chunks"] == 0 and int(seg["length"][0]) == 8


def test_removed_rows_close_the_ordinals_up(hip_engine):
    rng = np.random.default_rng(2)
    n = 3000
    keys, words, asset_keys, special = clipped(rng, n)
    with dropping(sp_table(hip_engine, 8, keys, words)) as (t,):
        _, _, _, before = check(hip_engine, t, keys, words[:, :1], asset_keys, 3)
        gone = rng.choice(np.arange(2, n), size=700, replace=False)
        assert t.remove(keys[gone]) == 700
        keep = np.setdiff1d(np.arange(n), gone)
        _, _, info, after = check(hip_engine, t, keys[keep], words[keep, :1], asset_keys, 3)
        assert info["segments"] > 0 and info["live_rows"] <= len(keep)
        # chunks inside clips went: runs were cut, and what lies behind a removed chunk moved down
        assert len(after) != len(before) or after.tobytes() != before.tobytes()
        assert int(before["length"].sum()) > int(after["length"].sum()) and int(after["length"].max()) >= 2
        t.remove(keys[keep[1:]])
        rec, chunks, info, seg = check(hip_engine, t, keys[:1], words[:1, :1], asset_keys, 64, launches=False)       # one row: nothing launched
        assert len(rec) == 0 and len(seg) == 0 and int(chunks.sum()) == 1
        assert info == {"chunk_pairs": 0, "records": 0, "live_rows": 1, "stop_chunks": 0, "segments": 0}
        t.remove(keys[:1])
        rec, chunks, info, seg = check(hip_engine, t, keys[:0], words[:0, :1], asset_keys, 64, launches=False)       # empty
        assert len(rec) == 0 and len(seg) == 0 and int(chunks.sum()) == 0
        assert info == {"chunk_pairs": 0, "records": 0, "live_rows": 0, "stop_chunks": 0, "segments": 0}


def test_ends_pass_32_bits(hip_engine):
    a, b = 0x0123456789ABCDEF, 0xFEDCBA9876543210
    keys = chunk_keys([1, 1, 2, 2], [0xFFFFFE00, 0xFFFFFF00, 0, 0xFFFFFF00], [0x100, 0x1000, 8, 0x1000])
    words = np.array([[a], [b], [a], [b]], dtype=np.uint64)
    with dropping(sp_table(hip_engine, 8, keys, words)) as (t,):
        _, _, info, seg = check(hip_engine, t, keys, words, np.array([1, 2], dtype=np.uint64), 0)
        assert [tuple(int(v) for v in s) for s in seg.tolist()] == [(0, 1, 0, 0, 2, 0, 0xFFFFFE00, 0, 0x100000F00, 0x100000F00)]


def test_capacity_is_exact_on_both_kernels(hip_engine):
    rng = np.random.default_rng(9)
    keys, words, asset_keys, _ = clipped(rng, 1500)
    rc, exp_rec, exp_chunks, exp_info, exp_seg = model_segments(keys, words[:, :1], asset_keys, 3)
    total = exp_info["chunk_pairs"]
    assert total > 100
    assert model_segments(keys, words[:, :1], asset_keys, 3, capacity=total - 1)[0] == ENOSPC
    with dropping(sp_table(hip_engine, 8, keys, words)) as (t,):
        for option in (forced, valu):
            with option(hip_engine):
                rc, _, _, info, _ = raw_call(hip_engine, t, 3, asset_keys, total - 1)
                assert rc == -errno.ENOSPC and int(info[0]) == total
                assert "capacity" in hip_engine._lib.isccsearch_last_error().decode()
                rc, _, _, info, _ = raw_call(hip_engine, t, 3, asset_keys, 0)
                assert rc == -errno.ENOSPC and int(info[0]) == total
                rc, rec, chunks, info, seg = raw_call(hip_engine, t, 3, asset_keys, total)
                assert rc == 0
                same_result((rec[: int(info[1])], chunks, dict(zip(INFO_NAMES, info.tolist())), seg[: int(info[4])]),
                            (exp_rec, exp_chunks, exp_info, exp_seg), "capacity == total")
        with pytest.raises(ValueError, match="exceed max_pairs"):
            t.join_segments(3, asset_keys, 0, total - 1)
        got = t.join_segments(3, asset_keys, 0, total)
        same_result(got, (exp_rec, exp_chunks, exp_info, exp_seg), "max_pairs == total")


def test_refused_arguments_leave_the_outputs_untouched(hip_engine):
    keys = chunk_keys([1, 2, 3])
    words = np.array([[5], [5], [6]], dtype=np.uint64)
    call = hip_engine._lib.isccsearch_join_segments
    last_error = lambda: hip_engine._lib.isccsearch_last_error().decode()
    with dropping(sp_table(hip_engine, 8, keys, words), hip_engine.open_table(_lib.METRIC_HAMMING, 1, 8),
                  hip_engine.open_table(_lib.METRIC_NPHD, 1, 32)) as (t, t_kw1, t_nphd):
        t_kw1.add(np.array([1, 2], dtype=np.uint64), words[:2])
        good = np.array([1, 2, 3], dtype=np.uint64)
        records = np.full(8, 0xEE, dtype=np.uint8).repeat(32).view(_lib.OVERLAP_DTYPE)
        segments = np.full(4, 0xEE, dtype=np.uint8).repeat(48).view(_lib.SEGMENT_DTYPE)
        chunks = np.full(3, 0xEEEEEEEE, dtype=np.uint32)
        info = np.full(5, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
        P = _lib.ptr
        h = hip_engine.handle
        base = dict(h=h, table=t.id, max_hamming=0, max_doc_freq=0, dup_limit=1000, n_assets=3, asset_keys=P(good), capacity=4,
                    out_pairs=P(records), out_segments=P(segments), out_chunks=P(chunks), out_info=P(info))
        unsorted, repeated = np.array([1, 3, 2], dtype=np.uint64), np.array([1, 2, 2], dtype=np.uint64)
        cases = [
            (dict(h=None), -errno.EINVAL, "handle"),
            (dict(asset_keys=None), -errno.EINVAL, "NULL"),
            (dict(out_chunks=None), -errno.EINVAL, "NULL"),
            (dict(out_info=None), -errno.EINVAL, "NULL"),
            (dict(out_pairs=None), -errno.EINVAL, "out_pairs"),
            (dict(out_segments=None), -errno.EINVAL, "out_segments"),
            (dict(table=t_kw1.id), -errno.EINVAL, "key_words"),
            (dict(table=t_nphd.id), -errno.EINVAL, "HAMMING"),
            (dict(n_assets=0), -errno.EINVAL, "n_assets"),
            (dict(n_assets=0xFFFFFFFF), -errno.EINVAL, "n_assets"),
            (dict(asset_keys=P(unsorted)), -errno.EINVAL, "asset_keys[2]"),
            (dict(asset_keys=P(repeated)), -errno.EINVAL, "asset_keys[2]"),
            (dict(max_hamming=-1), -errno.EINVAL, "max_hamming"),
            (dict(max_doc_freq=11, dup_limit=10), -errno.EINVAL, "dup_limit"),
            (dict(capacity=1 << 31), -errno.E2BIG, "32 bits"),
        ]
        before = counters(hip_engine)
        untouched = lambda: (bool(np.all(records.view(np.uint8) == 0xEE)) and bool(np.all(segments.view(np.uint8) == 0xEE))
                             and bool(np.all(chunks == 0xEEEEEEEE)) and bool(np.all(info == 0xEEEEEEEEEEEEEEEE)))
        for change, want, word in cases:
            args = dict(base, **change)
            rc = call(*args.values())
            assert rc == want and word in last_error(), (change, rc, last_error())
            assert untouched(), change
        assert counters(hip_engine) == before
        with pytest.raises(ValueError, match="ascending"):
            t.join_segments(0, unsorted, 0, 10)
        # what is allowed: both outputs NULL with capacity 0 (here -ENOSPC: one chunk pair), max_doc_freq == dup_limit
        assert call(*dict(base, capacity=0, out_pairs=None, out_segments=None).values()) == -errno.ENOSPC and int(info[0]) == 1
        assert call(*dict(base, max_doc_freq=10, dup_limit=10).values()) == 0 and info.tolist() == [1, 2, 3, 0, 1] and chunks.tolist() == [1, 1, 1]
        assert tuple(int(v) for v in segments[0]) == (0, 1, 0, 0, 1, 0, 0, 1, 1, 2)


def test_find_shared_content_end_to_end(hip_engine):
    """About 300 assets and 3 000 chunks of one type: the device result equals the model-backed one of ``test_shared_segments``."""
    rng = np.random.default_rng(31)
    assets = library(rng, 300, chunks=(4, 14))
    # and a clip of ten chunks whose fifth chunk was replaced: max_gap=1 makes one segment of its two runs
    clip = [rnd(rng) for _ in range(10)]
    assets.append(make_asset(rng, 300, simprints={CT: chunks_of(clip)}))
    assets.append(make_asset(rng, 301, simprints={CT: chunks_of([rnd(rng)] + clip[:4] + [rnd(rng)] + clip[5:])}))
    cpu = cpu_index(assets)
    exp = cpu.find_shared_content(max_doc_freq=0, segments=True, max_gap=1)
    idx = HipIndex(hip_engine, HipOptions())
    try:
        idx.add_assets(assets)
        assert 2500 < idx._sp_tables[CT].size < _lib.MAX_K
        _, m0 = counters(hip_engine)
        with forced(hip_engine):
            got = idx.find_shared_content(max_doc_freq=0, segments=True, max_gap=1)
        _, m1 = counters(hip_engine)
        with valu(hip_engine):
            ref = idx.find_shared_content(max_doc_freq=0, segments=True, max_gap=1)
        assert m1 > m0 and counters(hip_engine)[1] == m1
        assert len(got) > 100 and got == exp and ref == exp
        runs = [s for p in got for t in p.types.values() for s in t.segments]
        assert max(s.chunks for s in runs) >= 4 and any(s.span > s.chunks for s in runs)
        kwargs = dict(min_chunks=2, max_doc_freq=5, segments=True, min_segment=2)
        assert idx.find_shared_content(**kwargs) == cpu.find_shared_content(**kwargs)
        # segments=False stays the call it was
        assert idx.find_shared_content(max_doc_freq=0) == cpu.find_shared_content(max_doc_freq=0)
    finally:
        idx.close()
