"""
The device-resident result lists and their merge against host references (``csrc/device_api.hip.h``, ``merge_kernel``).

A. ``merge_kernel`` on synthetic ``Record`` lists (``tests/device_lists.py``) against ``reference_merge``: list counts, the block
   boundary of the element loop, the direct and the indirect result path, both layouts, counts of every shape, the overflow
   marker, exact ties, the ordered entry points, ``merge_many`` and every refusal.
B. ``search_device`` / ``search_within_device`` / the asynchronous search against the oracle, the raw records read back: keys,
   distances, prefix lengths, counts, and ``dist_rank`` ordering as the fraction hamming / prefix_bits does.

Every comparison is exact integer equality.
"""

import ctypes
import errno
import functools
import os

import numpy as np
import pytest
import torch

from device_lists import check_record_order, make_lists, mixed_counts, pack, reference_merge, upload
from iscc_search_amd import _lib
from iscc_search_amd.engine import _alloc_out
from iscc_search_amd.sharded import block_bytes
from oracle import oracle_topk
from oracle_engine import OracleTable
from test_gpu_parity import METRIC_HAMMING, METRIC_NPHD, _mask_to_len, _rand_words

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ("keys", "hamming", "prefix_bits", "count")
GUARD = 4096
TINY_ROWS = 16384                    # the library's default: tables are built once below it and once above (20 000 rows)


def _assert_same(got, exp, what=""):
    for g, e, name in zip(got, exp, NAMES):
        np.testing.assert_array_equal(g, e, err_msg=f"{what} {name}")


def _merge(engine, lists, counts, k, key_words, layout="blocks", **kw):
    n_lists, nq, _ = lists.shape
    dev, rec, cnt, ls, cs = upload(lists, counts, layout)
    return engine.merge_device(n_lists, nq, k, key_words, rec, cnt, ls, cs, **kw)


def _check_merge(engine, rng, n_lists, nq, k, key_words, counts=None, layout="blocks"):
    counts = mixed_counts(rng, n_lists, nq, k) if counts is None else counts
    lists = make_lists(rng, n_lists, nq, k, key_words, counts)
    _assert_same(_merge(engine, lists, counts, k, key_words, layout), reference_merge(lists, counts, k, key_words),
                 f"n_lists={n_lists} nq={nq} k={k} key_words={key_words} {layout}:")
    return lists, counts


# ---------------------------------------------------------------------------------------------------------------------
# A. merge_kernel on synthetic lists
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["blocks", "split"])
@pytest.mark.parametrize("key_words", [1, 2])
@pytest.mark.parametrize("n_lists", [1, 2, 3, 8, 16])
def test_merge_list_counts_and_layouts(hip_engine, n_lists, key_words, layout):
    """1 to 16 lists of 0, 1, k - 1 or k records per query; ``split``: list_stride != count_stride, gaps behind the records."""
    _check_merge(hip_engine, np.random.default_rng(1000 + 10 * n_lists + key_words), n_lists, 9, 10, key_words, layout=layout)


@pytest.mark.parametrize("key_words", [1, 2])
@pytest.mark.parametrize("k", [1, 2, 255, 256, 257])
def test_merge_element_loop_around_the_block_size(hip_engine, k, key_words):
    """The element loop strides by BLOCK = 256 over n_lists * k."""
    _check_merge(hip_engine, np.random.default_rng(2000 + k), 3, 5, k, key_words)


@pytest.mark.parametrize("nq,direct", [(10, True), (12, False)])
def test_merge_direct_and_indirect_result_path(hip_engine, nq, direct):
    """k = 4 096 x 2 lists: 983 080 result bytes are written straight into pinned memory, 1 179 696 go through device memory."""
    k = 4096
    assert (nq * k * 24 + nq * 4 <= (1 << 20)) == direct
    rng = np.random.default_rng(3000 + nq)
    counts = np.full((2, nq), k, dtype=np.uint32)
    counts[:, : nq // 2] = mixed_counts(rng, 2, nq // 2, k)
    _check_merge(hip_engine, rng, 2, nq, k, 2, counts)


@pytest.mark.parametrize("k", [10, 256])
def test_merge_many_blocks(hip_engine, k):
    """300 queries = 300 blocks; at k = 256 the host unpacks 76 800 records, above the 65 536 where it takes its thread pool."""
    _check_merge(hip_engine, np.random.default_rng(4000 + k), 4, 300, k, 1 if k == 10 else 2)


def test_merge_count_shapes(hip_engine):
    rng = np.random.default_rng(5000)
    n_lists, nq, k = 4, 9, 10
    # every count 0
    zeros = np.zeros((n_lists, nq), dtype=np.uint32)
    lists = make_lists(rng, n_lists, nq, k, 2, zeros)
    got = _merge(hip_engine, lists, zeros, k, 2)
    assert not got[3].any() and not got[0].any() and not got[1].any() and not got[2].any()
    # the total over the lists stays below k for some queries
    few = rng.integers(0, 4, size=(n_lists, nq)).astype(np.uint32)
    few[:, 0], few[:, 1] = [1, 0, 2, 0], [3, 3, 3, 3]
    assert (few.sum(axis=0) < k).any() and (few.sum(axis=0) >= k).any()
    _check_merge(hip_engine, rng, n_lists, nq, k, 1, few)
    # raw counts above k are clamped to k
    for raw in (k + 5, 0xFFFFFFFE):
        above = mixed_counts(rng, n_lists, nq, k)
        above[2, :] = raw
        above[0, 3] = raw
        _check_merge(hip_engine, rng, n_lists, nq, k, 2, above)
    # one list full, all the others empty
    for full in (0, n_lists - 1):
        one = np.zeros((n_lists, nq), dtype=np.uint32)
        one[full] = k
        lists, _ = _check_merge(hip_engine, rng, n_lists, nq, k, 1, one)
        np.testing.assert_array_equal(_merge(hip_engine, lists, one, k, 1)[0], lists[full]["key_lo"])


@pytest.mark.parametrize("n_lists", [1, 3])
def test_merge_passes_the_overflow_marker_on(hip_engine, n_lists):
    rng = np.random.default_rng(6000 + n_lists)
    nq, k = 9, 10
    counts = mixed_counts(rng, n_lists, nq, k)
    counts[0, 2] = counts[n_lists - 1, 7] = _lib.COUNT_OVERFLOW
    lists = make_lists(rng, n_lists, nq, k, 2, counts)
    got = _merge(hip_engine, lists, counts, k, 2)
    assert [q for q in range(nq) if got[3][q] == _lib.COUNT_OVERFLOW] == [2, 7]
    assert not got[0][[2, 7]].any() and not got[1][[2, 7]].any() and not got[2][[2, 7]].any()
    _assert_same(got, reference_merge(lists, counts, k, 2))


def test_merge_exact_ties_go_to_the_lower_list(hip_engine):
    """The same (dist_rank, key) in two lists: both records come out, the lower list's first, no slot stale or written twice."""
    rng = np.random.default_rng(7000)
    n_lists, nq, k = 3, 6, 10
    counts = np.full((n_lists, nq), k, dtype=np.uint32)
    lists = make_lists(rng, n_lists, nq, k, 2, counts)
    pairs = [(0, 2), (0, 1), (1, 2), (0, 2), (1, 2), (0, 1)]          # per query: the two lists that share a record
    for q, (a, b) in enumerate(pairs):
        lists["dist_rank"][a, q, 0] = 0                     # below the alphabet: list a's head is the query's first record ...
        twin = lists[a, q, 0].copy()
        twin["hamming"], twin["prefix_bits"] = 4000 + q, 5000 + q
        lists[b, q, 0] = twin                               # ... and list b's head equals it in (rank, key), with a payload of its own
    got = _merge(hip_engine, lists, counts, k, 2)
    _assert_same(got, reference_merge(lists, counts, k, 2))
    for q, (a, b) in enumerate(pairs):
        assert got[1][q, :2].tolist() == [int(lists[a, q, 0]["hamming"]), 4000 + q]
        assert (got[0][q, 0] == got[0][q, 1]).all() and int(got[2][q, 1]) == 5000 + q
        given = {(int(r["key_hi"]), int(r["key_lo"]), int(r["hamming"]), int(r["prefix_bits"])) for r in lists[:, q].reshape(-1)}
        out = [(int(got[0][q, i, 0]), int(got[0][q, i, 1]), int(got[1][q, i]), int(got[2][q, i])) for i in range(int(got[3][q]))]
        assert len(out) == k and len(set(out)) == k and set(out) <= given


def test_merge_ordered_behind_the_producer_stream(hip_engine):
    """The lists arrive by a non-blocking copy on another stream: ``after_stream`` orders the merge behind it on the device."""
    rng = np.random.default_rng(8000)
    n_lists, nq, k = 3, 64, 200
    counts = mixed_counts(rng, n_lists, nq, k)
    lists = make_lists(rng, n_lists, nq, k, 2, counts)
    exp = reference_merge(lists, counts, k, 2)
    buf, rec_off, cnt_off, ls, cs = pack(lists, counts, "blocks")
    pinned = torch.from_numpy(buf).pin_memory()
    side = torch.cuda.Stream(device=DEV)
    own = torch.cuda.ExternalStream(hip_engine.stream(), device=DEV)
    for stream in (side, own):
        dev = torch.zeros(buf.size, dtype=torch.uint8, device=DEV)          # all counts 0 until the copy lands
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            dev.copy_(pinned, non_blocking=True)
        got = hip_engine.merge_device(n_lists, nq, k, 2, dev.data_ptr() + rec_off, dev.data_ptr() + cnt_off, ls, cs,
                                      after_stream=stream.cuda_stream)
        _assert_same(got, exp, "side stream:" if stream is side else "the library's stream:")
        torch.cuda.synchronize()


def test_merge_many_requests_of_different_shapes(hip_engine):
    """Four merges behind one synchronisation; k = 1 and odd nq make the per-request offsets need their 16-byte rounding."""
    rng = np.random.default_rng(9000)
    shapes = [(2, 9, 1, 1), (3, 7, 10, 2), (5, 1, 33, 1), (1, 5, 100, 2)]       # (n_lists, nq, k, key_words)
    assert any((nq * k * 24 + nq * 4) % 16 for _, nq, k, _ in shapes)
    keep, merges, exps = [], [], []
    for n_lists, nq, k, key_words in shapes:
        counts = mixed_counts(rng, n_lists, nq, k)
        lists = make_lists(rng, n_lists, nq, k, key_words, counts)
        dev, rec, cnt, ls, cs = upload(lists, counts, "split" if n_lists == 3 else "blocks")
        keep.append(dev)
        merges.append((n_lists, nq, k, key_words, rec, cnt, ls, cs))
        exps.append(reference_merge(lists, counts, k, key_words))
    for after in (torch.cuda.current_stream().cuda_stream, hip_engine.stream()):
        outs = hip_engine.merge_many(merges, after)
        assert len(outs) == len(shapes)
        for i, (got, exp) in enumerate(zip(outs, exps)):
            _assert_same(got, exp, f"request {i}:")


def test_merge_many_refuses_more_than_the_direct_block(hip_engine):
    """Results above 1 MiB in all: -E2BIG -> RuntimeError before any launch; the engine merges on as before."""
    rng = np.random.default_rng(9100)
    n_lists, nq, k = 1, 6, 4096
    counts = np.full((n_lists, nq), k, dtype=np.uint32)
    lists = make_lists(rng, n_lists, nq, k, 1, counts)
    dev, rec, cnt, ls, cs = upload(lists, counts)
    req = (n_lists, nq, k, 1, rec, cnt, ls, cs)
    assert 2 * (nq * k * 24 + nq * 4) > (1 << 20) >= nq * k * 24 + nq * 4
    with pytest.raises(RuntimeError, match="exceed"):
        hip_engine.merge_many([req, req], hip_engine.stream())
    exp = reference_merge(lists, counts, k, 1)
    _assert_same(hip_engine.merge_many([req], hip_engine.stream())[0], exp)
    _assert_same(hip_engine.merge_device(*req), exp)


BAD_MERGES = {                        # what to change in a valid request (n_lists, nq, k, key_words, rec, cnt, list_stride, count_stride)
    "n_lists=0": lambda r: (0,) + r[1:],
    "k=0": lambda r: r[:2] + (0,) + r[3:],
    "k=4097": lambda r: r[:2] + (4097,) + r[3:],
    "key_words=3": lambda r: r[:3] + (3,) + r[4:],
    "list_stride=12": lambda r: r[:6] + (12, r[7]),
    "count_stride=6": lambda r: r[:7] + (6,),
    "records+4": lambda r: r[:4] + (r[4] + 4,) + r[5:],
    "counts+2": lambda r: r[:5] + (r[5] + 2,) + r[6:],
}


@pytest.mark.parametrize("what", list(BAD_MERGES))
def test_merge_refusals(hip_engine, what):
    """Refused on the host, before any launch: ValueError through ``merge_device`` and inside a ``merge_many`` request."""
    rng = np.random.default_rng(9200)
    n_lists, nq, k = 2, 5, 8
    counts = mixed_counts(rng, n_lists, nq, k)
    lists = make_lists(rng, n_lists, nq, k, 2, counts)
    dev, rec, cnt, ls, cs = upload(lists, counts)
    good = (n_lists, nq, k, 2, rec, cnt, ls, cs)
    bad = BAD_MERGES[what](good)
    # the C entry points themselves (the wrapper's own array shapes refuse some of these before the call)
    out, addr = _alloc_out(nq, 4097, 2)
    lib = hip_engine._lib
    a = (hip_engine.handle, *bad[:4], ctypes.c_void_p(bad[4]), ctypes.c_void_p(bad[5]), bad[6], bad[7])
    assert lib.isccsearch_merge_device(*a, *addr) == -errno.EINVAL
    assert lib.isccsearch_merge_device_after(*a, ctypes.c_void_p(hip_engine.stream()), *addr) == -errno.EINVAL
    with pytest.raises(ValueError):
        hip_engine.merge_device(*bad)
    with pytest.raises(ValueError):
        hip_engine.merge_device(*bad, after_stream=hip_engine.stream())
    with pytest.raises(ValueError):
        hip_engine.merge_many([good, bad], hip_engine.stream())
    _assert_same(hip_engine.merge_device(*good), reference_merge(lists, counts, k, 2))


# ---------------------------------------------------------------------------------------------------------------------
# B. device-resident searches against the oracle
# ---------------------------------------------------------------------------------------------------------------------
class _Block:
    """A {records | counts} block in device memory between two guard bands of 0xA5."""

    def __init__(self, nq, k):
        self.nq, self.k = nq, k
        self.rec_bytes, self.blk = block_bytes(nq, k)
        self.dev = torch.full((GUARD + self.blk + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        self.rec = self.dev.data_ptr() + GUARD
        self.cnt = self.rec + self.rec_bytes

    def read(self):
        """(records [nq][k], counts [nq]); nothing outside them may have been written."""
        host = self.dev.cpu().numpy()
        used = self.rec_bytes + self.nq * 4
        assert (host[:GUARD] == 0xA5).all(), "bytes in front of the block were written"
        assert (host[GUARD + used :] == 0xA5).all(), "bytes behind the counts were written"
        rec = host[GUARD : GUARD + self.rec_bytes].view(_lib.RECORD_DTYPE).reshape(self.nq, self.k)
        return rec, host[GUARD + self.rec_bytes : GUARD + used].view(np.uint32)


def _assert_records(rec, cnt, exp, key_words, what="", prefix_only=False):
    """Raw records against (keys, hamming, prefix_bits, count) of the oracle; ``prefix_only``: each list is the oracle's first ``count`` rows."""
    if not prefix_only:
        np.testing.assert_array_equal(cnt, exp[3], err_msg=f"{what} counts")
    for q in range(len(cnt)):
        c = int(cnt[q])
        assert c <= int(exp[3][q]), f"{what} query {q}: count {c} above the oracle's {int(exp[3][q])}"
        r = rec[q, :c]
        if key_words == 2:
            np.testing.assert_array_equal(np.stack([r["key_hi"], r["key_lo"]], axis=1), exp[0][q, :c], err_msg=f"{what} keys, query {q}")
        else:
            np.testing.assert_array_equal(r["key_lo"], exp[0][q, :c], err_msg=f"{what} keys, query {q}")
        np.testing.assert_array_equal(r["hamming"], exp[1][q, :c], err_msg=f"{what} hamming, query {q}")
        np.testing.assert_array_equal(r["prefix_bits"], exp[2][q, :c], err_msg=f"{what} prefix bits, query {q}")
        check_record_order(rec[q], c, key_words)


def _search(table, q, qn, k, r=None, **kw):
    blk = _Block(q.shape[0], k)
    table.search_device(q, qn, k, blk.rec, blk.cnt, max_hamming=r, **kw)
    torch.cuda.synchronize()
    return blk.read()


def _keys(rng, n, key_words):
    if key_words == 2:
        return np.stack([rng.integers(1, 40, size=n).astype(np.uint64), rng.permutation(n).astype(np.uint64) + np.uint64(1)], axis=1)
    return rng.permutation(np.arange(n, dtype=np.uint64) * np.uint64(977) + np.uint64(3))


@functools.lru_cache(maxsize=None)
def _hamming_data(n, nbytes, key_words):
    """Random rows, every 7th one of six codes (a third of those a bit or two away); queries: the six codes, near-duplicates of
    single rows and random ones -- ties at every cut.  Returns (keys, words, queries, the oracle table)."""
    rng = np.random.default_rng(n + 10 * nbytes + key_words)
    mw = (nbytes + 7) // 8
    words = _rand_words(rng, n, mw, nbytes)
    pool = _rand_words(rng, 6, mw, nbytes)
    for i in range(0, n, 7):
        words[i] = pool[int(rng.integers(0, 6))]
        if i % 3 == 0:
            words[i, 0] ^= np.uint64(1) << np.uint64(int(rng.integers(56, 64)))
    keys = _keys(rng, n, key_words)
    near = words[[1, 2]].copy()                              # rows 1, 2 are random: a neighbour at 1 bit, the next far away
    near[:, 0] ^= np.uint64(1) << np.uint64(60)
    q = np.concatenate([pool, near, _rand_words(rng, 1, mw, nbytes)])
    ot = OracleTable(METRIC_HAMMING, key_words, nbytes)
    ot.add(keys, words, trusted_unique=True)
    for a in (keys, words, q):
        a.setflags(write=False)
    return keys, words, q, ot


@pytest.mark.parametrize("n", [3000, 20000])
@pytest.mark.parametrize("nbytes,key_words", [(8, 1), (16, 2)])
def test_search_device_hamming_vs_oracle(hip_engine, nbytes, key_words, n):
    keys, words, q, ot = _hamming_data(n, nbytes, key_words)
    assert (n <= TINY_ROWS) == (n == 3000) and q.shape[0] == 9
    t = hip_engine.open_table(METRIC_HAMMING, key_words, nbytes)
    try:
        t.add(keys, words)
        for k in (1, 10, 300):
            exp = oracle_topk(METRIC_HAMMING, keys, words, None, q, None, k, fixed_nbytes=nbytes)
            _assert_records(*_search(t, q, None, k), exp, key_words, f"top-{k}:")
            exp = ot.search_within(q, None, k, 2)
            assert exp[3].min() < exp[3].max()               # some lists are short of k
            _assert_records(*_search(t, q, None, k, r=2), exp, key_words, f"within 2, k={k}:")
    finally:
        t.drop()


@pytest.mark.parametrize("n", [3000, 20000])
def test_search_device_chunk_loop_beyond_1024_queries(hip_engine, n):
    """nq = 1 024 + 6: the second chunk writes at ``out + pos * k`` / ``d_counts + pos`` -- queries 1024.. as exact as query 0,
    nothing outside [nq][k] touched."""
    keys, words, _, ot = _hamming_data(n, 8, 1)
    rng = np.random.default_rng(77)
    nq, k = 1030, 7
    q = words[rng.integers(0, n, size=nq)].copy()
    for b in range(3):                                       # 0 to 3 bits away from a stored row
        q[:, 0] ^= (rng.integers(0, 2, size=nq).astype(np.uint64)) << np.uint64(3 + 17 * b)
    t = hip_engine.open_table(METRIC_HAMMING, 1, 8)
    try:
        t.add(keys, words)
        exp = oracle_topk(METRIC_HAMMING, keys, words, None, q, None, k, fixed_nbytes=8)
        rec, cnt = _search(t, q, None, k)
        _assert_records(rec, cnt, exp, 1, "top-k:")
        exp = ot.search_within(q, None, k, 3)
        assert exp[3][1024:].min() >= 1 and len(set(exp[3].tolist())) > 1
        rec, cnt = _search(t, q, None, k, r=3)
        _assert_records(rec, cnt, exp, 1, "within 3:")
    finally:
        t.drop()


NPHD_LENGTHS = (4, 8, 12, 16, 32)


@functools.lru_cache(maxsize=None)
def _nphd_data(big):
    """Rows of 4, 8, 12, 16 and 32 bytes -- one segment each; families that share a prefix at every length.  ``big``: the 8-byte
    segment holds 20 000 rows (beyond the one-launch path), every other a few hundred."""
    rng = np.random.default_rng(40 + big)
    sizes = {4: 300, 8: 20000 if big else 900, 12: 500, 16: 700, 32: 600}
    lens = rng.permutation(np.concatenate([np.full(c, b, dtype=np.uint8) for b, c in sizes.items()]))
    n = len(lens)
    words = _rand_words(rng, n, 4, lens)
    base = _rand_words(rng, 3, 4, 32)
    for i in range(0, n, 5):
        words[i] = _mask_to_len(base[i % 3 : i % 3 + 1], lens[i : i + 1])[0]
        if i % 4 == 0:
            words[i, 0] ^= np.uint64(1) << np.uint64(int(rng.integers(32, 64)))     # inside every prefix
    keys = _keys(rng, n, 1)
    q = np.concatenate([base, base[:2], _rand_words(rng, 1, 4, 32)])
    q[3, 0] ^= np.uint64(1) << np.uint64(40)
    q[4, 0] ^= np.uint64(3) << np.uint64(50)
    ot = OracleTable(METRIC_NPHD, 1, 32)
    ot.add(keys, words, lens, trusted_unique=True)
    for a in (keys, words, lens, q):
        a.setflags(write=False)
    return keys, words, lens, q, ot


def _nphd_queries(q, qlen):
    return _mask_to_len(q, qlen), np.full(q.shape[0], qlen, dtype=np.uint8)


def _nphd_cases(keys, words, lens, q32, ot):
    """(label, queries, lengths, k, radius, expected) for every query length: top-k and three radii."""
    for qlen in (4, 8, 12, 32):
        q, qn = _nphd_queries(q32, qlen)
        yield f"len {qlen} top-20:", q, qn, 20, None, oracle_topk(METRIC_NPHD, keys, words, lens, q, qn, 20)
        for r in (0, 5, 8 * qlen):
            yield f"len {qlen} within {r}:", q, qn, 40, r, ot.search_within(q, qn, 40, r)


@pytest.mark.parametrize("big", [0, 1])
@pytest.mark.parametrize("asynchronous", [False, True])
def test_search_device_nphd_several_segments(hip_engine, big, asynchronous):
    """Five segments: the synchronous multi-segment path (per-segment lists fixed and merged).  ``asynchronous``: the same calls
    through ``consumer_stream`` fall back to it -- complete when they return, no overflow marker."""
    keys, words, lens, q32, ot = _nphd_data(big)
    t = hip_engine.open_table(METRIC_NPHD, 1, 32)
    try:
        t.add(keys, words, lens)
        assert len(t.segments()) == len(NPHD_LENGTHS) and (max(t.segments().values()) > TINY_ROWS) == bool(big)
        kw = {"consumer_stream": torch.cuda.current_stream().cuda_stream} if asynchronous else {}
        for label, q, qn, k, r, exp in _nphd_cases(keys, words, lens, q32, ot):
            rec, cnt = _search(t, q, qn, k, r=r, **kw)
            assert not (cnt == _lib.COUNT_OVERFLOW).any()
            _assert_records(rec, cnt, exp, 1, label)
        mixed = np.array([8, 8, 32, 8, 8, 8], dtype=np.uint8)
        blk = _Block(6, 5)
        for kw2 in ({}, kw):
            with pytest.raises(ValueError, match="one byte length"):
                t.search_device(_mask_to_len(q32, mixed), mixed, 5, blk.rec, blk.cnt, **kw2)
    finally:
        t.drop()


@pytest.mark.parametrize("self_hint_path", [False, True])
@pytest.mark.parametrize("n", [3000, 20000])
def test_search_device_async_with_a_hint(hip_engine, n, self_hint_path):
    """
    One segment, ``consumer_stream`` given: no hint and a hint of every bit give the oracle's top-k; under a tight hint each
    list is the oracle's list cut short -- its first ``count`` rows, all k of them when the k-th lies strictly within the hint,
    and never fewer than the rows strictly within it.  (Whether a row AT the hint is listed is not pinned.)
    ``self_hint_path``: ``spec_max_queries = 0`` hands the hint to the single self-tightening pass instead of a range-limited
    one; that pass runs on the matrix cores, which tables of this size reach with ``mfma_min_rows`` lowered.
    """
    keys, words, q, _ = _hamming_data(n, 8, 1)
    k, tight = 10, 8
    exp = oracle_topk(METRIC_HAMMING, keys, words, None, q, None, k, fixed_nbytes=8)
    kth = exp[1][:, k - 1].astype(np.int64)
    assert (kth < tight).any() and (kth > tight).any()
    side = torch.cuda.Stream(device=DEV)
    t = hip_engine.open_table(METRIC_HAMMING, 1, 8)

    def run(hint):
        blk = _Block(q.shape[0], k)
        t.search_device(q, None, k, blk.rec, blk.cnt, consumer_stream=side.cuda_stream, hint=hint)
        side.synchronize()
        return blk.read()

    # a hint of every bit lists the whole table per query: room for it, so that no list is handed back as overflowed
    opts = dict(candidate_cap=32768)
    if self_hint_path:
        opts.update(spec_max_queries=0, mfma_min_rows=4096)
    try:
        t.add(keys, words)
        with hip_engine.options(**opts):
            before = hip_engine.stats()["mfma_launches"]
            _assert_records(*run(None), exp, 1, "no hint:")
            _assert_records(*run(64), exp, 1, "hint 64:")
            rec, cnt = run(tight)
            assert not (cnt == _lib.COUNT_OVERFLOW).any()
            _assert_records(rec, cnt, exp, 1, f"hint {tight}:", prefix_only=True)
            for i in range(q.shape[0]):
                assert int(cnt[i]) >= int((exp[1][i, :k] < tight).sum()), f"query {i}: rows strictly within the hint are missing"
                if kth[i] < tight:
                    assert int(cnt[i]) == k, f"query {i}: k-th distance {kth[i]} < hint {tight}, count {int(cnt[i])}"
            if not self_hint_path:
                assert (cnt < k).any()
            if self_hint_path and n > TINY_ROWS and not os.environ.get("ISCC_HIP_OPTS"):
                assert hip_engine.stats()["mfma_launches"] > before
    finally:
        t.drop()


def test_search_device_refusals(hip_engine):
    keys, words, q, _ = _hamming_data(3000, 8, 1)
    t = hip_engine.open_table(METRIC_HAMMING, 1, 8)
    try:
        t.add(keys, words)
        blk = _Block(q.shape[0], 10)
        stream = torch.cuda.current_stream().cuda_stream
        for kw in ({}, {"consumer_stream": stream}):
            with pytest.raises(ValueError):
                t.search_device(q, None, 0, blk.rec, blk.cnt, **kw)
            with pytest.raises(ValueError):
                t.search_device(q, None, 10, blk.rec, blk.cnt, max_hamming=257, **kw)
            with pytest.raises(ValueError):
                t.search_device(q, np.full(q.shape[0], 4, dtype=np.uint8), 10, blk.rec, blk.cnt, **kw)
        # the C entry points themselves: a Hamming query of the wrong length (the wrapper refuses it before the call)
        lib, short = hip_engine._lib, np.full(q.shape[0], 4, dtype=np.uint8)
        a = (hip_engine.handle, t.id, q.shape[0], _lib.ptr(np.ascontiguousarray(q)), _lib.ptr(short), 10)
        out = (ctypes.c_void_p(blk.rec), ctypes.c_void_p(blk.cnt))
        assert lib.isccsearch_search_device(*a, *out) == -errno.EINVAL
        assert lib.isccsearch_search_within_device(*a, 3, *out) == -errno.EINVAL
        assert lib.isccsearch_search_device_async(*a, -1, *out, ctypes.c_void_p(stream)) == -errno.EINVAL
        torch.cuda.synchronize()
        rec, cnt = blk.read()
        assert (rec.view(np.uint8) == 0xA5).all() and (cnt.view(np.uint8) == 0xA5).all()       # nothing was launched
    finally:
        t.drop()


def test_three_shards_searched_and_merged_on_the_device_equal_the_oracle(hip_engine):
    """The multi-length rows over three tables of unequal size, one without 32-byte rows: per query length ``search_device`` on
    every shard into one gathered tensor, ``merge_device(3, ...)`` == the oracle over all rows.  Records of different
    prefix lengths meet in this merge."""
    keys, words, lens, q32, ot = _nphd_data(0)
    n = len(lens)
    short = np.nonzero(lens != 32)[0]
    third = short[:400]                                      # no 32-byte row
    rest = np.setdiff1d(np.arange(n), third)
    parts = [rest[: len(rest) // 4], rest[len(rest) // 4 :], third]
    assert sorted(len(p) for p in parts) != [len(p) for p in parts] and sum(len(p) for p in parts) == n
    shards = [hip_engine.open_table(METRIC_NPHD, 1, 32) for _ in parts]
    try:
        for t, p in zip(shards, parts):
            t.add(keys[p], words[p], lens[p])
        assert 32 not in shards[2].segments() and 32 in shards[0].segments() and 32 in shards[1].segments()
        for label, q, qn, k, r, exp in _nphd_cases(keys, words, lens, q32, ot):
            nq = q.shape[0]
            rec_bytes, blk = block_bytes(nq, k)
            gathered = torch.full((3 * blk,), 0xA5, dtype=torch.uint8, device=DEV)
            for i, t in enumerate(shards):
                t.search_device(q, qn, k, gathered.data_ptr() + i * blk, gathered.data_ptr() + i * blk + rec_bytes, max_hamming=r)
            torch.cuda.synchronize()
            got = hip_engine.merge_device(3, nq, k, 1, gathered.data_ptr(), gathered.data_ptr() + rec_bytes, blk, blk)
            np.testing.assert_array_equal(got[3], exp[3], err_msg=f"{label} counts")
            for qi in range(nq):
                c = int(exp[3][qi])
                for g, e, name in zip(got[:3], exp[:3], NAMES):
                    np.testing.assert_array_equal(g[qi, :c], e[qi, :c], err_msg=f"{label} {name}, query {qi}")
                    assert not g[qi, c:].any()
            if r is None and int(qn[0]) == 32:
                assert len(np.unique(got[2][0])) > 1, "no two prefix lengths met in the merge"
    finally:
        for t in shards:
            t.drop()
