"""
``isccsearch_join_degrees`` and ``isccsearch_join_within_live`` (``HipTable.join_degrees``, ``HipTable.join_within`` with ``live_keys``),
``find_hubs`` and ``max_degree`` on an MI355X.

Every case runs on BOTH kernels -- the matrix-core form under ``mfma=1, join_mfma=1, join_mfma_min_rows=0`` and the XOR + popcount form
under ``join_mfma=0`` --, reads the statistics to see which kernel ran, and holds the degrees, the links and the live pairs of either to
the host model (``degree_model``: one dense matrix of all-pairs distances) and to each other, for exact equality.  Random codes of 64
bits or more at radius 8 have no pair at these sizes, so every pair is planted.  No table has more than 2 100 rows; the sizes are those
at which the two emit paths change behaviour: 16 / 8 rows per block, 64 lanes, 2 048-row slabs on the VALU kernel; 64-row steps and the
held chunk of the DEGREE form on the matrix cores.
"""

import ctypes
import errno

import numpy as np
import pytest

import degree_model as model
from iscc_search_amd import _lib
from iscc_search_amd.index import HipIndex, HipOptions
from test_gpu_duplicates import mask_lengths, table_with
from test_gpu_join_mfma import NAMES, counters, dropping, forced, valu
from test_hubs import build as oracle_index, hub_assets

pytestmark = pytest.mark.gpu

RADIUS = 8
SLAB = 2048
GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def degree_chunk_rows(W, n):
    """Held rows per chunk of a DEGREE launch over a held segment of n rows of W words: csrc/mfma_scan.hip, mfma_join_groups_per_chunk --
    mfma_groups_per_chunk (an even number of 32-row groups; as many chunks as max_groups[W] asks for, each as small as that number of
    chunks allows), less pairs of groups until the image with its 4 bytes per held row fits 48 KB: 30 groups for 32 at W = 1 (rings:
    4 waves x 8 entries x 36 dwords)."""
    max_groups = {1: 32, 2: 16, 3: 10, 4: 8}[W]
    need = max((n + 31) // 32, 2)
    need += need & 1
    if need > max_groups:
        chunks = -(-need // max_groups)
        need = min(-(-need // chunks) + (-(-need // chunks) & 1), max_groups)
    while need > 2 and need * (W * 1024 + 256 + 128) + 4 * 8 * 36 * 4 > 48 * 1024:
        need -= 2
    return need * 32


# the smallest table of W words that takes a second held chunk: 32 groups (1 024 rows) of 64-bit codes are one chunk of every other
# form and two of this one
JUST_ABOVE_A_CHUNK = {1: 961, 2: 513, 3: 321, 4: 257}


def test_the_chunk_sizes_this_file_relies_on():
    assert degree_chunk_rows(1, 960) == 960 and degree_chunk_rows(1, 1024) == 960
    for W, n in JUST_ABOVE_A_CHUNK.items():
        assert degree_chunk_rows(W, n - 1) >= n - 1 and degree_chunk_rows(W, n) < n, (W, n)


def thresholds(lengths, tau=RADIUS):
    mh = np.full(33, -1, dtype=np.int16)
    for p in lengths:
        mh[p] = tau
    return mh


def flip_at(code, bits):
    out = code.copy()
    for b in bits:
        out[b // 64] ^= np.uint64(1 << (b % 64))
    return out


def flip(rng, code, bits, W):
    """``code`` with ``bits`` distinct bits of its first W words flipped"""
    return flip_at(code, rng.choice(64 * W, size=bits, replace=False).tolist())


def planted_table(rng, n, nbytes, hub=300):
    """
    (keys, words, nb, hub_keys): n random codes of nbytes bytes in row order, and planted among them, as far as n has room: pairs at one
    bit -- rows 0 and 1, and pairs that straddle a row-block, a wave step, the chunk of the DEGREE form and a slab (rows b - 1 and b);
    a hub of ``hub`` equal codes; a clique of 5 within 4 bits of each other; a chain a - b - c at 8 bits each with d(a, c) = 16.  Keys
    are unrelated to the row order.
    """
    W = (nbytes + 7) // 8
    words = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    words[:, W:] = 0
    keys = rng.permutation(np.arange(1, n + 1, dtype=np.uint64) * GOLDEN)
    fixed = set()
    for b in (1, 8, 16, 64, degree_chunk_rows(W, n), SLAB):
        if b < n and not {b - 1, b} & fixed:
            words[b] = flip(rng, words[b - 1], 1, W)
            fixed |= {b - 1, b}
    free = [int(r) for r in rng.permutation(n) if int(r) not in fixed]
    hub_rows = []
    if len(free) >= hub + 40:
        hub_rows, free = free[:hub], free[hub:]
        words[hub_rows] = words[hub_rows[0]]
    if len(free) >= 5:
        clique, free = free[:5], free[5:]
        for r in clique[1:]:
            words[r] = flip(rng, words[clique[0]], 2, W)
    if len(free) >= 3:
        a, b, c = free[:3]
        bits = rng.choice(64 * W, size=16, replace=False).tolist()
        words[b] = flip_at(words[a], bits[:8])
        words[c] = flip_at(words[b], bits[8:])
    nb = np.full(n, nbytes, dtype=np.uint8)
    return keys, mask_lengths(words, nb), nb, np.sort(keys[hub_rows])


def live_lists(rng, keys, hub_keys):
    """every key | none | every second key | keys the table does not hold mixed in | the hub's keys left out"""
    srt = np.sort(np.asarray(keys, dtype=np.uint64))
    absent = np.setdiff1d(rng.integers(1, 2**63, size=20, dtype=np.uint64), srt)
    return [srt, srt[:0], srt[::2], np.union1d(srt[1::3], absent), np.setdiff1d(srt, hub_keys)]


def both_kernels(engine, call, launches):
    """``call()`` on the matrix cores and on the VALU kernel: equal results, the counters saying which kernel ran (or that none did)."""
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
        assert (l2, m2) == (l0, m0), "nothing to join: nothing launched"
    return got, ref


def check(engine, table, rows, mh, live, matrix=None):
    """Degrees, links and live pairs of both kernels against the model of the table ``rows`` = (keys, words, nb); returns (degrees, links)."""
    keys, words, nb = rows
    live = np.asarray(live, dtype=np.uint64)
    matrix = matrix if matrix is not None else model.near_matrix(words, nb, mh)
    launches = len(nb) >= 2 and len(live) >= 2
    (deg, links), (deg_valu, links_valu) = both_kernels(engine, lambda: table.join_degrees(mh, live), launches)
    exp_deg, exp_links = model.join_degrees(keys, words, nb, mh, live, matrix)
    assert deg.dtype == np.uint32 and deg.shape == live.shape
    print(f"rows {len(nb)} listed {len(live)}: links {links} (VALU {links_valu}, model {exp_links}), largest degree {int(deg.max(initial=0))}")
    assert links == links_valu and np.array_equal(deg, deg_valu), "matrix cores against VALU"
    assert links == exp_links and np.array_equal(deg, exp_deg), "against the model"
    assert int(deg.sum(dtype=np.uint64)) == 2 * links
    pairs, pairs_valu = both_kernels(engine, lambda: table.join_within(mh, 10_000_000, live), launches)
    exp_pairs = model.join_within_live(keys, words, nb, mh, live, matrix)
    for g, v, e, name in zip(pairs, pairs_valu, exp_pairs, NAMES):
        assert g.dtype == v.dtype == e.dtype and np.array_equal(g, v), name + " (matrix cores against VALU)"
        assert g.shape == e.shape and np.array_equal(g, e), name + " (against the model)"
    assert len(pairs[2]) == links
    if len(live) == len(nb) and np.array_equal(live, np.sort(keys)):            # every key listed: the plain self-join, byte for byte
        plain = table.join_within(mh, 10_000_000)
        assert links == len(plain[2])
        for g, e, name in zip(pairs, plain, NAMES):
            assert g.dtype == e.dtype and g.tobytes() == e.tobytes(), name + " (against join_within)"
    return deg, links


def check_lists(engine, table, rows, mh, hub_keys, seed):
    matrix = model.near_matrix(rows[1], rows[2], mh)
    return [check(engine, table, rows, mh, live, matrix) for live in live_lists(np.random.default_rng(seed), rows[0], hub_keys)]


# ---- (a) Hamming tables of every compared width at the sizes where a path changes
SIZES = [0, 1, 2, 15, 16, 17, 63, 64, 65, 2047, 2048, 2049]


@pytest.mark.parametrize("nbytes", [8, 16, 24, 32])
@pytest.mark.parametrize("n", SIZES + ["chunk + 1"])
def test_hamming_tables(hip_engine, n, nbytes):
    W = nbytes // 8
    n = JUST_ABOVE_A_CHUNK[W] if n == "chunk + 1" else n
    rng = np.random.default_rng(1000 * nbytes + n)
    keys, words, nb, hub_keys = planted_table(rng, n, nbytes)
    rows = (keys, words, nb)
    with dropping(table_with(hip_engine, _lib.METRIC_HAMMING, 1, nbytes, *rows)) as (t,):
        results = check_lists(hip_engine, t, rows, thresholds([nbytes]), hub_keys, n)
        deg, links = results[0]
        if n >= 2:
            assert links > 0                                # (every size from 2 rows on holds a planted pair)
        if n >= 400:
            hub = len(hub_keys)
            assert hub == 300 and links >= hub * (hub - 1) // 2 and int(deg.max()) == hub - 1
            assert results[4][1] == links - hub * (hub - 1) // 2         # the hub's keys left out: its pairs are gone, nothing else
        assert results[1][1] == 0 and results[2][1] <= links


# ---- (b) NPHD: segments of 8, 16 and 32 bytes -- cross-segment launches -- and a partial last word
def nphd_table(rng, n, lengths, hub):
    """Random rows of mixed lengths; a hub of rows that are ONE 32-byte code cut to the row's length (distance 0 over every common prefix);
    rows that differ from a hub row only behind a shorter partner's length"""
    words = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    nb = rng.choice(lengths, size=n).astype(np.uint8)
    rows = rng.permutation(n)
    hub_rows, tail_rows = rows[:hub], rows[hub:hub + 30]
    words[hub_rows] = words[hub_rows[0]]
    words[tail_rows] = words[hub_rows[0]]
    words[tail_rows, 3] ^= np.uint64(0xFFFFFFFFFFFFFFFF)            # bytes 24 .. 31: far from the 32-byte hub rows, equal to the shorter ones
    words[tail_rows, 1] ^= np.uint64(0x00000000FFFF0000)            # bytes 12 .. 13: 16 bits off over 16 bytes or more, equal over 12 or 8
    nb[tail_rows] = max(lengths)
    keys = rng.permutation(np.arange(1, n + 1, dtype=np.uint64) * GOLDEN)
    return keys, mask_lengths(words, nb), nb, np.sort(keys[hub_rows])


@pytest.mark.parametrize("lengths,n", [((8, 16, 32), 2100), ((12,), 700), ((12, 16), 900)])
def test_nphd_tables(hip_engine, lengths, n):
    rng = np.random.default_rng(n)
    keys, words, nb, hub_keys = nphd_table(rng, n, list(lengths), 300)
    rows = (keys, words, nb)
    with dropping(table_with(hip_engine, _lib.METRIC_NPHD, 1, 32, *rows)) as (t,):
        results = check_lists(hip_engine, t, rows, thresholds(lengths), hub_keys, n)
        deg, links = results[0]
        assert links >= 300 * 299 // 2 and int(deg.max()) >= 299
        if len(lengths) > 1:
            assert links > 300 * 299 // 2 + 30 * 29 // 2               # the tail rows pair with the shorter hub rows: across segments


# ---- (c) every row equal: the ring fills and is walked mid-step, every counter is hit from every wave
@pytest.mark.parametrize("nbytes", [8, 32])
def test_a_thousand_equal_rows(hip_engine, nbytes):
    n = 1000
    rng = np.random.default_rng(nbytes)
    code = rng.integers(0, 2**64, size=(1, 4), dtype=np.uint64)
    nb = np.full(n, nbytes, dtype=np.uint8)
    words = mask_lengths(np.repeat(code, n, axis=0), nb)
    keys = rng.permutation(np.arange(1, n + 1, dtype=np.uint64) * GOLDEN)
    rows = (keys, words, nb)
    with dropping(table_with(hip_engine, _lib.METRIC_HAMMING, 1, nbytes, *rows)) as (t,):
        deg, links = check(hip_engine, t, rows, thresholds([nbytes], 0), np.sort(keys))
        assert links == 499_500 and deg.tolist() == [999] * n
        deg, links = check(hip_engine, t, rows, thresholds([nbytes], 0), np.sort(keys)[::2])
        assert links == 500 * 499 // 2 and deg.tolist() == [499] * 500


# ---- (d) the capacity protocol of isccsearch_join_within_live
def test_enospc_reports_the_exact_total_and_the_retry_fits(hip_engine):
    rng = np.random.default_rng(77)
    keys, words, nb, hub_keys = planted_table(rng, 700, 8, hub=100)
    rows = (keys, words, nb)
    mh = thresholds([8])
    live = np.setdiff1d(np.sort(keys), hub_keys[::4])
    exp = model.join_within_live(*rows, mh, live)
    total = len(exp[2])
    assert total > 2000
    call = hip_engine._lib.isccsearch_join_within_live

    def once(capacity):
        out = (np.zeros(max(capacity, 1), np.uint64), np.zeros(max(capacity, 1), np.uint64), np.zeros(max(capacity, 1), np.uint32), np.zeros(max(capacity, 1), np.uint16))
        found = ctypes.c_uint64(0)
        rc = call(hip_engine.handle, t.id, _lib.ptr(mh), len(live), _lib.ptr(live), capacity, *(_lib.ptr(a) for a in out), ctypes.byref(found))
        return rc, int(found.value), out

    with dropping(table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, *rows)) as (t,):
        for kernel in (forced, valu):
            with kernel(hip_engine):
                for capacity in (0, 1, total - 1):
                    rc, found, _ = once(capacity)
                    assert rc == -errno.ENOSPC and found == total, (capacity, rc, found)
                rc, found, out = once(total)
                assert rc == 0 and found == total
                for g, e, name in zip(out, exp, NAMES):
                    assert np.array_equal(g, e), name
        # the Python layer retries once with the reported total, and surfaces max_pairs
        with pytest.raises(ValueError, match=f"{total} pairs exceed max_pairs={total - 1}"):
            t.join_within(mh, total - 1, live)
        assert len(t.join_within(mh, total, live)[2]) == total


# ---- (e) refusals: all on the host, nothing launched, the outputs untouched
def test_refusals_leave_the_outputs_untouched(hip_engine):
    rng = np.random.default_rng(51)
    n = 40
    keys, words, nb, _ = planted_table(rng, n, 8)
    live = np.sort(keys)
    mh = thresholds([8], 64)
    degrees_call, live_call = hip_engine._lib.isccsearch_join_degrees, hip_engine._lib.isccsearch_join_within_live
    SENTINEL = 0xA5
    with dropping(table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, keys, words, nb), hip_engine.open_table(_lib.METRIC_HAMMING, 2, 8)) as (t, wide):
        before = counters(hip_engine)

        def refused(message, table=t, mh=mh, n_live=n, live=live, degree=True, links=True, outputs=(True, True, True, True), total=True, which=(0, 1)):
            out_degree = np.full(n, SENTINEL * 0x01010101, dtype=np.uint32)
            out_links = ctypes.c_uint64(SENTINEL)
            outs = (np.full(n * n, SENTINEL, np.uint64), np.full(n * n, SENTINEL, np.uint64), np.full(n * n, SENTINEL, np.uint32), np.full(n * n, SENTINEL, np.uint16))
            out_total = ctypes.c_uint64(SENTINEL)
            if 0 in which:
                rc = degrees_call(hip_engine.handle, table.id, _lib.ptr(mh), n_live, _lib.ptr(live), _lib.ptr(out_degree) if degree else None,
                                  ctypes.byref(out_links) if links else None)
                assert rc == -errno.EINVAL and message in _lib.last_error(), (rc, _lib.last_error())
            if 1 in which:
                rc = live_call(hip_engine.handle, table.id, _lib.ptr(mh), n_live, _lib.ptr(live), n * n,
                               *(_lib.ptr(a) if given else None for a, given in zip(outs, outputs)), ctypes.byref(out_total) if total else None)
                assert rc == -errno.EINVAL and message in _lib.last_error(), (rc, _lib.last_error())
            assert np.all(out_degree == SENTINEL * 0x01010101) and out_links.value == SENTINEL and out_total.value == SENTINEL
            assert all(np.all(a == SENTINEL) for a in outs)

        refused("NULL", mh=None)
        refused("NULL", live=None)
        refused("NULL", degree=False, which=(0,))
        refused("NULL", links=False, which=(0,))
        refused("NULL", total=False, which=(1,))
        for x in range(4):
            refused("NULL output array", outputs=tuple(y != x for y in range(4)), which=(1,))
        refused("key_words", table=wide)
        refused("n_live", n_live=0xFFFFFFFF)
        refused("n_live", n_live=1 << 32)
        swapped = live.copy()
        swapped[[7, 8]] = swapped[[8, 7]]
        refused("live_keys[8]", live=swapped)
        repeated = live.copy()
        repeated[5] = repeated[4]
        refused("live_keys[5]", live=repeated)
        assert counters(hip_engine) == before             # all of it on the host: nothing was launched
        with pytest.raises(ValueError, match=r"live_keys\[8\]"):
            t.join_degrees(mh, swapped)
        with pytest.raises(ValueError, match=r"live_keys\[8\]"):
            t.join_within(mh, 10_000, swapped)
        for call in (lambda: wide.join_degrees(mh, live), lambda: wide.join_within(mh, 10_000, live)):
            with pytest.raises(ValueError, match="64-bit keys"):
                call()
        # ... and the calls that all of these were one argument away from
        deg, links = check(hip_engine, t, (keys, words, nb), mh, live)
        assert links == n * (n - 1) // 2 and deg.tolist() == [n - 1] * n


def test_nothing_to_join_still_fills_the_outputs(hip_engine):
    call = hip_engine._lib.isccsearch_join_degrees
    mh = thresholds([8], 64)
    none = (np.zeros(0, dtype=np.uint64), np.zeros((0, 1), dtype=np.uint64), np.zeros(0, dtype=np.uint8))
    with dropping(hip_engine.open_table(_lib.METRIC_HAMMING, 1, 8)) as (t,):
        for live in ([], [7], [7, 9]):
            deg, links = check(hip_engine, t, none, mh, live)
            assert deg.tolist() == [0] * len(live) and links == 0
        one = (np.array([7], dtype=np.uint64), np.array([[123]], dtype=np.uint64), np.array([8], dtype=np.uint8))
        t.add(one[0], one[1])
        deg, links = check(hip_engine, t, one, mh, [5, 7, 9])
        assert deg.tolist() == [0, 0, 0] and links == 0
        t.add(np.array([9], dtype=np.uint64), np.array([[123]], dtype=np.uint64))
        two = (np.array([7, 9], dtype=np.uint64), np.array([[123], [123]], dtype=np.uint64), np.array([8, 8], dtype=np.uint8))
        before = counters(hip_engine)
        # one listed key: no pair of listed rows, nothing launched, and the outputs (here: a sentinel pattern) are overwritten
        out_degree = np.full(1, 0xA5A5A5A5, dtype=np.uint32)
        out_links = ctypes.c_uint64(0xA5)
        live = np.array([9], dtype=np.uint64)
        assert call(hip_engine.handle, t.id, _lib.ptr(mh), 1, _lib.ptr(live), _lib.ptr(out_degree), ctypes.byref(out_links)) == 0
        assert out_degree.tolist() == [0] and out_links.value == 0 and counters(hip_engine) == before
        # n_live = 0 takes NULL arrays
        assert call(hip_engine.handle, t.id, _lib.ptr(mh), 0, None, None, ctypes.byref(out_links)) == 0 and out_links.value == 0
        deg, links = check(hip_engine, t, two, mh, [5, 7, 9])
        assert deg.tolist() == [0, 1, 1] and links == 1
        # thresholds that admit no prefix: nothing to launch either
        deg, links = t.join_degrees(thresholds([]), [7, 9])
        assert deg.tolist() == [0, 0] and links == 0


# ---- (f) end to end: the index of test_hubs on the device against the oracle-backed engine
def test_find_hubs_and_max_degree_end_to_end(hip_engine):
    oracle = oracle_index()
    idx = HipIndex(hip_engine, HipOptions())
    try:
        idx.add_assets(hub_assets())
        cases = [(lambda i: i.find_hubs(), True), (lambda i: i.find_hubs(min_degree=11), True), (lambda i: i.find_hubs(threshold=1.0), True),
                 (lambda i: i.find_duplicates(max_degree=10, max_pairs=500), True), (lambda i: i.find_duplicates(max_degree=2), True),
                 (lambda i: i.find_duplicate_groups(max_degree=10), True), (lambda i: i.find_duplicates(), True)]
        for call, launches in cases:
            exp = call(oracle)
            got, ref = both_kernels(hip_engine, lambda: call(idx), launches)
            assert exp and got == exp and ref == exp
        with pytest.raises(ValueError, match="exceed max_pairs=500"):
            idx.find_duplicates(max_pairs=500)
    finally:
        idx.close()
