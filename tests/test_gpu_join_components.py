"""
``isccsearch_join_components`` (``HipTable.join_components``) and ``find_duplicate_groups`` on an MI355X.

Every case runs on BOTH kernels -- the matrix-core form under ``mfma=1, join_mfma=1, join_mfma_min_rows=0`` and the XOR + popcount
form under ``join_mfma=0`` -- from the same input array, reads the statistics to see which kernel ran, and compares ``parent`` and the
links of either with the host model (``components_model``: brute-force pairs, a dict union-find) and with each other, for exact
equality.  No table has more than 5 000 rows; the sizes are those at which the two emit paths change behaviour: 16 rows per block
and 2 048-row slabs on the VALU kernel; 32-row groups, 64-row steps, the 1 024-row chunk and the second block on the matrix cores.
"""

import ctypes
import errno

import numpy as np
import pytest

import components_model as model
from iscc_search_amd import _lib
from iscc_search_amd.index import HipIndex, HipOptions
from test_duplicate_groups import bfs_groups
from test_duplicates import build_assets
from test_gpu_duplicates import mask_lengths, planted, table_with
from test_gpu_join_mfma import N_TWO_BLOCKS, counters, dropping, forced, valu
from test_gpu_matches import only

pytestmark = pytest.mark.gpu


def both_kernels(engine, table, mh, live_keys, live_labels, parent_in, launches=True):
    """One call per kernel from copies of ``parent_in``: (parent, links), equal on both, the counters saying which kernel ran."""
    live_keys = np.asarray(live_keys, dtype=np.uint64)
    live_labels = np.asarray(live_labels, dtype=np.uint32)
    l0, m0 = counters(engine)
    on_mfma = np.array(parent_in, dtype=np.uint32)
    with forced(engine):
        links_mfma = table.join_components(mh, live_keys, live_labels, on_mfma)
    l1, m1 = counters(engine)
    on_valu = np.array(parent_in, dtype=np.uint32)
    with valu(engine):
        links_valu = table.join_components(mh, live_keys, live_labels, on_valu)
    l2, m2 = counters(engine)
    if launches:
        assert m1 > m0 and l1 - l0 == m1 - m0, "the forced call did not run on the matrix cores alone"
        assert m2 == m1 and l2 > l1, "the join_mfma=0 call did not run on the VALU kernel alone"
    else:
        assert (l2, m2) == (l0, m0), "nothing to join: nothing launched"
    assert links_mfma == links_valu, "links (matrix cores against VALU)"
    assert np.array_equal(on_mfma, on_valu), "parent (matrix cores against VALU)"
    return on_mfma, links_mfma


def check(engine, table, rows, mh, live_keys, live_labels, parent_in, launches=True):
    """Both kernels against the model of one call over ``rows`` = (keys, words, nb)."""
    got, links = both_kernels(engine, table, mh, live_keys, live_labels, parent_in, launches)
    exp, exp_links = model.join_components(*rows, mh, live_keys, live_labels, parent_in)
    assert links == exp_links, "links against the model"
    assert got.dtype == np.uint32 and np.array_equal(got, exp), "parent against the model"
    return got, links


def identity(n):
    return np.arange(n, dtype=np.uint32)


def ranked(keys):
    """live_keys = all keys ascending, label = rank"""
    live = np.sort(np.asarray(keys, dtype=np.uint64))
    return live, identity(len(live))


def hamming64(rng, n, pool=None):
    words = planted(rng, n, 8, pool=pool if pool is not None else max(2, n // 30))
    keys = rng.permutation(np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))     # labels unrelated to row order
    return keys, words, np.full(n, 8, dtype=np.uint8)


# ---- (a) ordinary tables
@pytest.mark.parametrize("n", [2, 17, 65, 1025, 2049, N_TWO_BLOCKS])
def test_hamming64_all_keys_live(hip_engine, n):
    rng = np.random.default_rng(n)
    rows = hamming64(rng, n)
    rows[1][1] = rows[1][0]                          # one pair at distance 0 in every size
    live, labels = ranked(rows[0])
    with dropping(table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, *rows)) as (t,):
        for tau in (0, 5):
            got, links = check(hip_engine, t, rows, only(8, tau), live, labels, identity(n))
            assert links == len(t.join_within(only(8, tau), 10_000_000)[2]) > 0
            assert np.all(got <= identity(n)) and np.array_equal(got[got], got)          # flat, roots the minima


# ---- (b) one dense component
def test_one_dense_component(hip_engine):
    n = 1025
    rng = np.random.default_rng(5)
    keys, words, nb = hamming64(rng, n)
    same = np.repeat(words[:1], n, axis=0)
    live, labels = ranked(keys)
    with dropping(table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, keys, same, nb)) as (t,):
        got, links = check(hip_engine, t, (keys, same, nb), only(8, 0), live, labels, identity(n))     # every union on the same few roots
        assert links == n * (n - 1) // 2 == 524_800 and not got.any()
    with dropping(table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, keys, words, nb)) as (t,):
        got, links = check(hip_engine, t, (keys, words, nb), only(8, 64), live, labels, identity(n))   # the ring fills and is walked many times per step
        assert links == n * (n - 1) // 2 and not got.any()


# ---- (c) deep paths: thermometer codes, row i of a chain = base ^ (i leading ones), so h(i, j) = |i - j|; tau = 1 links neighbours only
def leading_ones(i, W):
    out = np.zeros(4, dtype=np.uint64)
    for w in range(W):
        k = min(max(i - 64 * w, 0), 64)
        out[w] = np.uint64(((1 << k) - 1) << (64 - k))
    return out


def chains(rng, n_chains, length, W):
    """(words [n_chains * length, 4], position of every row along its chain); rows chain by chain"""
    ones = np.stack([leading_ones(i, W) for i in range(length)])
    base = rng.integers(0, 2**64, size=(n_chains, 4), dtype=np.uint64)
    base[:, W:] = 0
    words = (base[:, None, :] ^ ones[None, :, :]).reshape(n_chains * length, 4)
    return words, np.tile(np.arange(length), n_chains)


@pytest.mark.parametrize("order", ["permuted", "ascending", "descending"])
@pytest.mark.parametrize("nbytes,n_chains,length", [(32, 12, 257), (8, 40, 65)])
def test_deep_paths(hip_engine, nbytes, n_chains, length, order):
    rng = np.random.default_rng(nbytes)
    W = nbytes // 8
    words, pos = chains(rng, n_chains, length, W)
    n = len(words)
    chain = np.repeat(np.arange(n_chains), length)
    along = {"ascending": pos, "descending": length - 1 - pos}.get(order)
    if along is None:
        along = np.concatenate([rng.permutation(length) for _ in range(n_chains)])
    row_label = (chain * length + along).astype(np.uint32)            # labels along each chain in the order asked for
    keys = rng.permutation(np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    store = rng.permutation(n)                                         # rows stored in no order either
    srt = np.argsort(keys)
    nb = np.full(n, nbytes, dtype=np.uint8)
    rows = (keys[store], words[store], nb)
    with dropping(table_with(hip_engine, _lib.METRIC_HAMMING, 1, nbytes, *rows)) as (t,):
        got, links = check(hip_engine, t, rows, only(nbytes, 1), keys[srt], row_label[srt], identity(n))
        assert links >= n_chains * (length - 1)
        assert len(np.unique(got)) <= n_chains and np.all(got[row_label] <= chain * length)     # a chain is one component


# ---- (d) across segments: NPHD lengths {8, 12, 16, 24, 32}, max_hamming[p] = p
def test_nphd_across_segments(hip_engine):
    rng = np.random.default_rng(13)
    lengths = [8, 12, 16, 24, 32]
    n_fill, n_tri = 2400, 60
    words = planted(rng, n_fill, 32, pool=120, flips=8)
    nb = rng.choice(lengths, size=n_fill).astype(np.uint8)
    # triples: an 8-byte row 3 bits off the first word of a 16-byte and of a 32-byte row that differ in 32 bits of their second word
    base = rng.integers(0, 2**64, size=(n_tri, 4), dtype=np.uint64)
    r32, r16, r8 = base.copy(), base.copy(), base.copy()
    r16[:, 1] ^= np.uint64(0x00000000FFFFFFFF)
    r8[:, 0] ^= np.uint64(0b111)
    words = np.concatenate([words, r8, r16, r32])
    nb = np.concatenate([nb, np.full(n_tri, 8), np.full(n_tri, 16), np.full(n_tri, 32)]).astype(np.uint8)
    words = mask_lengths(words, nb)
    n = len(nb)
    keys = rng.permutation(n).astype(np.uint64) + np.uint64(10)
    mh = np.full(33, -1, dtype=np.int16)
    for p in lengths:
        mh[p] = p
    live, labels = ranked(keys)
    rows = (keys, words, nb)
    with dropping(table_with(hip_engine, _lib.METRIC_NPHD, 1, 32, *rows)) as (t,):
        got, links = check(hip_engine, t, rows, mh, live, labels, identity(n))
        assert links == len(t.join_within(mh, 10_000_000)[2])
        tri = np.searchsorted(live, keys[n_fill:]).reshape(3, n_tri)
        assert np.array_equal(got[tri[0]], got[tri[1]]) and np.array_equal(got[tri[0]], got[tri[2]])
        # without the 8-byte rows' labels only what else joins a pair of them still does
        rest = np.concatenate([keys[:n_fill], keys[n_fill + n_tri:]])
        live2, labels2 = ranked(rest)
        got2, links2 = check(hip_engine, t, rows, mh, live2, labels2, identity(len(rest)))
        assert links2 < links


# ---- (e) rows without a label
def test_bridge_row_without_a_label(hip_engine):
    rng = np.random.default_rng(21)
    x = int(rng.integers(0, 2**63))
    words = rng.integers(0, 2**64, size=(103, 1), dtype=np.uint64)
    words[:3, 0] = [x, x ^ 1, x ^ 3]                  # A ~ S ~ B at one bit each, A and B two bits apart
    keys = np.arange(100, 203, dtype=np.uint64)
    nb = np.full(103, 8, dtype=np.uint8)
    rows = (keys, words, nb)
    with dropping(table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, *rows)) as (t,):
        got, links = check(hip_engine, t, rows, only(8, 1), keys, identity(103), identity(103))
        assert got[:3].tolist() == [0, 0, 0] and links >= 2
        live = np.delete(keys, 1)                     # S is compared, never linked, never counted
        got, links_without = check(hip_engine, t, rows, only(8, 1), live, identity(102), identity(102))
        assert got[0] == 0 and got[1] == 1 and links_without == links - 2
        # a listed key the table does not hold is a vertex of its own and changes nothing else
        live = np.concatenate([np.delete(keys, 1), [np.uint64(5000)]])
        got, links_absent = check(hip_engine, t, rows, only(8, 1), live, identity(103), identity(103))
        assert got[0] == 0 and got[1] == 1 and got[102] == 102 and links_absent == links_without


def test_half_the_keys_live_and_shared_labels(hip_engine):
    rng = np.random.default_rng(22)
    n = 1025
    rows = hamming64(rng, n)
    with dropping(table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, *rows)) as (t,):
        live = np.sort(rng.choice(rows[0], size=n // 2, replace=False))
        labels = rng.permutation(len(live)).astype(np.uint32)
        _, links_half = check(hip_engine, t, rows, only(8, 5), live, labels, identity(len(live)))
        _, links_all = check(hip_engine, t, rows, only(8, 5), *ranked(rows[0]), identity(n))
        assert 0 < links_half < links_all
        # two keys sharing a label are one vertex
        live, rank = ranked(rows[0])
        got, links_shared = check(hip_engine, t, rows, only(8, 5), live, rank // 2, identity((n + 1) // 2))
        assert links_shared == links_all


# ---- (f) parent in and out
def test_parent_in_and_out(hip_engine):
    rng = np.random.default_rng(31)
    n = 2049
    rows = hamming64(rng, n)
    live, labels = ranked(rows[0])
    part_a, part_b = labels % 3 != 0, labels % 3 != 1
    with dropping(table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, *rows)) as (t,):
        # two calls with different thresholds and live rows, the second on the first's output = one model run over both edge sets
        first, links_a = check(hip_engine, t, rows, only(8, 2), live[part_a], labels[part_a], identity(n))
        second, links_b = check(hip_engine, t, rows, only(8, 5), live[part_b], labels[part_b], first)
        edges = model.linked_pairs(*rows, only(8, 2), live[part_a], labels[part_a]) + model.linked_pairs(*rows, only(8, 5), live[part_b], labels[part_b])
        assert links_a + links_b == len(edges)
        assert np.array_equal(second, model.components(n, identity(n), edges)) and not np.array_equal(first, second)
        # calling again with the output changes nothing
        again, links_again = check(hip_engine, t, rows, only(8, 5), live[part_b], labels[part_b], second)
        assert np.array_equal(again, second) and links_again == links_b
        # a hand-made input forest that is not flat: chains 9 -> 8 -> .. -> 0, 19 -> .. -> 10, .., and every 7th label under label 3
        forest = identity(n)
        forest[1:1000] = np.where(np.arange(1, 1000) % 10 != 0, np.arange(0, 999), np.arange(1, 1000))
        forest[1001::7] = 3
        assert np.all(forest <= identity(n)) and not np.array_equal(forest[forest], forest)
        got, _ = check(hip_engine, t, rows, only(8, 2), live, labels, forest)
        assert not np.array_equal(got, first)


def test_two_tables_in_sequence(hip_engine):
    rng = np.random.default_rng(32)
    x, y, z = (int(v) for v in rng.integers(0, 2**63, size=3))
    keys = np.array([11, 22, 33], dtype=np.uint64)       # assets A, B, C in both tables
    nb = np.full(3, 8, dtype=np.uint8)
    first = (keys, np.array([[x], [x ^ 1], [y]], dtype=np.uint64), nb)      # A ~ B only
    second = (keys, np.array([[z], [y], [y ^ 2]], dtype=np.uint64), nb)     # B ~ C only
    with dropping(table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, *first), table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, *second)) as (t1, t2):
        parent, links = check(hip_engine, t1, first, only(8, 1), keys, identity(3), identity(3))
        assert parent.tolist() == [0, 0, 2] and links == 1
        parent, links = check(hip_engine, t2, second, only(8, 1), keys, identity(3), parent)
        assert parent.tolist() == [0, 0, 0] and links == 1


# ---- (g) after removals: the rows behind the segment's end link nothing
def test_after_removals(hip_engine):
    rng = np.random.default_rng(41)
    n = 3000
    keys, words, nb = hamming64(rng, n, pool=60)
    live, labels = ranked(keys)                          # still lists the removed keys
    with dropping(table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, keys, words, nb)) as (t,):
        _, links_before = check(hip_engine, t, (keys, words, nb), only(8, 4), live, labels, identity(n))
        gone = rng.choice(n, size=700, replace=False)
        assert t.remove(keys[gone]) == 700
        keep = np.setdiff1d(np.arange(n), gone)
        got, links = check(hip_engine, t, (keys[keep], words[keep], nb[keep]), only(8, 4), live, labels, identity(n))
        assert 0 < links < links_before
        removed = np.searchsorted(live, keys[gone])
        assert np.array_equal(got[removed], removed)     # a removed row's label is alone


# ---- (h) refusals, and tables with nothing to join
def test_refusals_leave_parent_unchanged(hip_engine):
    rng = np.random.default_rng(51)
    n = 40
    rows = hamming64(rng, n)
    live, labels = ranked(rows[0])
    call = hip_engine._lib.isccsearch_join_components
    mh = only(8, 64)
    with dropping(table_with(hip_engine, _lib.METRIC_HAMMING, 1, 8, *rows), hip_engine.open_table(_lib.METRIC_HAMMING, 2, 8)) as (t, wide):
        before = counters(hip_engine)

        def refused(table=t, mh=mh, n_live=n, live=live, labels=labels, n_labels=n, parent=identity(n), links=True, message=""):
            parent = None if parent is None else np.array(parent, dtype=np.uint32)
            kept = None if parent is None else parent.tobytes()
            out = ctypes.c_uint64(77)
            rc = call(hip_engine.handle, table.id, _lib.ptr(mh), n_live, _lib.ptr(live), _lib.ptr(labels), n_labels, _lib.ptr(parent),
                      ctypes.byref(out) if links else None)
            assert rc == -errno.EINVAL and message in _lib.last_error(), (rc, _lib.last_error())
            assert parent is None or parent.tobytes() == kept

        refused(mh=None, message="NULL")
        refused(live=None, message="NULL")
        refused(labels=None, message="NULL")
        refused(parent=None, message="NULL")
        refused(links=False, message="NULL")
        refused(table=wide, message="key_words")
        refused(n_labels=0, message="n_labels")
        refused(n_labels=0xFFFFFFFF, message="n_labels")
        swapped = live.copy()
        swapped[[7, 8]] = swapped[[8, 7]]
        refused(live=swapped, message="live_keys[8]")
        repeated = live.copy()
        repeated[5] = repeated[4]
        refused(live=repeated, message="live_keys[5]")
        high = labels.copy()
        high[9] = n
        refused(labels=high, message="live_labels[9]")
        above = identity(n)
        above[11] = 12
        refused(parent=above, message="parent[11]")
        assert counters(hip_engine) == before             # all of it on the host: nothing was launched
        with pytest.raises(ValueError, match=r"parent\[11\]"):
            t.join_components(mh, live, labels, above)
        with pytest.raises(ValueError, match="64-bit keys"):
            wide.join_components(mh, live, labels, identity(n))
        with pytest.raises(ValueError, match="uint32"):
            t.join_components(mh, live, labels, np.arange(n, dtype=np.int64))
        # ... and the call that all of these were one argument away from
        got, links = check(hip_engine, t, rows, mh, live, labels, identity(n))
        assert links == n * (n - 1) // 2 and not got.any()


def test_empty_and_one_row_tables(hip_engine):
    forest = np.array([0, 0, 1, 2, 4], dtype=np.uint32)      # not flat: flattened even where nothing is joined
    with dropping(hip_engine.open_table(_lib.METRIC_HAMMING, 1, 8)) as (t,):
        none = (np.zeros(0, dtype=np.uint64), np.zeros((0, 1), dtype=np.uint64), np.zeros(0, dtype=np.uint8))
        got, links = check(hip_engine, t, none, only(8, 64), [7], [4], forest, launches=False)
        assert got.tolist() == [0, 0, 0, 0, 4] and links == 0
        got, links = check(hip_engine, t, none, only(8, 64), [], [], forest, launches=False)
        assert got.tolist() == [0, 0, 0, 0, 4] and links == 0
        one = (np.array([7], dtype=np.uint64), np.array([[123]], dtype=np.uint64), np.array([8], dtype=np.uint8))
        t.add(one[0], one[1])
        got, links = check(hip_engine, t, one, only(8, 64), [7], [4], forest, launches=False)
        assert got.tolist() == [0, 0, 0, 0, 4] and links == 0


# ---- (i) end to end
def test_find_duplicate_groups_end_to_end(hip_engine):
    idx = HipIndex(hip_engine, HipOptions())
    strict = HipIndex(hip_engine, HipOptions(match_threshold_units=0.9))
    try:
        assets = build_assets(np.random.default_rng(17), 2000)
        idx.add_assets(assets)
        strict.add_assets(assets)
        cases = [(dict(), idx, {}), (dict(unit_types=["DATA_NONE_V0", "INSTANCE_NONE_V0"]), idx, dict(unit_types=["DATA_NONE_V0", "INSTANCE_NONE_V0"])),
                 (dict(threshold=0.9), strict, {})]
        for kwargs, pairs_of, pair_kwargs in cases:
            exp = bfs_groups(pairs_of, pairs_of.find_duplicates(**pair_kwargs))
            l0, m0 = counters(hip_engine)
            with forced(hip_engine):
                got = idx.find_duplicate_groups(**kwargs)
            l1, m1 = counters(hip_engine)
            with valu(hip_engine):
                ref = idx.find_duplicate_groups(**kwargs)
            l2, m2 = counters(hip_engine)
            assert m1 > m0 and l1 - l0 == m1 - m0 and m2 == m1 and l2 > l1
            assert len(exp) > 20 and [g.iscc_ids for g in got] == exp and got == ref
            assert all(g.size == len(g.iscc_ids) for g in got)
    finally:
        idx.close()
        strict.close()
