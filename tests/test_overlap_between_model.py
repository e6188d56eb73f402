"""
The host model of ``isccsearch_join_overlaps_between`` (``tests/overlap_between_model.py``) against cases worked by hand, against a plain
triple loop and against the self-join's model on the union table (CPU tier).  The GPU tier (``test_gpu_overlaps_between.py``) and
``test_shared_matches.py`` rest on this model.
"""

import numpy as np
import pytest

from overlap_between_model import ENOSPC, INFO_NAMES, SKIP_SAME_ASSET, chunk_keys, model_overlaps_between
from overlap_model import model_overlaps
from test_overlap_model import code, table

EMPTY = (np.zeros((0, 2), np.uint64), np.zeros((0, 1), np.uint64))


def as_tuples(records):
    return [tuple(int(r[f]) for f in ("reserved", "src", "dst", "matched", "sum_hamming", "chunk_pairs")) for r in records]


def info_of(*values):
    return dict(zip(INFO_NAMES, values))


def test_the_smallest_distance_two_sided():
    s = code(0, 20, 40)
    cands = [s ^ code(1, 2, 3, 4, 5), s ^ code(6, 7), s ^ code(8, 9)]          # 5, 2 and 2 bits off s
    ka, wa = table([(1, s)])
    kb, wb = table([(2, c) for c in cands])
    rc, rec, chunks_a, chunks_b, info = model_overlaps_between(ka, wa, kb, wb, [1], [2], 5)
    assert rc == 0
    # A -> B: ONE matched row with its smallest distance 2, three chunk pairs; B -> A: three matched rows, 5 + 2 + 2
    assert as_tuples(rec) == [(0, 0, 0, 1, 2, 3), (1, 0, 0, 3, 9, 3)]
    assert chunks_a.tolist() == [1] and chunks_b.tolist() == [3] and info == info_of(3, 2, 1, 0, 3, 0)
    # the sides swapped: the same two records with the directions exchanged
    rc, rec, chunks_a, chunks_b, info = model_overlaps_between(kb, wb, ka, wa, [2], [1], 5)
    assert as_tuples(rec) == [(0, 0, 0, 3, 9, 3), (1, 0, 0, 1, 2, 3)] and info == info_of(3, 2, 3, 0, 1, 0)
    # radius 2: the candidate at distance 5 is out of reach
    rc, rec, _, _, info = model_overlaps_between(ka, wa, kb, wb, [1], [2], 2)
    assert as_tuples(rec) == [(0, 0, 0, 1, 2, 2), (1, 0, 0, 2, 4, 2)]


def test_two_label_spaces_and_the_order_of_the_records():
    x, y = code(1, 9), code(2, 17, 40)
    ka, wa = table([(10, x), (30, y), (30, x)])
    kb, wb = table([(7, y), (20, x), (20, y ^ 1)])
    rc, rec, chunks_a, chunks_b, info = model_overlaps_between(ka, wa, kb, wb, [10, 30], [7, 20, 25], 1)
    # labels: A 10 -> 0, 30 -> 1; B 7 -> 0, 20 -> 1, 25 -> 2 (no rows)
    assert as_tuples(rec) == [
        (0, 0, 1, 1, 0, 1),          # 10 -> 20: x
        (0, 1, 0, 1, 0, 1),          # 30 -> 7: y
        (0, 1, 1, 2, 1, 2),          # 30 -> 20: y finds y ^ 1 at distance 1, x finds x
        (1, 0, 1, 1, 0, 1),          # 7 -> 30
        (1, 1, 0, 1, 0, 1),          # 20 -> 10
        (1, 1, 1, 2, 1, 2),          # 20 -> 30: x at 0, y ^ 1 at 1
    ]
    assert chunks_a.tolist() == [1, 2] and chunks_b.tolist() == [1, 2, 0] and info == info_of(4, 6, 3, 0, 3, 0)


def test_stop_chunks_are_decided_per_table():
    boiler = code(3, 33)
    ka, wa = table([(1000, boiler), (1000, code(5))])
    kb, wb = table([(a, boiler) for a in range(1, 51)] + [(60, code(9))])
    listed_b = list(range(1, 51)) + [60]
    # in B 50 assets hold the chunk: above a cut of 49 (in A one asset holds it: A's row is no stop chunk, but has nothing left to pair with)
    rc, rec, chunks_a, chunks_b, info = model_overlaps_between(ka, wa, kb, wb, [1000], listed_b, 0, max_doc_freq=49)
    assert rc == 0 and len(rec) == 0 and info == info_of(0, 0, 2, 0, 51, 50)
    assert chunks_a.tolist() == [2] and chunks_b.tolist() == [1] * 51          # stop chunks still count
    rc, rec, chunks_a, chunks_b, info = model_overlaps_between(ka, wa, kb, wb, [1000], listed_b, 0, max_doc_freq=50)
    assert info == info_of(50, 100, 2, 0, 51, 0)
    assert as_tuples(rec)[:2] == [(0, 0, 0, 1, 0, 1), (0, 0, 1, 1, 0, 1)] and as_tuples(rec)[50] == (1, 0, 0, 1, 0, 1)
    # the other way round: a chunk frequent in A only stops A's rows
    rc, rec, _, _, info = model_overlaps_between(kb, wb, ka, wa, listed_b, [1000], 0, max_doc_freq=49)
    assert len(rec) == 0 and info == info_of(0, 0, 51, 50, 2, 0)
    # the union table would count 51 holders: per table the cut of 50 lets the chunk through
    assert model_overlaps_between(ka, wa, kb, wb, [1000], listed_b, 0, max_doc_freq=50, dup_limit=50)[4]["chunk_pairs"] == 50


def test_the_same_asset_flag_both_ways():
    x, y = code(7, 8), code(12)
    ka, wa = table([(5, x), (5, y), (6, x)])
    kb, wb = table([(5, x), (5, x), (9, y)])
    rc, rec, chunks_a, chunks_b, info = model_overlaps_between(ka, wa, kb, wb, [5, 6], [5, 9], 0, flags=SKIP_SAME_ASSET)
    # asset 5 is held by both tables: its chunks do not pair with each other, 6 -> 5 and 5 -> 9 do
    assert as_tuples(rec) == [(0, 0, 1, 1, 0, 1), (0, 1, 0, 1, 0, 2), (1, 0, 1, 2, 0, 2), (1, 1, 0, 1, 0, 1)]
    assert info == info_of(3, 4, 3, 0, 3, 0)
    rc, rec, chunks_a, chunks_b, info = model_overlaps_between(ka, wa, kb, wb, [5, 6], [5, 9], 0, flags=0)
    assert as_tuples(rec) == [(0, 0, 0, 1, 0, 2), (0, 0, 1, 1, 0, 1), (0, 1, 0, 1, 0, 2), (1, 0, 0, 2, 0, 2), (1, 0, 1, 2, 0, 2), (1, 1, 0, 1, 0, 1)]
    assert info == info_of(5, 6, 3, 0, 3, 0)
    # only same-asset pairs: with the flag capacity 0 is enough
    rc, rec, _, _, info = model_overlaps_between(ka[:1], wa[:1], kb[:2], wb[:2], [5], [5], 0, capacity=0)
    assert rc == 0 and len(rec) == 0 and info["chunk_pairs"] == 0
    assert model_overlaps_between(ka[:1], wa[:1], kb[:2], wb[:2], [5], [5], 0, flags=0, capacity=1)[0] == ENOSPC


def test_unlisted_assets_and_a_listed_asset_without_rows():
    x = code(11)
    ka, wa = table([(1, x), (2, x)])
    kb, wb = table([(3, x), (4, x)])
    rc, rec, chunks_a, chunks_b, info = model_overlaps_between(ka, wa, kb, wb, [1, 8], [2, 4], 0)     # A's 2 and B's 3 unlisted; 8 and B's 2 without rows
    assert as_tuples(rec) == [(0, 0, 1, 1, 0, 1), (1, 1, 0, 1, 0, 1)]
    assert chunks_a.tolist() == [1, 0] and chunks_b.tolist() == [0, 1] and info == info_of(1, 2, 1, 0, 1, 0)


def test_capacity_outcome():
    x = code(4)
    ka, wa = table([(1, x), (2, x)])
    kb, wb = table([(3, x), (4, x)])
    rc, rec, _, _, info = model_overlaps_between(ka, wa, kb, wb, [1, 2], [3, 4], 0, capacity=3)
    assert rc == ENOSPC and rec is None and info == {"chunk_pairs": 4}
    rc, rec, _, _, info = model_overlaps_between(ka, wa, kb, wb, [1, 2], [3, 4], 0, capacity=4)
    assert rc == 0 and info["records"] == 8 and info["chunk_pairs"] == 4


def test_empty_tables():
    ka, wa = table([(2, code(1)), (3, code(1))])
    for a, b, exp in (((ka, wa), EMPTY, info_of(0, 0, 2, 0, 0, 0)), (EMPTY, (ka, wa), info_of(0, 0, 0, 0, 2, 0)), (EMPTY, EMPTY, info_of(0, 0, 0, 0, 0, 0))):
        rc, rec, chunks_a, chunks_b, info = model_overlaps_between(*a, *b, [2, 3], [2, 3], 64, max_doc_freq=2)
        assert rc == 0 and len(rec) == 0 and info == exp
        assert int(chunks_a.sum()) == exp["live_rows_a"] and int(chunks_b.sum()) == exp["live_rows_b"]


def random_side(rng, n, W, pool, first_asset, n_assets):
    words = pool[rng.integers(0, len(pool), size=n)].copy()
    for i in range(n):
        for _ in range(int(rng.integers(0, 4))):
            words[i, rng.integers(0, W)] ^= np.uint64(1) << np.uint64(rng.integers(0, 64))
    assets = rng.integers(first_asset, first_asset + n_assets, size=n)
    return chunk_keys(assets, offsets=rng.permutation(n)), words


def triple_loop(keys_a, words_a, keys_b, words_b, listed_a, listed_b, max_hamming, max_doc_freq, dup_limit, skip):
    """The definition, spelled out with Python ints."""
    sides = []
    for keys, words, listed in ((keys_a, words_a, listed_a), (keys_b, words_b, listed_b)):
        listed = [int(a) for a in listed]
        asset = [int(k[0]) for k in keys]
        codes = [tuple(int(w) for w in row) for row in words]
        live = [a in listed for a in asset]
        stop = [False] * len(keys)
        if max_doc_freq > 0:
            by_code = {}
            for i, c in enumerate(codes):
                by_code.setdefault(c, []).append(i)
            for rows in by_code.values():
                first = sorted(rows, key=lambda j: (int(keys[j][0]), int(keys[j][1])))[:dup_limit]
                for i in rows:
                    stop[i] = live[i] and len({asset[j] for j in first}) > max_doc_freq
        sides.append((listed, asset, codes, live, stop))
    (la, aa, ca, va, sa), (lb, ab, cb, vb, sb) = sides
    recs, total = {}, 0
    for i in range(len(aa)):
        if not va[i] or sa[i]:
            continue
        for j in range(len(ab)):
            if not vb[j] or sb[j] or (skip and aa[i] == ab[j]):
                continue
            h = sum(bin(x ^ y).count("1") for x, y in zip(ca[i], cb[j]))
            if h > max_hamming:
                continue
            total += 1
            for k, row in (((0, la.index(aa[i]), lb.index(ab[j])), i), ((1, lb.index(ab[j]), la.index(aa[i])), j)):
                r = recs.setdefault(k, {})
                r[row] = min(r.get(row, h), h)
                r["pairs"] = r.get("pairs", 0) + 1
    out = []
    for k, r in sorted(recs.items()):
        pairs = r.pop("pairs")
        out.append(k + (len(r), sum(r.values()), pairs))
    chunks_a = [sum(1 for i in range(len(aa)) if va[i] and aa[i] == a) for a in la]
    chunks_b = [sum(1 for j in range(len(ab)) if vb[j] and ab[j] == a) for a in lb]
    return out, chunks_a, chunks_b, info_of(total, len(out), sum(va), sum(sa), sum(vb), sum(sb))


@pytest.mark.parametrize("seed", range(4))
def test_against_a_triple_loop(seed):
    rng = np.random.default_rng(seed)
    n_a, n_b = int(rng.integers(150, 320)), int(rng.integers(150, 320))
    W = int(rng.choice([1, 2, 4]))
    pool = rng.integers(0, 2**64, size=(40, W), dtype=np.uint64)
    # the asset ranges overlap: some assets are held by both tables
    ka, wa = random_side(rng, n_a, W, pool, 1, 40)
    kb, wb = random_side(rng, n_b, W, pool, 25, 40)
    listed_a = np.unique(np.concatenate([ka[rng.random(n_a) < 0.8, 0], [999]])).astype(np.uint64)
    listed_b = np.unique(np.concatenate([kb[rng.random(n_b) < 0.8, 0], [998]])).astype(np.uint64)
    for max_hamming, max_doc_freq, dup_limit, flags in ((0, 0, 1000, 1), (3, 0, 1000, 0), (3, 4, 1000, 1), (5, 2, 6, 0)):
        rc, rec, chunks_a, chunks_b, info = model_overlaps_between(ka, wa, kb, wb, listed_a, listed_b, max_hamming, max_doc_freq, dup_limit, flags)
        exp = triple_loop(ka, wa, kb, wb, listed_a, listed_b, max_hamming, max_doc_freq, dup_limit, bool(flags))
        assert rc == 0 and info["chunk_pairs"] > 0
        assert (as_tuples(rec), chunks_a.tolist(), chunks_b.tolist(), info) == exp


@pytest.mark.parametrize("seed", range(4))
def test_against_the_self_join_of_the_union_table(seed):
    """Disjoint asset keys, no frequency cut: the self-join of A and B in one table, all assets listed, restricted to the pairs with one
    asset from each side, has the same matched, sum_hamming and chunk_pairs per ordered pair."""
    rng = np.random.default_rng(100 + seed)
    n_a, n_b = int(rng.integers(100, 300)), int(rng.integers(100, 300))
    W = int(rng.choice([1, 2]))
    pool = rng.integers(0, 2**64, size=(30, W), dtype=np.uint64)
    ka, wa = random_side(rng, n_a, W, pool, 1, 30)
    kb, wb = random_side(rng, n_b, W, pool, 1001, 30)
    listed_a, listed_b = np.unique(ka[:, 0]), np.unique(kb[:, 0])
    union = np.concatenate([listed_a, listed_b])              # ascending: every key of A is below every key of B
    for max_hamming in (0, 4):
        rc, rec, chunks_a, chunks_b, info = model_overlaps_between(ka, wa, kb, wb, listed_a, listed_b, max_hamming)
        rc_u, rec_u, chunks_u, info_u = model_overlaps(np.concatenate([ka, kb]), np.concatenate([wa, wb]), union, max_hamming)
        assert rc == 0 and rc_u == 0 and len(rec) > 0
        n = len(listed_a)
        exp = []
        for r in rec_u:
            src, dst = int(r["src"]), int(r["dst"])
            if (src < n) == (dst < n):
                continue                                       # both assets of one side
            direction = int(src >= n)
            exp.append((direction, src - n * direction, dst - n * (1 - direction), int(r["matched"]), int(r["sum_hamming"]), int(r["chunk_pairs"])))
        assert as_tuples(rec) == sorted(exp)
        assert chunks_a.tolist() == chunks_u[:n].tolist() and chunks_b.tolist() == chunks_u[n:].tolist()
        assert sum(t[5] for t in exp) == 2 * info["chunk_pairs"]
