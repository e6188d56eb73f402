#!/usr/bin/env python3
"""
Rate of the device joins (isccsearch_join_within and isccsearch_join_between) on synthetic tables, on the XOR + popcount kernel
(csrc/join.hip.h), on the matrix cores (csrc/mfma_join_kernel.hip.h) or on both in one run.

Tables: 64-bit HAMMING rows at 64 Ki, 256 Ki, 1 Mi and 4 Mi rows, and 256-bit NPHD tables (all rows 32 bytes) at 256 Ki and 1 Mi
rows.  Synthetic rows are random words (isccsearch_add_synthetic), so almost no pair is within the threshold and the time is that
of the scan: n(n-1)/2 pair distances for the self-join, n x n for --between (two tables of n different random rows each, or of
--rows-a x --rows-b rows).  One JSON line per table.

--mfma 0 | 1: the XOR + popcount kernel (option join_mfma=0) or the matrix cores for every launch (join_mfma=1,
join_mfma_min_rows=0).  A leg is one warm-up call and the MEDIAN of --reps timed calls.  The line carries seconds and pair
distances per second; for the XOR + popcount kernel also the fraction of the VALU issue rate -- 64 lanes / ((4 W + 0.5)
instructions x 4 cycles) per SIMD and clock, the figure bench.py uses for that scan (W = 64-bit words per row).
--mfma both (the default): three legs per table in the order VALU, matrix cores, VALU (A B A), so that a drift of the box shows
between the two VALU legs.  The line carries the three rates and `ratio` = matrix cores / mean of the two VALU legs, and the tool
asserts that the legs found the same number of pairs.

--components: isccsearch_join_components (the joins' LINK form: pairs united in a union-find array on the device) against
isccsearch_join_within of the SAME build and run, on the same tables.  Per table and kernel three legs A B A (join_within,
join_components, join_within), each one warm-up call and the median of --reps; `ratio` = join_components / mean of the two
join_within legs, and `around_the_joins_seconds` is a join_components call with every prefix excluded: the labels of the rows, the
flatten step and the copies of the arrays, without a join launch.  Then the DENSE table join_within cannot answer under the default
max_pairs: --dense-rows 64-bit rows (default 1 Mi) in clusters of --cluster identical rows, tau 0, on both kernels: seconds, links,
nanoseconds per link.

--overlaps: isccsearch_join_overlaps (the joins' OVERLAP form and the aggregation of csrc/overlap.hip) on simprint tables: 64-bit and
128-bit simprints, 128-bit keys, about 16 chunks per asset in random row order, --shared per cent of the assets containing a run of
4-8 chunks of another asset (0-2 bits flipped).  Three legs A B A over both kernels (VALU, matrix cores, VALU); per leg join_overlaps
and isccsearch_join_within on the same table and tau -- the same scan, so their difference is the price of the emit form plus the
aggregation -- each one warm-up call and the median of --reps.  For tables of up to --search-rows rows also the only way there was
before: one HipSimprintIndex.search_raw per asset (limit 100, the threshold that gives the same radius), timed once.

--overlaps-between: isccsearch_join_overlaps_between (the cross join's OVERLAP form and the same aggregation) on TWO simprint tables of
equal size: the generator of --overlaps split over two tables -- 64-bit and 128-bit simprints, about 16 chunks per asset in random row
order, disjoint asset keys, --shared per cent of A's assets containing a run of 4-8 chunks of an asset of B (0-2 bits flipped).  Three
legs A B A over both kernels; per leg join_overlaps_between and, on the same two tables and tau, isccsearch_join_between -- the same
scan --, each one warm-up call and the median of --reps.

--segments: isccsearch_join_segments (join_overlaps plus the run detection of csrc/segments.hip, from one join launch) against
isccsearch_join_overlaps on the tables of --overlaps, whose planted runs of 4-8 chunks are the segments to find.  On either kernel three
legs A B A (join_overlaps, join_segments, join_overlaps), each one warm-up call and the median of --reps; the tool asserts that both
calls agree on chunk pairs and records and that the segments' lengths add up to the chunk pairs.

--segments-between: isccsearch_join_segments_between (join_overlaps_between plus the two-table run detection of csrc/segments.hip, from
one join launch) against isccsearch_join_overlaps_between on the two tables of --overlaps-between, whose planted runs of 4-8 chunks are
the segments to find.  On either kernel three legs A B A (join_overlaps_between, join_segments_between, join_overlaps_between), each one
warm-up call and the median of --reps; the tool asserts that both calls agree on chunk pairs and records and that the segments' lengths
add up to the chunk pairs.  Its output is what profiles/join_segments_between_rate.txt records.

--degrees: isccsearch_join_degrees (the joins' DEGREE form: a count per row, no pairs) against isccsearch_join_within and
isccsearch_join_components of the SAME build and run, on 64-bit HAMMING and 256-bit NPHD tables of host-generated rows (keys 1..n).
(a) uniform random rows: per kernel five legs A B C B A (join_within, join_components, join_degrees, join_components, join_within), each
one warm-up call and the median of --reps; `degrees_to_components` = join_degrees / mean of the two join_components legs -- they share
the scan.  (b) the same rows with the code of row 0 planted in --hub rows (default 10 000: 5 * 10^7 pairs, over join_within's default
max_pairs): legs B C B; the tool asserts that the calls agree on the links and that exactly the hub's rows have degree >= hub - 1.
--baseline DIR: a built checkout of another commit (the parent).  Before anything else the existing modes (the pair join, --components,
--overlaps) run from DIR, from this tree and from DIR again, every run a process of its own, their lines printed under the tree's name:
this tree's join_within, join_components and join_overlaps between two runs of the baseline.  Its output is what
profiles/join_degrees_rate.txt records.

usage: python tools/bench_duplicates.py [--mfma both] [--reps 5] [--sizes 65536,262144,1048576,4194304] [--nphd-sizes 262144,1048576] [--tau 6]
       python tools/bench_duplicates.py --between [--rows-a N --rows-b M] [the same options]
       python tools/bench_duplicates.py --components [--sizes 1048576 --nphd-sizes 1048576] [--dense-rows 1048576 --cluster 1000]
       python tools/bench_duplicates.py --overlaps [--sizes 65536,262144,1048576] [--shared 3] [--search-rows 65536]
       python tools/bench_duplicates.py --overlaps-between [--sizes 65536,262144,1048576] [--shared 3]
       python tools/bench_duplicates.py --segments [--sizes 65536,1048576] [--shared 3]
       python tools/bench_duplicates.py --segments-between [--sizes 65536,262144,1048576] [--shared 3]
       python tools/bench_duplicates.py --degrees [--sizes 65536,1048576 --nphd-sizes 65536,1048576] [--hub 10000] [--baseline DIR]
"""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from iscc_search_amd import _lib  # noqa: E402
from iscc_search_amd.engine import HipEngine  # noqa: E402

SIMDS, CLOCK_HZ = 1024, 2.4e9     # 256 CUs x 4 SIMDs, max clock (as bench.py)


def valu_peak_pairs(words):
    return SIMDS * CLOCK_HZ * 64 / ((4.0 * words + 0.5) * 4.0)


def table_name(metric, nbytes):
    return f"{'HAMMING' if metric == _lib.METRIC_HAMMING else 'NPHD'} {8 * nbytes}-bit"


def median_of(join, reps, found=lambda out: len(out[2])):
    """(seconds, pairs found): median of `reps` calls after one warm-up (code objects, buffers)."""
    join()
    times, pairs_found = [], 0
    for _ in range(reps):
        t0 = time.perf_counter()
        out = join()                                    # ends in a device synchronise (the pair count is read back)
        times.append(time.perf_counter() - t0)
        pairs_found = found(out)
    return statistics.median(times), pairs_found


def leg(engine, mfma, join, reps, found=lambda out: len(out[2]), launches_expected=True):
    """One leg on one kernel; the statistics must say that kernel ran, and no other."""
    opts = dict(mfma=1, join_mfma=1, join_mfma_min_rows=0) if mfma else dict(join_mfma=0)
    before = engine.stats()
    with engine.options(**opts):
        seconds, pairs_found = median_of(join, reps, found)
    after = engine.stats()
    launches = after["join_launches"] - before["join_launches"]
    on_mfma = after["join_mfma_launches"] - before["join_mfma_launches"]
    assert (launches > 0) == launches_expected and on_mfma == (launches if mfma else 0), (mfma, launches, on_mfma)
    return seconds, pairs_found


def measure(engine, which, join, pairs, words, reps):
    """The legs `which` asks for over one join: {seconds, rates, ratio, pairs_found}."""
    out = {}
    if which != "both":
        seconds, found = leg(engine, which == "1", join, reps)
        out.update(kernel="mfma" if which == "1" else "valu", seconds=round(seconds, 5), pair_distances_per_s=float(f"{pairs / seconds:.4g}"), pairs_found=found)
        if which == "0":
            out["valu_issue_fraction"] = round(pairs / seconds / valu_peak_pairs(words), 3)
        return out
    a1, f1 = leg(engine, False, join, reps)
    b, fb = leg(engine, True, join, reps)
    a2, f2 = leg(engine, False, join, reps)
    assert f1 == fb == f2, f"the kernels disagree on the number of pairs: VALU {f1}, matrix cores {fb}, VALU {f2}"
    rates = [pairs / s for s in (a1, b, a2)]
    out.update(valu_seconds=[round(a1, 5), round(a2, 5)], mfma_seconds=round(b, 5),
               valu_pair_distances_per_s=[float(f"{rates[0]:.4g}"), float(f"{rates[2]:.4g}")], mfma_pair_distances_per_s=float(f"{rates[1]:.4g}"),
               ratio=round(rates[1] / ((rates[0] + rates[2]) / 2), 3), pairs_found=fb,
               valu_issue_fraction=round((rates[0] + rates[2]) / 2 / valu_peak_pairs(words), 3))
    return out


def run(engine, which, metric, nbytes, n, tau, reps):
    t = engine.open_table(metric, 1, nbytes)
    try:
        t.add_synthetic(nbytes, n, seed=1234 + n, first_row=0, key_base=1)
        mh = np.full(_lib.MAX_BYTES + 1, -1, dtype=np.int16)
        mh[nbytes] = tau
        out = {"join": "within", "table": table_name(metric, nbytes), "rows": n, "tau": tau}
        out.update(measure(engine, which, lambda: t.join_within(mh, 1 << 20), n * (n - 1) / 2, (nbytes + 7) // 8, reps))
        return out
    finally:
        t.drop()


def run_between(engine, which, metric, nbytes, n_a, n_b, tau, reps):
    """The cross join of two tables of different random rows."""
    ta, tb = engine.open_table(metric, 1, nbytes), engine.open_table(metric, 1, nbytes)
    try:
        ta.add_synthetic(nbytes, n_a, seed=1234 + n_a, first_row=0, key_base=1)
        tb.add_synthetic(nbytes, n_b, seed=4321 + n_b, first_row=0, key_base=1)
        mh = np.full(_lib.MAX_BYTES + 1, -1, dtype=np.int16)
        mh[nbytes] = tau
        out = {"join": "between", "table": table_name(metric, nbytes), "rows_a": n_a, "rows_b": n_b, "tau": tau}
        out.update(measure(engine, which, lambda: ta.join_between(tb, mh, 1 << 20), float(n_a) * n_b, (nbytes + 7) // 8, reps))
        return out
    finally:
        ta.drop()
        tb.drop()


def components_call(t, mh, n):
    """join_components over all rows of a table whose keys are 1..n (label = row of add_synthetic), from the identity each time."""
    live_keys = np.arange(1, n + 1, dtype=np.uint64)
    live_labels = np.arange(n, dtype=np.uint32)
    start, parent = live_labels.copy(), live_labels.copy()

    def call():
        np.copyto(parent, start)
        return t.join_components(mh, live_keys, live_labels, parent), parent
    return call


def run_components(engine, metric, nbytes, n, tau, reps):
    """join_components against join_within on one synthetic table: A B A per kernel."""
    t = engine.open_table(metric, 1, nbytes)
    try:
        t.add_synthetic(nbytes, n, seed=1234 + n, first_row=0, key_base=1)
        mh = np.full(_lib.MAX_BYTES + 1, -1, dtype=np.int16)
        mh[nbytes] = tau
        within = lambda: t.join_within(mh, 1 << 20)                   # noqa: E731
        components = components_call(t, mh, n)
        around = components_call(t, np.full(_lib.MAX_BYTES + 1, -1, dtype=np.int16), n)
        out = {"join": "components", "table": table_name(metric, nbytes), "rows": n, "tau": tau}
        for mfma in (False, True):
            a1, f1 = leg(engine, mfma, within, reps)
            b, links = leg(engine, mfma, components, reps, found=lambda o: o[0])
            a2, f2 = leg(engine, mfma, within, reps)
            assert f1 == links == f2, f"join_within found {f1} and {f2} pairs, join_components {links} links"
            extra, _ = leg(engine, mfma, around, reps, found=lambda o: o[0], launches_expected=False)
            out["mfma" if mfma else "valu"] = dict(within_seconds=[round(a1, 5), round(a2, 5)], components_seconds=round(b, 5),
                                                   ratio=round(b / ((a1 + a2) / 2), 4), around_the_joins_seconds=round(extra, 5), links=links)
        return out
    finally:
        t.drop()


def run_dense(engine, n, cluster, reps):
    """64-bit rows in clusters of `cluster` identical rows, stored in random order: every pair of a cluster is a link at tau 0."""
    rng = np.random.default_rng(99)
    t = engine.open_table(_lib.METRIC_HAMMING, 1, 8)
    try:
        codes = rng.integers(0, 2**64, size=(n + cluster - 1) // cluster, dtype=np.uint64)
        words = np.repeat(codes, cluster)[:n][rng.permutation(n)]
        t.add(np.arange(1, n + 1, dtype=np.uint64), words[:, None])
        mh = np.full(_lib.MAX_BYTES + 1, -1, dtype=np.int16)
        mh[8] = 0
        call = components_call(t, mh, n)
        sizes = np.unique(words, return_counts=True)[1].astype(np.int64)
        expected = int((sizes * (sizes - 1) // 2).sum())
        out = {"join": "components, dense", "table": table_name(_lib.METRIC_HAMMING, 8), "rows": n, "cluster": cluster, "tau": 0}
        for mfma in (False, True):
            seconds, links = leg(engine, mfma, call, reps, found=lambda o: o[0])
            groups = len(np.unique(call()[1]))
            assert links == expected and groups == len(sizes), (links, expected, groups, len(sizes))
            out["mfma" if mfma else "valu"] = dict(seconds=round(seconds, 5), links=links, ns_per_link=round(seconds / links * 1e9, 4), groups=groups)
        return out
    finally:
        t.drop()


def degrees_call(t, mh, n):
    """join_degrees over all rows of a table whose keys are 1..n"""
    live_keys = np.arange(1, n + 1, dtype=np.uint64)
    return lambda: t.join_degrees(mh, live_keys)


def run_degrees(engine, metric, nbytes, n, tau, reps, hub):
    """join_degrees against join_within and join_components: (a) random rows, A B C B A per kernel; (b) with a hub planted, B C B."""
    rng = np.random.default_rng(1234 + n + nbytes)
    W = nbytes // 8
    words = rng.integers(0, 2**64, size=(n, W), dtype=np.uint64)
    keys = np.arange(1, n + 1, dtype=np.uint64)
    mh = np.full(_lib.MAX_BYTES + 1, -1, dtype=np.int16)
    mh[nbytes] = tau
    nb = None if metric == _lib.METRIC_HAMMING else np.full(n, nbytes, dtype=np.uint8)
    lines = []
    for planted in (0, hub):
        if planted:
            words[rng.choice(np.arange(1, n), size=planted - 1, replace=False)] = words[0]
        t = engine.open_table(metric, 1, nbytes)
        try:
            for lo in range(0, n, 1 << 18):
                t.add(keys[lo:lo + (1 << 18)], words[lo:lo + (1 << 18)], None if nb is None else nb[lo:lo + (1 << 18)])
            within = lambda: t.join_within(mh, 1 << 20)                   # noqa: E731
            components, degrees = components_call(t, mh, n), degrees_call(t, mh, n)
            out = {"join": "degrees", "rows_are": f"random, one code in {planted} rows" if planted else "random", "table": table_name(metric, nbytes),
                   "rows": n, "tau": tau}
            for mfma in (False, True):
                a1, f1 = leg(engine, mfma, within, reps) if not planted else (None, None)
                b1, links_1 = leg(engine, mfma, components, reps, found=lambda o: o[0])
                c, (degree, links) = leg(engine, mfma, degrees, reps, found=lambda o: o)
                b2, links_2 = leg(engine, mfma, components, reps, found=lambda o: o[0])
                a2, f2 = leg(engine, mfma, within, reps) if not planted else (None, None)
                assert links_1 == links == links_2 and int(degree.sum(dtype=np.uint64)) == 2 * links, (links_1, links, links_2)
                res = dict(components_seconds=[round(b1, 5), round(b2, 5)], degrees_seconds=round(c, 5),
                           degrees_to_components=round(c / ((b1 + b2) / 2), 4), links=links, largest_degree=int(degree.max()))
                if planted:
                    # (the few pairs random rows have among themselves may have lost a row to the hub, or gained the hub's)
                    assert links >= planted * (planted - 1) // 2 and int((degree >= planted - 1).sum()) == planted, (links, planted)
                else:
                    assert f1 == links == f2, f"join_within found {f1} and {f2} pairs, join_degrees {links} links"
                    res.update(within_seconds=[round(a1, 5), round(a2, 5)], degrees_to_within=round(c / ((a1 + a2) / 2), 4))
                out["mfma" if mfma else "valu"] = res
            lines.append(out)
        finally:
            t.drop()
    return lines


def existing_modes(tree, name, sizes, nphd_sizes, reps, tau):
    """The pair join, --components and --overlaps of the tool of ``tree`` (this one, or a built checkout of another commit), each in a
    process of its own with that tree's package and library; their lines, printed under ``name``."""
    env = {k: v for k, v in os.environ.items() if k != "ISCC_HIP_LIB"}
    common = ["--sizes", sizes, "--reps", str(reps), "--tau", str(tau)]
    for mode in (["--nphd-sizes", nphd_sizes], ["--components", "--dense-rows", "0", "--nphd-sizes", nphd_sizes], ["--overlaps", "--search-rows", "0"]):
        cmd = [sys.executable, os.path.join(tree, "tools", "bench_duplicates.py"), *mode, *common]
        done = subprocess.run(cmd, capture_output=True, text=True, cwd=tree, env=env)
        if done.returncode != 0:
            raise RuntimeError(f"{' '.join(cmd)} failed:\n{done.stdout}\n{done.stderr}")
        for line in done.stdout.splitlines():
            if line.startswith("{"):
                print(json.dumps({"tree": name, **json.loads(line)}), flush=True)


def simprint_rows(rng, n, nbytes, per_asset, shared_pct):
    """(keys [n, 2], words [n, W], asset keys): n chunks dealt to assets of `per_asset`, some assets containing runs of another's."""
    W = nbytes // 8
    words = rng.integers(0, 2**64, size=(n, W), dtype=np.uint64)
    n_assets = max(2, n // per_asset)
    asset_of = (np.arange(n) // per_asset).clip(max=n_assets - 1)
    for a in rng.choice(n_assets, size=max(1, n_assets * shared_pct // 100), replace=False).tolist():
        b = int(rng.integers(0, n_assets - 1))
        b += b >= a
        run = int(rng.integers(4, 9))
        dst, src = a * per_asset, b * per_asset + int(rng.integers(0, per_asset - run + 1))
        words[dst:dst + run] = words[src:src + run]
        for _ in range(2):
            words[dst:dst + run, 0] ^= np.left_shift(np.uint64(1), rng.integers(0, 64, size=run).astype(np.uint64)) * (rng.random(run) < 0.5)
    asset_keys = np.arange(1, n_assets + 1, dtype=np.uint64) * np.uint64(1000003)
    keys = np.stack([asset_keys[asset_of], (np.arange(n, dtype=np.uint64) << np.uint64(32)) | np.uint64(1)], axis=1)       # offset: the chunk's number
    order = rng.permutation(n)
    return keys[order], words[order], asset_keys


def run_overlaps(engine, nbytes, n, tau, reps, shared_pct, search_rows):
    """join_overlaps and join_within on one simprint table, A B A over both kernels; the search_raw loop for small tables."""
    from iscc_search_amd.simprint import HipSimprintIndex

    rng = np.random.default_rng(4242 + n + nbytes)
    keys, words, asset_keys = simprint_rows(rng, n, nbytes, 16, shared_pct)
    index = HipSimprintIndex(engine, ndim=8 * nbytes)
    t = index._index._table
    try:
        for lo in range(0, n, 1 << 18):
            t.add(keys[lo:lo + (1 << 18)], words[lo:lo + (1 << 18)], None, trusted_unique=True)
        mh = np.full(_lib.MAX_BYTES + 1, -1, dtype=np.int16)
        mh[nbytes] = tau
        overlaps = lambda: t.join_overlaps(tau, asset_keys, 0, 1 << 22)      # noqa: E731
        within = lambda: t.join_within(mh, 1 << 22)                          # noqa: E731
        out = {"join": "overlaps", "table": f"simprints {8 * nbytes}-bit", "rows": n, "assets": len(asset_keys), "tau": tau, "legs": []}
        for mfma in (False, True, False):
            o_s, info = leg(engine, mfma, overlaps, reps, found=lambda o: o[2])
            w_s, pairs = leg(engine, mfma, within, reps)
            out["legs"].append(dict(kernel="mfma" if mfma else "valu", overlaps_seconds=round(o_s, 5), within_seconds=round(w_s, 5),
                                    overlaps_minus_within_seconds=round(o_s - w_s, 5), chunk_pairs=info["chunk_pairs"], records=info["records"],
                                    within_row_pairs=pairs))
        assert len({(l["chunk_pairs"], l["records"]) for l in out["legs"]}) == 1, "the legs disagree"
        if n <= search_rows:
            # the only way before: one search per asset by its own simprints, the other assets read off every result list
            by_asset = {}
            raw = np.ascontiguousarray(words).astype(">u8").tobytes()
            for i, key in enumerate(keys[:, 0].tolist()):
                by_asset.setdefault(key, []).append(raw[i * nbytes:(i + 1) * nbytes])
            threshold = 1.0 - tau / (8.0 * nbytes)
            t0 = time.perf_counter()
            listed = 0
            for key, simprints in by_asset.items():
                listed += len(index.search_raw(simprints, limit=100, threshold=threshold, total_assets=len(by_asset))) - 1
            out["search_raw_loop"] = dict(seconds=round(time.perf_counter() - t0, 3), searches=len(by_asset), assets_listed=listed)
        return out
    finally:
        index.close()


def run_segments(engine, nbytes, n, tau, reps, shared_pct):
    """join_overlaps, join_segments, join_overlaps (A B A) on one simprint table, on either kernel."""
    from iscc_search_amd.simprint import HipSimprintIndex

    rng = np.random.default_rng(4242 + n + nbytes)
    keys, words, asset_keys = simprint_rows(rng, n, nbytes, 16, shared_pct)
    index = HipSimprintIndex(engine, ndim=8 * nbytes)
    t = index._index._table
    try:
        for lo in range(0, n, 1 << 18):
            t.add(keys[lo:lo + (1 << 18)], words[lo:lo + (1 << 18)], None, trusted_unique=True)
        overlaps = lambda: t.join_overlaps(tau, asset_keys, 0, 1 << 22)      # noqa: E731
        segments = lambda: t.join_segments(tau, asset_keys, 0, 1 << 22)      # noqa: E731
        out = {"join": "segments", "table": f"simprints {8 * nbytes}-bit", "rows": n, "assets": len(asset_keys), "tau": tau, "kernels": []}
        for mfma in (False, True):
            a1, info_a = leg(engine, mfma, overlaps, reps, found=lambda o: o[2])
            b, info_b = leg(engine, mfma, segments, reps, found=lambda o: (o[2], int(o[3]["length"].sum()), int(o[3]["length"].max()) if len(o[3]) else 0))
            a2, _ = leg(engine, mfma, overlaps, reps, found=lambda o: o[2])
            info_b, in_runs, longest = info_b
            assert {k: info_b[k] for k in info_a} == info_a and in_runs == info_b["chunk_pairs"], "join_segments disagrees with join_overlaps"
            out["kernels"].append(dict(kernel="mfma" if mfma else "valu", overlaps_seconds=[round(a1, 5), round(a2, 5)], segments_seconds=round(b, 5),
                                       segments_minus_overlaps_seconds=round(b - (a1 + a2) / 2, 5), chunk_pairs=info_b["chunk_pairs"],
                                       records=info_b["records"], segments=info_b["segments"], longest_run=longest))
        return out
    finally:
        index.close()


def simprint_two_tables(rng, n, nbytes, per_asset, shared_pct):
    """Two tables of n chunks each, (keys, words, asset keys) per side: ``simprint_rows`` with every run copied from B into A."""
    W = nbytes // 8
    n_assets = max(2, n // per_asset)
    asset_of = (np.arange(n) // per_asset).clip(max=n_assets - 1)
    words_a, words_b = (rng.integers(0, 2**64, size=(n, W), dtype=np.uint64) for _ in range(2))
    for a in rng.choice(n_assets, size=max(1, n_assets * shared_pct // 100), replace=False).tolist():
        b = int(rng.integers(0, n_assets))
        run = int(rng.integers(4, 9))
        dst, src = a * per_asset, b * per_asset + int(rng.integers(0, per_asset - run + 1))
        words_a[dst:dst + run] = words_b[src:src + run]
        for _ in range(2):
            words_a[dst:dst + run, 0] ^= np.left_shift(np.uint64(1), rng.integers(0, 64, size=run).astype(np.uint64)) * (rng.random(run) < 0.5)
    sides = []
    for first, words in ((1, words_a), (n_assets + 1, words_b)):
        asset_keys = np.arange(first, first + n_assets, dtype=np.uint64) * np.uint64(1000003)
        keys = np.stack([asset_keys[asset_of], (np.arange(n, dtype=np.uint64) << np.uint64(32)) | np.uint64(1)], axis=1)
        order = rng.permutation(n)
        sides.append((keys[order], words[order], asset_keys))
    return sides


def run_overlaps_between(engine, nbytes, n, tau, reps, shared_pct):
    """join_overlaps_between and join_between on two simprint tables of n rows each, A B A over both kernels."""
    rng = np.random.default_rng(2424 + n + nbytes)
    (keys_a, words_a, assets_a), (keys_b, words_b, assets_b) = simprint_two_tables(rng, n, nbytes, 16, shared_pct)
    ta, tb = engine.open_table(_lib.METRIC_HAMMING, 2, nbytes), engine.open_table(_lib.METRIC_HAMMING, 2, nbytes)
    try:
        for t, keys, words in ((ta, keys_a, words_a), (tb, keys_b, words_b)):
            for lo in range(0, n, 1 << 18):
                t.add(keys[lo:lo + (1 << 18)], words[lo:lo + (1 << 18)], None, trusted_unique=True)
        mh = np.full(_lib.MAX_BYTES + 1, -1, dtype=np.int16)
        mh[nbytes] = tau
        overlaps = lambda: ta.join_overlaps_between(tb, tau, assets_a, assets_b, 0, 1 << 22)      # noqa: E731
        between = lambda: ta.join_between(tb, mh, 1 << 22)                                        # noqa: E731
        out = {"join": "overlaps_between", "table": f"simprints {8 * nbytes}-bit", "rows_a": n, "rows_b": n, "assets_a": len(assets_a),
               "assets_b": len(assets_b), "tau": tau, "legs": []}
        for mfma in (False, True, False):
            o_s, info = leg(engine, mfma, overlaps, reps, found=lambda o: o[3])
            b_s, pairs = leg(engine, mfma, between, reps)
            out["legs"].append(dict(kernel="mfma" if mfma else "valu", overlaps_between_seconds=round(o_s, 5), between_seconds=round(b_s, 5),
                                    overlaps_between_minus_between_seconds=round(o_s - b_s, 5), chunk_pairs=info["chunk_pairs"],
                                    records=info["records"], between_row_pairs=pairs))
        assert len({(l["chunk_pairs"], l["records"], l["between_row_pairs"]) for l in out["legs"]}) == 1, "the legs disagree"
        return out
    finally:
        ta.drop()
        tb.drop()


def run_segments_between(engine, nbytes, n, tau, reps, shared_pct):
    """join_overlaps_between, join_segments_between, join_overlaps_between (A B A) on two simprint tables of n rows each, on either kernel."""
    rng = np.random.default_rng(2424 + n + nbytes)
    (keys_a, words_a, assets_a), (keys_b, words_b, assets_b) = simprint_two_tables(rng, n, nbytes, 16, shared_pct)
    ta, tb = engine.open_table(_lib.METRIC_HAMMING, 2, nbytes), engine.open_table(_lib.METRIC_HAMMING, 2, nbytes)
    try:
        for t, keys, words in ((ta, keys_a, words_a), (tb, keys_b, words_b)):
            for lo in range(0, n, 1 << 18):
                t.add(keys[lo:lo + (1 << 18)], words[lo:lo + (1 << 18)], None, trusted_unique=True)
        overlaps = lambda: ta.join_overlaps_between(tb, tau, assets_a, assets_b, 0, 1 << 22)      # noqa: E731
        segments = lambda: ta.join_segments_between(tb, tau, assets_a, assets_b, 0, 1 << 22)      # noqa: E731
        out = {"join": "segments_between", "table": f"simprints {8 * nbytes}-bit", "rows_a": n, "rows_b": n, "assets_a": len(assets_a),
               "assets_b": len(assets_b), "tau": tau, "kernels": []}
        for mfma in (False, True):
            a1, info_a = leg(engine, mfma, overlaps, reps, found=lambda o: o[3])
            b, info_b = leg(engine, mfma, segments, reps, found=lambda o: (o[3], int(o[4]["length"].sum()), int(o[4]["length"].max()) if len(o[4]) else 0))
            a2, _ = leg(engine, mfma, overlaps, reps, found=lambda o: o[3])
            info_b, in_runs, longest = info_b
            assert {k: info_b[k] for k in info_a} == info_a and in_runs == info_b["chunk_pairs"], "join_segments_between disagrees with join_overlaps_between"
            out["kernels"].append(dict(kernel="mfma" if mfma else "valu", overlaps_between_seconds=[round(a1, 5), round(a2, 5)],
                                       segments_between_seconds=round(b, 5), segments_minus_overlaps_seconds=round(b - (a1 + a2) / 2, 5),
                                       chunk_pairs=info_b["chunk_pairs"], records=info_b["records"], segments=info_b["segments"], longest_run=longest))
        return out
    finally:
        ta.drop()
        tb.drop()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mfma", choices=("0", "1", "both"), default="both", help="the kernel: XOR + popcount, matrix cores, or A B A over both")
    ap.add_argument("--reps", type=int, default=5, help="timed calls per leg (their median counts)")
    ap.add_argument("--sizes", default="65536,262144,1048576,4194304", help="row counts of the 64-bit HAMMING tables")
    ap.add_argument("--nphd-sizes", default="262144,1048576", help="row counts of the 256-bit NPHD tables (empty: none)")
    ap.add_argument("--tau", type=int, default=6, help="max Hamming distance of the 64-bit tables (4x that for 256 bits)")
    ap.add_argument("--between", action="store_true", help="the cross join of two tables of each size instead of the self-join")
    ap.add_argument("--rows-a", type=int, default=0, help="--between: rows of table A (with --rows-b: this one pair of sizes only)")
    ap.add_argument("--rows-b", type=int, default=0, help="--between: rows of table B")
    ap.add_argument("--components", action="store_true", help="join_components against join_within (A B A per kernel), then the dense table")
    ap.add_argument("--dense-rows", type=int, default=1 << 20, help="--components: rows of the dense table (0: skip it)")
    ap.add_argument("--cluster", type=int, default=1000, help="--components: identical rows per cluster of the dense table")
    ap.add_argument("--overlaps", action="store_true", help="join_overlaps against join_within on simprint tables (A B A over both kernels)")
    ap.add_argument("--overlaps-between", action="store_true", help="join_overlaps_between against join_between on two simprint tables (A B A over both kernels)")
    ap.add_argument("--segments", action="store_true", help="join_segments against join_overlaps on simprint tables (A B A on either kernel)")
    ap.add_argument("--segments-between", action="store_true",
                    help="join_segments_between against join_overlaps_between on two simprint tables (A B A on either kernel)")
    ap.add_argument("--degrees", action="store_true", help="join_degrees against join_within and join_components (A B C B A per kernel), random rows and a planted hub")
    ap.add_argument("--hub", type=int, default=10_000, help="--degrees: rows that hold the planted code")
    ap.add_argument("--baseline", default="", help="--degrees: a built checkout of another commit whose existing modes run before and after this tree's")
    ap.add_argument("--shared", type=int, default=3, help="--overlaps, --overlaps-between, --segments, --segments-between: per cent of the assets that contain a run of another asset's chunks")
    ap.add_argument("--search-rows", type=int, default=65536, help="--overlaps: tables of up to this many rows also time one search_raw per asset")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",") if s]
    nphd_sizes = [int(s) for s in a.nphd_sizes.split(",") if s]
    if a.degrees and a.baseline:                     # (before this process opens the device: one process on the card at a time)
        for tree, name in ((a.baseline, "baseline"), (ROOT, "this"), (a.baseline, "baseline")):
            existing_modes(os.path.abspath(tree), name, a.sizes, a.nphd_sizes, a.reps, a.tau)
    engine = HipEngine(a.device)
    try:
        if a.degrees:
            for metric, nbytes, table_sizes in ((_lib.METRIC_HAMMING, 8, sizes), (_lib.METRIC_NPHD, 32, nphd_sizes)):
                for n in table_sizes:
                    for line in run_degrees(engine, metric, nbytes, n, a.tau * nbytes // 8, a.reps, min(a.hub, n // 2)):
                        print(json.dumps(line), flush=True)
            return
        if a.segments_between:
            for nbytes in (8, 16):
                for n in sizes:
                    print(json.dumps(run_segments_between(engine, nbytes, n, a.tau * nbytes // 8, a.reps, a.shared)), flush=True)
            return
        if a.overlaps_between:
            for nbytes in (8, 16):
                for n in sizes:
                    print(json.dumps(run_overlaps_between(engine, nbytes, n, a.tau * nbytes // 8, a.reps, a.shared)), flush=True)
            return
        if a.segments:
            for nbytes in (8, 16):
                for n in sizes:
                    print(json.dumps(run_segments(engine, nbytes, n, a.tau * nbytes // 8, a.reps, a.shared)), flush=True)
            return
        if a.overlaps:
            for nbytes in (8, 16):
                for n in sizes:
                    print(json.dumps(run_overlaps(engine, nbytes, n, a.tau * nbytes // 8, a.reps, a.shared, a.search_rows)), flush=True)
            return
        if a.components:
            for n in sizes:
                print(json.dumps(run_components(engine, _lib.METRIC_HAMMING, 8, n, a.tau, a.reps)), flush=True)
            for n in nphd_sizes:
                print(json.dumps(run_components(engine, _lib.METRIC_NPHD, 32, n, 4 * a.tau, a.reps)), flush=True)
            if a.dense_rows:
                print(json.dumps(run_dense(engine, a.dense_rows, a.cluster, a.reps)), flush=True)
            return
        if a.between:
            given = a.rows_a > 0 and a.rows_b > 0
            for n_a, n_b in [(a.rows_a, a.rows_b)] if given else [(n, n) for n in sizes]:
                print(json.dumps(run_between(engine, a.mfma, _lib.METRIC_HAMMING, 8, n_a, n_b, a.tau, a.reps)), flush=True)
            for n_a, n_b in [(a.rows_a, a.rows_b)] if given else [(n, n) for n in nphd_sizes]:
                print(json.dumps(run_between(engine, a.mfma, _lib.METRIC_NPHD, 32, n_a, n_b, 4 * a.tau, a.reps)), flush=True)
            return
        for n in sizes:
            print(json.dumps(run(engine, a.mfma, _lib.METRIC_HAMMING, 8, n, a.tau, a.reps)), flush=True)
        for n in nphd_sizes:
            print(json.dumps(run(engine, a.mfma, _lib.METRIC_NPHD, 32, n, 4 * a.tau, a.reps)), flush=True)
    finally:
        engine.close()


if __name__ == "__main__":
    main()
