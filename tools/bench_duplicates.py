#!/usr/bin/env python3
"""
Rate of the device joins (isccsearch_join_within and isccsearch_join_between, csrc/join.hip.h) on synthetic tables.

Tables: 64-bit HAMMING rows at 1 M and 10 M rows, and a 256-bit NPHD table (all rows 32 bytes).  Synthetic rows are random
words (isccsearch_add_synthetic), so almost no pair is within the threshold and the time is that of the scan: n(n-1)/2 pair
distances.  Prints one line per table: seconds (best of --reps after one warm-up), pair distances per second, and the
fraction of the VALU issue rate -- 64 lanes / ((4 W + 0.5) instructions x 4 cycles) per SIMD and clock, the figure bench.py
uses for the XOR + popcount scan (W = 64-bit words per row).

--between: the cross join of two synthetic tables of --rows-a and --rows-b rows (rows_a x rows_b pair distances), for 64-bit
HAMMING and 256-bit NPHD rows, each next to the self-join of the --rows-a table: one line per width with both rates and
their ratio.

usage: python tools/bench_duplicates.py [--reps 3] [--sizes 1000000,10000000] [--nphd-rows 1000000] [--tau 6]
       python tools/bench_duplicates.py --between [--rows-a 1000000] [--rows-b 1000000] [--reps 3] [--tau 6]
"""

import argparse
import json
import os
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


def best_of(join, reps):
    """(seconds, pairs found): best of `reps` calls after one warm-up (code objects, buffers)."""
    join()
    best, pairs_found = None, 0
    for _ in range(reps):
        t0 = time.perf_counter()
        out = join()                                    # ends in a device synchronise (the pair count is read back)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
        pairs_found = len(out[2])
    return best, pairs_found


def run(engine, metric, nbytes, n, tau, reps):
    t = engine.open_table(metric, 1, nbytes)
    try:
        t.add_synthetic(nbytes, n, seed=1234 + n, first_row=0, key_base=1)
        mh = np.full(_lib.MAX_BYTES + 1, -1, dtype=np.int16)
        mh[nbytes] = tau
        best, pairs_found = best_of(lambda: t.join_within(mh, 1 << 20), reps)
        words = (nbytes + 7) // 8
        pairs = n * (n - 1) / 2
        rate = pairs / best
        return {"table": table_name(metric, nbytes), "rows": n, "tau": tau,
                "seconds": round(best, 5), "pair_distances_per_s": float(f"{rate:.4g}"), "pairs_found": pairs_found,
                "valu_issue_fraction": round(rate / valu_peak_pairs(words), 3)}
    finally:
        t.drop()


def run_between(engine, metric, nbytes, n_a, n_b, tau, reps):
    """The cross join of two tables of different random rows, and the self-join of the first for comparison."""
    ta, tb = engine.open_table(metric, 1, nbytes), engine.open_table(metric, 1, nbytes)
    try:
        ta.add_synthetic(nbytes, n_a, seed=1234 + n_a, first_row=0, key_base=1)
        tb.add_synthetic(nbytes, n_b, seed=4321 + n_b, first_row=0, key_base=1)
        mh = np.full(_lib.MAX_BYTES + 1, -1, dtype=np.int16)
        mh[nbytes] = tau
        within_s, _ = best_of(lambda: ta.join_within(mh, 1 << 20), reps)
        between_s, pairs_found = best_of(lambda: ta.join_between(tb, mh, 1 << 20), reps)
        within_rate = n_a * (n_a - 1) / 2 / within_s
        between_rate = n_a * n_b / between_s
        return {"table": table_name(metric, nbytes), "rows_a": n_a, "rows_b": n_b, "tau": tau,
                "between_seconds": round(between_s, 5), "between_pair_distances_per_s": float(f"{between_rate:.4g}"),
                "within_seconds": round(within_s, 5), "within_pair_distances_per_s": float(f"{within_rate:.4g}"),
                "between_over_within": round(between_rate / within_rate, 3), "pairs_found": pairs_found,
                "valu_issue_fraction": round(between_rate / valu_peak_pairs((nbytes + 7) // 8), 3)}
    finally:
        ta.drop()
        tb.drop()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="1000000,10000000", help="row counts of the 64-bit tables")
    ap.add_argument("--nphd-rows", type=int, default=1_000_000, help="rows of the 256-bit NPHD table (0: skip)")
    ap.add_argument("--tau", type=int, default=6, help="max Hamming distance of the 64-bit tables (4x that for 256 bits)")
    ap.add_argument("--between", action="store_true", help="the cross join of two tables next to the self-join's rate")
    ap.add_argument("--rows-a", type=int, default=1_000_000, help="--between: rows of table A")
    ap.add_argument("--rows-b", type=int, default=1_000_000, help="--between: rows of table B")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    engine = HipEngine(a.device)
    try:
        if a.between:
            print(json.dumps(run_between(engine, _lib.METRIC_HAMMING, 8, a.rows_a, a.rows_b, a.tau, a.reps)), flush=True)
            print(json.dumps(run_between(engine, _lib.METRIC_NPHD, 32, a.rows_a, a.rows_b, 4 * a.tau, a.reps)), flush=True)
            return
        for n in [int(s) for s in a.sizes.split(",") if s]:
            print(json.dumps(run(engine, _lib.METRIC_HAMMING, 8, n, a.tau, a.reps)), flush=True)
        if a.nphd_rows:
            print(json.dumps(run(engine, _lib.METRIC_NPHD, 32, a.nphd_rows, 4 * a.tau, a.reps)), flush=True)
    finally:
        engine.close()


if __name__ == "__main__":
    main()
