#!/usr/bin/env python3
"""
Rate of the device self-join (isccsearch_join_within, csrc/join.hip.h) on synthetic tables.

Tables: 64-bit HAMMING rows at 1 M and 10 M rows, and a 256-bit NPHD table (all rows 32 bytes).  Synthetic rows are random
words (isccsearch_add_synthetic), so almost no pair is within the threshold and the time is that of the scan: n(n-1)/2 pair
distances.  Prints one line per table: seconds (best of --reps after one warm-up), pair distances per second, and the
fraction of the VALU issue rate -- 64 lanes / ((4 W + 0.5) instructions x 4 cycles) per SIMD and clock, the figure bench.py
uses for the XOR + popcount scan (W = 64-bit words per row).

usage: python tools/bench_duplicates.py [--reps 3] [--sizes 1000000,10000000] [--nphd-rows 1000000] [--tau 6]
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


def run(engine, metric, nbytes, n, tau, reps):
    t = engine.open_table(metric, 1, nbytes)
    try:
        t.add_synthetic(nbytes, n, seed=1234 + n, first_row=0, key_base=1)
        mh = np.full(_lib.MAX_BYTES + 1, -1, dtype=np.int16)
        mh[nbytes] = tau
        t.join_within(mh, 1 << 20)                      # warm-up (code objects, buffers)
        best, pairs_found = None, 0
        for _ in range(reps):
            t0 = time.perf_counter()
            out = t.join_within(mh, 1 << 20)            # ends in a device synchronise (the pair count is read back)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
            pairs_found = len(out[2])
        words = (nbytes + 7) // 8
        pairs = n * (n - 1) / 2
        rate = pairs / best
        return {"table": f"{'HAMMING' if metric == _lib.METRIC_HAMMING else 'NPHD'} {8 * nbytes}-bit", "rows": n, "tau": tau,
                "seconds": round(best, 5), "pair_distances_per_s": float(f"{rate:.4g}"), "pairs_found": pairs_found,
                "valu_issue_fraction": round(rate / valu_peak_pairs(words), 3)}
    finally:
        t.drop()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="1000000,10000000", help="row counts of the 64-bit tables")
    ap.add_argument("--nphd-rows", type=int, default=1_000_000, help="rows of the 256-bit NPHD table (0: skip)")
    ap.add_argument("--tau", type=int, default=6, help="max Hamming distance of the 64-bit tables (4x that for 256 bits)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    engine = HipEngine(a.device)
    try:
        for n in [int(s) for s in a.sizes.split(",") if s]:
            print(json.dumps(run(engine, _lib.METRIC_HAMMING, 8, n, a.tau, a.reps)), flush=True)
        if a.nphd_rows:
            print(json.dumps(run(engine, _lib.METRIC_NPHD, 32, a.nphd_rows, 4 * a.tau, a.reps)), flush=True)
    finally:
        engine.close()


if __name__ == "__main__":
    main()
