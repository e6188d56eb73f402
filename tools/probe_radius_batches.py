#!/usr/bin/env python3
"""
What the fixed-radius pass of large 64-bit batches (engine option ``radius_batches``) does over a rotation of query batches, beside the
hinted single pass (``radius_batches=0``) on the same table in the same process -> profiles/radius_batches_ab.txt.

Per arm: wall and scan time per step (HIP events around the scan launches, inside the engine), steps that stood / did not, queries
repaired per step, scan launches per step, and -- from a second, shorter loop under ``count_candidates`` -- candidates per query.

usage (GPU box): python tools/probe_radius_batches.py [ROWS [QUERIES [K [STEPS [BATCHES]]]]]     defaults 100000000 1024 10 40 8
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from iscc_search_amd import _lib  # noqa: E402
from iscc_search_amd.engine import HipEngine  # noqa: E402


def main():
    rows, nq, k, steps, n_batches = (int(x) for x in (sys.argv[1:] + ["100000000", "1024", "10", "40", "8"][len(sys.argv) - 1 :])[:5])
    engine = HipEngine(0)
    for item in filter(None, os.environ.get("ISCC_HIP_OPTS", "").split(",")):
        engine.set_option(item.split("=")[0].strip(), int(item.split("=")[1]))
    t = engine.open_table(_lib.METRIC_HAMMING, 1, 8)
    t.add_synthetic(8, rows, 12345)
    rng = np.random.default_rng(7)
    batches = [rng.integers(1, 2**64, size=(nq, 1), dtype=np.uint64) for _ in range(n_batches)]

    def loop(n, **options):
        for name, value in options.items():
            engine.set_option(name, value)
        engine.stats(reset=True)
        t0 = time.perf_counter()
        for i in range(n):
            t.search(batches[i % n_batches], None, k)
        wall = (time.perf_counter() - t0) / n
        st = engine.stats(reset=True)
        for name in options:
            engine.set_option(name, 0)
        return wall, st

    print(f"== {rows} x 64-bit, {nq} queries, k = {k}, {n_batches} batches in rotation, {steps} steps per arm, arms alternating")
    for rnd in range(3):
        for arm in (1, 0):
            engine.set_option("radius_batches", arm)
            loop(2 * n_batches)           # the hint of this arm's steps settles
            wall, st = loop(steps, profile=1)
            _, sc = loop(n_batches, count_candidates=1)
            print(f"   radius_batches={arm} run {rnd + 1}: wall {wall * 1e3:.3f} ms/step, scan {st['scan_ms'] / steps:.3f} ms/step in "
                  f"{st['scan_launches'] / steps:.2f} launches; held {st['spec_hits']}, did not {st['spec_misses']}, "
                  f"repaired queries {st['spec_repairs'] / steps:.2f} per step, self_retries {st['self_retries']}; "
                  f"{sc['candidates'] / max(1, sc['candidate_batches']) / nq:.0f} candidates per query")
    engine.close()


if __name__ == "__main__":
    main()
