"""
Bulk asset search rates (HipIndex.match_units_many / search_assets_many) beside the per-call search_assets rate, in one run.

    python tools/bench_assets_batch.py --assets 2500 --batch 1024 --limits 10,100
    python tools/bench_assets_batch.py --assets 1000000

Index: `--assets` assets x 4 units (META 64-bit, CONTENT-TEXT 64-bit, DATA 64-bit, INSTANCE 64-bit), near-duplicates of 256
base codes (1-3 bits flipped), so that keys recur across the unit lists.  Queries: the units of stored assets.  Prints one JSON
line per (form, limit): queries/s, ms per batch, the share of it spent inside the library call (isccsearch_match_assets:
searches, scoring, synchronisations; the rest is the host's preparation and unpacking), and per batch the engine's searches and
scan launches (stats()).
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from iscc_search_amd import codec  # noqa: E402
from iscc_search_amd.index import HipIndexManager  # noqa: E402
from iscc_search_amd.schema import IsccEntry, IsccIndex, IsccQuery  # noqa: E402


def build(m, n, rng):
    bases = rng.integers(0, 256, size=(256, 4, 8), dtype=np.uint8)
    ids = [codec.iscc_id_from_int(((1_000_000 + i) << 12) | (i & 0xFFF), 0) for i in range(n)]
    step = 50_000
    for first in range(0, n, step):
        assets = []
        for i in range(first, min(n, first + step)):
            b = bases[i % 256].copy()
            flips = rng.integers(0, 64, size=(3, 3))
            for t in range(3):
                for f in flips[t, : 1 + i % 3]:
                    b[t, f // 8] ^= 1 << (7 - f % 8)
            inst = rng.integers(0, 256, size=8, dtype=np.uint8).tobytes()
            units = [codec.encode_unit(codec.MT_META, 0, 0, b[0].tobytes()), codec.encode_unit(codec.MT_CONTENT, 0, 0, b[1].tobytes()),
                     codec.encode_unit(codec.MT_DATA, 0, 0, b[2].tobytes()), codec.encode_unit(codec.MT_INSTANCE, 0, 0, inst)]
            assets.append(IsccEntry(iscc_id=ids[i], units=units))
        m.add_assets("bench", assets)
    return ids


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--assets", type=int, default=2500)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--limits", default="10,100")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--single", type=int, default=300, help="per-call search_assets requests timed")
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    m = HipIndexManager("hip:///")
    m.create_index(IsccIndex(name="bench"))
    t0 = time.perf_counter()
    ids = build(m, args.assets, rng)
    build_s = time.perf_counter() - t0
    idx = m._index("bench")
    eng = idx._engine
    in_lib = [0.0]
    real = eng.match_assets

    def timed_match(*a):
        t = time.perf_counter()
        try:
            return real(*a)
        finally:
            in_lib[0] += time.perf_counter() - t

    eng.match_assets = timed_match
    picks = rng.integers(0, args.assets, size=args.batch)
    queries = [IsccQuery(units=list(idx.get_asset(ids[int(i)]).units)) for i in picks]
    for limit in (int(x) for x in args.limits.split(",")):
        base = dict(assets=args.assets, units=4, batch=args.batch, limit=limit, build_s=round(build_s, 1))
        for form, fn in (("match_units_many", lambda: idx.match_units_many(queries, limit)),
                         ("search_assets_many", lambda: m.search_assets_many("bench", queries, limit))):
            s0 = eng.stats()
            in_lib[0] = 0.0
            dt = timed(fn, args.steps, args.warmup)
            s1 = eng.stats()
            calls = args.steps + args.warmup
            lib_ms = in_lib[0] / calls * 1e3
            print(json.dumps(dict(base, form=form, qps=round(args.batch / dt), ms_per_batch=round(dt * 1e3, 3), ms_in_library_per_batch=round(lib_ms, 3),
                                  searches_per_batch=(s1["searches"] - s0["searches"]) / calls,
                                  scan_launches_per_batch=(s1["scan_launches"] - s0["scan_launches"]) / calls,
                                  mfma_launches_per_batch=(s1["mfma_launches"] - s0["mfma_launches"]) / calls)), flush=True)
        single = queries[: args.single]
        for q in single[:20]:
            m.search_assets("bench", q, limit)
        t0 = time.perf_counter()
        for q in single:
            m.search_assets("bench", q, limit)
        dt = (time.perf_counter() - t0) / len(single)
        print(json.dumps(dict(base, form="search_assets (per call)", qps=round(1 / dt), ms_per_call=round(dt * 1e3, 3))), flush=True)
    m.close()


if __name__ == "__main__":
    main()
