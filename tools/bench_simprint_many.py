#!/usr/bin/env python3
"""
Batched simprint search (HipSimprintIndex.search_raw_many: isccsearch_simprint_score_many) beside the per-request search_raw
loop, in one run, on one 128-bit simprint table of --chunks chunk fingerprints (40 per asset: the BASELINE config 5 table).

    python tools/bench_simprint_many.py                      # 10 M chunks, 1 024 requests x {16, 64} simprints, limits {20, 200}
    python tools/bench_simprint_many.py --chunks 1000000 --requests 256
    python tools/bench_simprint_many.py --exact              # hard-boundary requests: search_exact_many beside the search_exact loop

Requests: stored chunks with two bits flipped (approximate matches), threshold 0.75, detailed, device document frequencies
(the arguments search_assets uses).  Per (simprints per request, limit) the two forms alternate --repeats times after a
warm-up; every repeat prints requests/s of each, and the summary their medians and spread, the library searches and scan
launches per batch (engine.stats()), and whether both forms returned identical results (scores compared with ==).
Then search_assets_many against per-call search_assets on a manager index whose queries carry units and one simprint type.

--exact: the hard-boundary mode on the same table instead -- HipSimprintIndex.search_exact_many (isccsearch_simprint_exact_many)
beside a loop of search_exact, requests of stored chunks as they are (collisions), limit 20, detailed, dup_limit 1 000 (the
arguments search_assets(exact=True) uses), at --requests requests of 16, 64 and 200 simprints and at 2 requests of 1 simprint
(--exact-shapes 2x1,4x1,8x16: other (requests x simprints) shapes, e.g. the small ones that decide EXACT_MANY_FROM).
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from iscc_search_amd import codec  # noqa: E402
from iscc_search_amd.engine import HipEngine  # noqa: E402
from iscc_search_amd.index import HipIndexManager  # noqa: E402
from iscc_search_amd.schema import IsccEntry, IsccIndex, IsccQuery, IsccSimprint  # noqa: E402
from iscc_search_amd.simprint import HipSimprintIndex  # noqa: E402

CHUNKS_PER_ASSET = 40


def build(eng, n_chunks, rng, ndim=128):
    idx = HipSimprintIndex(eng, ndim=ndim)
    nb = ndim // 8
    picks = []
    for lo in range(0, n_chunks, 1 << 20):
        n = min(1 << 20, n_chunks - lo)
        rows = np.arange(lo, lo + n, dtype=np.uint64)
        keys = np.stack([rows // np.uint64(CHUNKS_PER_ASSET) + np.uint64(1),
                         ((rows % np.uint64(CHUNKS_PER_ASSET)) * np.uint64(100) << np.uint64(32)) | np.uint64(100)], axis=1)
        vecs = rng.integers(0, 256, size=(n, nb), dtype=np.uint8)
        idx._index.add(keys, vecs, trusted_unique=True)
        picks.append(vecs[rng.integers(0, n, size=max(1, (1 << 17) * n // n_chunks))].copy())
    return idx, np.concatenate(picks)


def same(a, b):
    key = lambda res: [[(r.iscc_id_body, r.score, r.matches, [(c.query, c.match, c.score, c.offset, c.size, c.freq) for c in r.chunks or []])
                        for r in x] for x in res]
    return key(a) == key(b)


def spread(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 1), min=round(xs[0], 1), max=round(xs[-1], 1), spread_pct=round(100 * (xs[-1] - xs[0]) / xs[len(xs) // 2], 1))


def raw_bench(eng, idx, pool, args, n_assets, rng):
    in_lib = [0.0]
    for name in ("score_assets", "score_assets_many"):     # wall time inside the library calls (search, scoring, synchronisations)
        inner = getattr(idx._index, name)

        def timed(*a, _inner=inner, **kw):
            t = time.perf_counter()
            try:
                return _inner(*a, **kw)
            finally:
                in_lib[0] += time.perf_counter() - t

        setattr(idx._index, name, timed)
    for nsp in (16, 64):
        for limit in (20, 200):
            q = pool[rng.integers(0, len(pool), size=args.requests * nsp)].copy()
            q[:, 0] ^= np.uint8(3)
            reqs = [[bytes(r) for r in q[i * nsp:(i + 1) * nsp]] for i in range(args.requests)]
            kw = dict(limit=limit, threshold=0.75, detailed=True, total_assets=n_assets, device_doc_freq=True)
            loop = lambda: [idx.search_raw(r, **kw) for r in reqs]
            many = lambda: idx.search_raw_many(reqs, **kw)
            ok = same(loop(), many())                    # (also the warm-up of both)
            rates = {"loop": [], "many": []}
            lib_ms = {"loop": [], "many": []}
            stats = {}
            for rep in range(args.repeats):
                for form, fn in (("loop", loop), ("many", many)) if rep % 2 == 0 else (("many", many), ("loop", loop)):
                    s0 = eng.stats()
                    in_lib[0] = 0.0
                    t0 = time.perf_counter()
                    fn()
                    dt = time.perf_counter() - t0
                    s1 = eng.stats()
                    rates[form].append(args.requests / dt)
                    lib_ms[form].append(in_lib[0] * 1e3)
                    stats[form] = dict(searches_per_batch=s1["searches"] - s0["searches"], scan_launches_per_batch=s1["scan_launches"] - s0["scan_launches"],
                                       mfma_launches_per_batch=s1["mfma_launches"] - s0["mfma_launches"])
                    print(json.dumps(dict(repeat=rep, simprints=nsp, limit=limit, form=form, requests_per_s=round(args.requests / dt, 1),
                                          ms_per_batch=round(dt * 1e3, 2), ms_in_library_per_batch=round(in_lib[0] * 1e3, 2))), flush=True)
            lo, ma = spread(rates["loop"]), spread(rates["many"])
            print(json.dumps(dict(summary="search_raw", chunks=idx.size, requests=args.requests, simprints=nsp, limit=limit, identical=ok,
                                  loop_requests_per_s=lo, many_requests_per_s=ma, speedup=round(ma["median"] / lo["median"], 2),
                                  loop_ms_in_library=spread(lib_ms["loop"])["median"], many_ms_in_library=spread(lib_ms["many"])["median"],
                                  loop=stats["loop"], many=stats["many"])), flush=True)


def exact_bench(eng, idx, pool, args, rng):
    in_lib = [0.0]
    for name in ("exact_assets", "exact_assets_many", "search_arrays"):     # wall time inside the library calls of either form
        inner = getattr(idx._index, name)

        def timed(*a, _inner=inner, **kw):
            t = time.perf_counter()
            try:
                return _inner(*a, **kw)
            finally:
                in_lib[0] += time.perf_counter() - t

        setattr(idx._index, name, timed)
    for n_req, nsp in args.exact_shapes:
        q = pool[rng.integers(0, len(pool), size=n_req * nsp)]
        reqs = [[bytes(r) for r in q[i * nsp:(i + 1) * nsp]] for i in range(n_req)]
        kw = dict(limit=20, threshold=0.0, detailed=True, dup_limit=args.dup_limit)
        loop = lambda: [idx.search_exact(r, **kw) for r in reqs]
        many = lambda: idx.search_exact_many(reqs, **kw)
        first = many()
        ok = same(loop(), first)                     # (also the warm-up of both)
        rates = {"loop": [], "many": []}
        lib_ms = {"loop": [], "many": []}
        stats = {}
        for rep in range(args.repeats):
            for form, fn in (("loop", loop), ("many", many)) if rep % 2 == 0 else (("many", many), ("loop", loop)):
                s0 = eng.stats()
                in_lib[0] = 0.0
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                s1 = eng.stats()
                rates[form].append(n_req / dt)
                lib_ms[form].append(in_lib[0] * 1e3)
                stats[form] = dict(searches_per_batch=s1["searches"] - s0["searches"], scan_launches_per_batch=s1["scan_launches"] - s0["scan_launches"],
                                   mfma_launches_per_batch=s1["mfma_launches"] - s0["mfma_launches"])
                print(json.dumps(dict(repeat=rep, requests=n_req, simprints=nsp, form=form, requests_per_s=round(n_req / dt, 1),
                                      ms_per_batch=round(dt * 1e3, 2), ms_in_library_per_batch=round(in_lib[0] * 1e3, 2))), flush=True)
        lo, ma = spread(rates["loop"]), spread(rates["many"])
        print(json.dumps(dict(summary="search_exact", chunks=idx.size, requests=n_req, simprints=nsp, limit=20, dup_limit=args.dup_limit, identical=ok,
                              results=sum(len(r) for r in first), loop_requests_per_s=lo, many_requests_per_s=ma,
                              speedup=round(ma["median"] / lo["median"], 2),
                              loop_ms_in_library=spread(lib_ms["loop"])["median"], many_ms_in_library=spread(lib_ms["many"])["median"],
                              loop=stats["loop"], many=stats["many"])), flush=True)


def assets_bench(args, rng):
    m = HipIndexManager("hip:///")
    m.create_index(IsccIndex(name="bench"))
    bases = rng.integers(0, 256, size=(256, 3, 8), dtype=np.uint8)
    sp_pool = rng.integers(0, 256, size=(4096, 16), dtype=np.uint8)
    assets = []
    for i in range(args.manager_assets):
        b = bases[i % 256]
        units = [codec.encode_unit(codec.MT_META, 0, 0, b[0].tobytes()), codec.encode_unit(codec.MT_CONTENT, 0, 0, b[1].tobytes()),
                 codec.encode_unit(codec.MT_DATA, 0, 0, b[2].tobytes()),
                 codec.encode_unit(codec.MT_INSTANCE, 0, 0, rng.integers(0, 256, size=8, dtype=np.uint8).tobytes())]
        sps = [IsccSimprint(simprint=codec.encode_base64(sp_pool[int(j)].tobytes()), offset=10 * c, size=10)
               for c, j in enumerate(rng.integers(0, len(sp_pool), size=8))]
        assets.append(IsccEntry(iscc_id=codec.iscc_id_from_int(((1_000_000 + i) << 12) | (i & 0xFFF), 0), units=units,
                                simprints={"CONTENT_TEXT_V0": sps}))
    m.add_assets("bench", assets)
    queries = []
    for i in rng.integers(0, len(assets), size=args.requests):
        a = assets[int(i)]
        sps = [codec.encode_base64(sp_pool[int(j)].tobytes()) for j in rng.integers(0, len(sp_pool), size=16)]
        queries.append(IsccQuery(units=list(a.units), simprints={"CONTENT_TEXT_V0": sps}))
    eng = m._index("bench")._engine
    limit = 100
    many = lambda: m.search_assets_many("bench", queries, limit)
    loop = lambda: [m.search_assets("bench", q, limit) for q in queries]
    ok = [r.model_dump() for r in many()] == [r.model_dump() for r in loop()]
    rates = {"loop": [], "many": []}
    stats = {}
    for rep in range(args.repeats):
        for form, fn in (("loop", loop), ("many", many)) if rep % 2 == 0 else (("many", many), ("loop", loop)):
            s0 = eng.stats()
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            s1 = eng.stats()
            rates[form].append(len(queries) / dt)
            stats[form] = dict(searches_per_batch=s1["searches"] - s0["searches"])
    lo, ma = spread(rates["loop"]), spread(rates["many"])
    print(json.dumps(dict(summary="search_assets_many", assets=args.manager_assets, queries=len(queries), units=4, simprint_types=1,
                          simprints_per_query=16, limit=limit, identical=ok, loop_queries_per_s=lo, many_queries_per_s=ma,
                          speedup=round(ma["median"] / lo["median"], 2), loop=stats["loop"], many=stats["many"])), flush=True)
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=10_000_000)
    ap.add_argument("--requests", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--manager-assets", type=int, default=20_000)
    ap.add_argument("--skip-raw", action="store_true")
    ap.add_argument("--exact", action="store_true", help="the hard-boundary mode: search_exact_many beside the search_exact loop, and nothing else")
    ap.add_argument("--dup-limit", type=int, default=1000, help="--exact: collisions listed per simprint (the rows per lookup of the batched form)")
    ap.add_argument("--exact-shapes", default=None, help="requests x simprints per request, comma-separated (default: REQUESTSx16,REQUESTSx64,REQUESTSx200,2x1)")
    args = ap.parse_args()
    shapes = args.exact_shapes or f"{args.requests}x16,{args.requests}x64,{args.requests}x200,2x1"
    args.exact_shapes = [tuple(int(v) for v in item.split("x")) for item in shapes.split(",")]
    rng = np.random.default_rng(0)
    if not args.skip_raw:
        eng = HipEngine(0)
        for item in filter(None, os.environ.get("ISCC_HIP_OPTS", "").split(",")):      # e.g. ISCC_HIP_OPTS=mfma=0
            eng.set_option(item.split("=")[0].strip(), int(item.split("=")[1]))
        t0 = time.perf_counter()
        idx, pool = build(eng, args.chunks, rng)
        print(json.dumps(dict(table="simprints ndim 128", chunks=idx.size, assets=args.chunks // CHUNKS_PER_ASSET, build_s=round(time.perf_counter() - t0, 1))), flush=True)
        if args.exact:
            exact_bench(eng, idx, pool, args, rng)
        else:
            raw_bench(eng, idx, pool, args, args.chunks // CHUNKS_PER_ASSET, rng)
        idx.close()
        eng.close()
    if not args.exact:
        assets_bench(args, rng)


if __name__ == "__main__":
    main()
