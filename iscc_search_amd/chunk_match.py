"""
Chunk (simprint) matching of ``HipIndex``: the per-type simprint searches of one query or of many, and their ranking into
``IsccChunkMatch`` lists (``iscc_search/indexes/usearch/index.py:1261-1469``).  Every function takes the index as ``idx``.
"""

from typing import Dict, List

from iscc_search_amd import codec
from iscc_search_amd.schema import IsccChunkMatch, IsccMatchedChunk, IsccQuery, Types


def _sp_string(s):
    return s.root if hasattr(s, "root") else s


def search_simprints(idx, query, limit, exact=False):
    # type: (object, IsccQuery, int, bool) -> List[IsccChunkMatch]
    """
    Per-type search, mean over types, order (-score, iscc_id): approximate-mode scoring of
    ``usearch/index.py:1357-1469``, or with ``exact`` the hard-boundary collision search of ``:1261-1355``.
    """
    total_assets = len(idx._assets)
    per_type = []
    for sp_type, simprint_objs in query.simprints.items():
        table = idx._sp_tables.get(sp_type)
        if table is None:
            continue
        q_bytes = [codec.decode_base64(_sp_string(s)) for s in simprint_objs]
        if exact:
            raw = table.search_exact(simprints=q_bytes, limit=limit * 2, threshold=idx._opts.match_threshold_simprints, detailed=True)
        else:
            raw = table.search_raw(
                simprints=q_bytes, limit=limit * 2, threshold=idx._opts.match_threshold_simprints, detailed=True,
                total_assets=total_assets, device_doc_freq=True,   # lmdb_ops.count_doc_freq, on the device
            )
        per_type.append((sp_type, raw))
    return rank_simprint_matches(idx, per_type, limit)


def search_simprints_many(idx, prepared, limit, exact=False):
    # type: (object, list, int, bool) -> Dict[int, list]
    """
    The simprint searches of ``search_simprints`` for every prepared query: per simprint type one ``search_raw_many`` -- with
    ``exact`` one ``search_exact_many`` -- over the queries that carry it, with ``search_simprints``' arguments.  Returns query
    index -> [(simprint type, SimprintMatchRaw list)] in each query's type order.
    """
    if not idx._sp_tables:
        return {}
    total_assets = len(idx._assets)
    requests = {}  # type: Dict[str, list]          simprint type -> [(query index, query simprints)]
    for i, (query, _, _) in enumerate(prepared):
        for sp_type, simprint_objs in (query.simprints or {}).items():
            if sp_type in idx._sp_tables:
                requests.setdefault(sp_type, []).append((i, [codec.decode_base64(_sp_string(s)) for s in simprint_objs]))
    found = {}  # type: Dict[tuple, list]
    for sp_type, items in requests.items():
        if exact:
            raws = idx._sp_tables[sp_type].search_exact_many(
                [q_bytes for _, q_bytes in items], limit=limit * 2, threshold=idx._opts.match_threshold_simprints, detailed=True)
        else:
            raws = idx._sp_tables[sp_type].search_raw_many(
                [q_bytes for _, q_bytes in items], limit=limit * 2, threshold=idx._opts.match_threshold_simprints, detailed=True,
                total_assets=total_assets, device_doc_freq=True,
            )
        for (i, _), raw in zip(items, raws):
            found[(i, sp_type)] = raw
    return {i: [(t, found[(i, t)]) for t in (query.simprints or {}) if (i, t) in found] for i, (query, _, _) in enumerate(prepared)}


def rank_simprint_matches(idx, per_type, limit):
    # type: (object, list, int) -> List[IsccChunkMatch]
    """The chunk matches of one query from its per-type ``SimprintMatchRaw`` lists (in the query's type order): mean over types, order (-score, iscc_id)."""
    per_asset = {}  # type: Dict[bytes, Dict[str, object]]
    for sp_type, raw in per_type:
        for r in raw:
            per_asset.setdefault(r.iscc_id_body, {})[sp_type] = r
    if not per_asset:
        return []
    ranked = []
    for body, type_results in per_asset.items():
        score = sum(r.score for r in type_results.values()) / len(type_results)
        digest = codec.decode_base32(codec.iscc_id_from_int(int.from_bytes(body, "big"), idx._realm_id or 0)[5:])
        ranked.append((score, digest, body, type_results))
    ranked.sort(key=lambda x: (-x[0], x[1]))
    out = []
    for score, digest, body, type_results in ranked[:limit]:
        source, metadata = idx._source_metadata(int.from_bytes(body, "big"))
        types = {}
        for sp_type, r in type_results.items():
            chunks = None
            if r.chunks is not None:
                chunks = [
                    IsccMatchedChunk(query=codec.encode_base64(c.query), match=codec.encode_base64(c.match),
                                     score=c.score, freq=max(1, c.freq), offset=c.offset, size=c.size, content=None)
                    for c in r.chunks
                ]
            types[sp_type] = Types(score=r.score, matches=r.matches, queried=r.queried, chunks=chunks)
        out.append(IsccChunkMatch(iscc_id="ISCC:" + codec.encode_base32(digest), score=score, types=types, source=source, metadata=metadata))
    return out
