"""
Per-unit reference of the unit part of ``search_assets`` (TEST INFRASTRUCTURE), as the reference backend runs it
(``iscc_search/indexes/usearch/index.py:786-839``, ``:1957-2045``): one search per query unit through the public vector-index
API, plain dicts and Python floats.  Shares nothing with ``iscc_search_amd.unit_match``, which it checks.
"""

import numpy as np

from iscc_search_amd import codec
from iscc_search_amd._lib import MAX_K

FIRST_K = 64     # an INSTANCE prefix match asks for this many first, then for everything up to MAX_K


def search_unit(idx, unit_type, body, limit):
    """{key: score} of one query unit against its table of ``HipIndex`` idx, in the table's result order; {} without a table."""
    table = idx._unit_tables.get(unit_type)
    if table is None:
        return {}
    vector = np.frombuffer(body, dtype=np.uint8)
    if unit_type.startswith("INSTANCE_"):            # bidirectional prefix match: every hit scores 1.0
        m = table.search_within(vector, count=FIRST_K, max_hamming=0)
        if len(m.keys) == FIRST_K:
            m = table.search_within(vector, count=MAX_K, max_hamming=0)
        return {int(key): 1.0 for key in m.keys}
    m = table.search(vector, count=limit)
    return {int(key): max(0.0, 1.0 - float(distance)) for key, distance in zip(m.keys, m.distances)}


def global_matches(idx, query, limit):
    """[(iscc_id, score, {unit_type: score})] that ``search_assets(query, limit)`` on ``HipIndex`` idx lists as global matches."""
    units, exclude = query.units, None
    if query.iscc_id:
        units, exclude = idx.get_asset(query.iscc_id).units, codec.iscc_id_to_int(query.iscc_id)
    elif not units:
        units = [str(u) for u in codec.code_units(query.iscc_code)]
    merged = {}
    for unit_str in units:
        unit = codec.Iscc(unit_str)
        for key, score in search_unit(idx, unit.unit_type, unit.body, limit).items():
            types = merged.setdefault(key, {})
            types[unit.unit_type] = max(score, types.get(unit.unit_type, 0.0))       # max per (key, type)
    thr, exp = idx._opts.match_threshold_units, idx._opts.confidence_exponent
    scored = []
    for key, types in merged.items():
        confident = [s for s in types.values() if s >= thr]
        if confident and key != exclude:
            scored.append((key, sum(s**exp for s in confident) / sum(confident), types))
    scored.sort(key=lambda r: r[1], reverse=True)                                     # stable: ties keep their merge order
    return [(codec.iscc_id_from_int(key, idx._realm_id or 0), min(1.0, total), types) for key, total, types in scored[:limit]]
