"""
Asset pairs by device joins: the host side of ``HipIndex.find_duplicates`` (``HipTable.join_within``) and ``find_matches``
(``HipTable.join_between``), scored as ``search_assets`` scores (``unit_match``).  A *side* of a join is ``(tables, asset_units)``:
unit type -> ``HipNphdIndex``, and asset key -> {unit_type: body} as indexed.  And asset GROUPS by the same joins with a union-find
on the device where the pairs were (``find_duplicate_groups``, ``HipTable.join_components``).  And asset pairs that share CHUNKS, by a
join of the simprint tables aggregated on the device (``shared_sides``, ``HipSimprintIndex.shared``): a self-join per table for
``find_shared_content``, a cross join of the two tables of every type for ``find_shared_matches``; with ``segments=True`` the same
join also locates the shared chunks.  And the HUBS of a unit table -- rows with more near-duplicates than a caller wants to see as pairs (a black
frame, silence, 10 000 re-uploads of one file) -- by a count per row on the device where the pairs were (``table_degrees``,
``HipTable.join_degrees``): ``find_hubs`` lists them, and ``max_degree`` keeps them out of the pairs and the groups.
"""

from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np

from iscc_search_amd.unit_match import _confidence_total, _is_instance, _unit_max_hamming, _unit_scores


@dataclass
class DuplicatePair:
    """One near-duplicate pair of ``find_duplicates``: ``score`` and ``types`` as ``search_assets`` from either asset lists the other."""

    iscc_id_a: str      # the smaller key
    iscc_id_b: str
    score: float
    types: Dict[str, float]   # the confident unit scores, in the unit order of asset a


@dataclass
class Hub:
    """One entry of ``find_hubs``: an asset and how many other assets are near-duplicates of it in one unit type."""

    iscc_id: str
    unit_type: str
    degree: int             # other assets that carry the type and whose unit is within the threshold of this asset's


@dataclass
class IndexMatch:
    """One pair of ``find_matches``: ``score`` and ``types`` as ``search_assets`` on the other index by asset a's units lists asset b."""

    iscc_id_a: str      # the asset of the index find_matches was called on
    iscc_id_b: str      # the asset of the other index
    score: float
    types: Dict[str, float]   # the confident unit scores, in the unit order of asset a


@dataclass
class DuplicateGroup:
    """One group of ``find_duplicate_groups``: a connected component of the near-duplicate pairs."""

    iscc_ids: List[str]     # ascending by key
    size: int


@dataclass
class SharedSegment:
    """One aligned run of a ``SharedChunks``: consecutive chunks of a (by offset) that match consecutive chunks of b."""

    offset_a: int           # bytes offset_a .. end_a of asset a ...
    end_a: int
    offset_b: int           # ... are bytes offset_b .. end_b of asset b
    end_b: int
    first_chunk_a: int      # the run's first chunk on either side: its rank among its asset's chunks by (offset, size)
    first_chunk_b: int
    chunks: int             # matched chunk pairs in the run
    span: int               # chunk ordinals covered on one side: ``chunks`` plus the gaps that ``max_gap`` bridged
    similarity: float       # 1 - sum of the pairs' distances / (chunks * ndim)


@dataclass
class SharedChunks:
    """One simprint type of a ``SharedContent`` pair: how much of each asset's chunks has a match in the other asset."""

    matched_a: int          # chunks of a with at least one chunk of b within the match threshold
    chunks_a: int           # chunks of a of this type, stop chunks included
    matched_b: int
    chunks_b: int
    chunk_pairs: int        # matching (chunk of a, chunk of b) pairs
    coverage_a: float       # mean over a's chunks of the best similarity 1 - d / ndim found in b, 0 where none
    coverage_b: float
    segments: Optional[List[SharedSegment]] = None   # with ``segments=True``: where, ordered by (offset_a, offset_b)


@dataclass
class SharedContent:
    """One pair of ``find_shared_content``: two assets that share chunks in at least one simprint type."""

    iscc_id_a: str          # the smaller key
    iscc_id_b: str
    score: float            # mean over ``types`` of max(coverage_a, coverage_b)
    types: Dict[str, SharedChunks]


@dataclass
class SharedMatch:
    """One pair of ``find_shared_matches``: an asset of the calling index and an asset of the other index that share chunks."""

    iscc_id_a: str          # the asset of the index find_shared_matches was called on
    iscc_id_b: str          # the asset of the other index
    score: float            # mean over ``types`` of max(coverage_a, coverage_b)
    types: Dict[str, SharedChunks]


def _merge_join(pair_scores, unit_type, join, instance, units_a, units_b):
    # type: (Dict[tuple, Dict[str, float]], str, tuple, bool, Dict[int, Dict[str, bytes]], Dict[int, Dict[str, bytes]]) -> None
    """One unit table's join result into the per-pair unit scores; ``units_a`` / ``units_b``: each side's units as indexed."""
    keys_a, keys_b, ham, pbits = join
    scores = [1.0] * len(ham) if instance else _unit_scores(ham, pbits).tolist()     # INSTANCE pairs score 1.0
    for a, b, score in zip(keys_a.tolist(), keys_b.tolist(), scores):
        ua, ub = units_a.get(a), units_b.get(b)
        # a row an update left behind in a table of a type the asset no longer carries is not compared
        if ua is None or ub is None or unit_type not in ua or unit_type not in ub:
            continue
        pair_scores.setdefault((a, b), {})[unit_type] = score


def _rank_pairs(pair_scores, units_a, thr, exp, min_score):
    # type: (Dict[tuple, Dict[str, float]], Dict[int, Dict[str, bytes]], float, int, Optional[float]) -> list
    """[(key_a, key_b, score, confident unit scores)] of the pairs with a confident unit, score descending, then (key_a, key_b)."""
    out = []
    for (a, b), by_type in pair_scores.items():
        # the unit order of asset a, as search_assets by a's units merges them
        confident = {t: by_type[t] for t in units_a[a] if t in by_type and by_type[t] >= thr}
        if not confident:
            continue
        score = min(1.0, _confidence_total(confident, exp))
        if min_score is not None and score < min_score:
            continue
        out.append((a, b, score, confident))
    out.sort(key=lambda r: (-r[2], r[0], r[1]))
    return out


def table_degrees(caller, units, unit_type, table, max_hamming):
    # type: (str, Dict[int, Dict[str, bytes]], str, object, np.ndarray) -> tuple
    """
    ``(live_keys, degrees)`` of one unit table at ``max_hamming``: its live rows -- those of the assets that carry ``unit_type`` as
    indexed, ascending by key; a row an update left behind in a table of a type its asset no longer carries is not among them --
    and for each the number of other live rows within the threshold (``HipTable.join_degrees``: counted on the device, no pairs).
    The one place that decides both, for ``find_hubs`` and for ``max_degree`` of the pairs and the groups.  Tables without
    ``join_degrees`` (a sharded engine's) raise NotImplementedError naming ``caller``.
    """
    if not hasattr(table, "join_degrees"):
        raise NotImplementedError(f"{caller} needs a single-GPU engine: pairs across shards need their rows exchanged")
    live_keys = np.array(sorted(k for k, by_type in units.items() if unit_type in by_type), dtype=np.uint64)
    degrees, _ = table.join_degrees(max_hamming, live_keys)
    return live_keys, degrees


def hub_side(caller, side, threshold, min_degree):
    # type: (str, tuple, float, int) -> list
    """[(key, unit_type, degree)] of every live row of ``side``'s unit tables with ``degree >= min_degree`` at ``match_threshold_units =
    threshold`` (``table_degrees``), ordered by (-degree, key, unit_type)."""
    tables, units = side
    out = []
    for unit_type in sorted(tables):
        live_keys, degrees = table_degrees(caller, units, unit_type, tables[unit_type]._table, _unit_max_hamming(threshold, _is_instance(unit_type)))
        keep = degrees >= min_degree
        out.extend((k, unit_type, d) for k, d in zip(live_keys[keep].tolist(), degrees[keep].tolist()))
    out.sort(key=lambda r: (-r[2], r[0], r[1]))
    return out


def join_sides(caller, side_a, side_b, opts, min_score, max_pairs, max_degree=None):
    # type: (str, tuple, tuple, object, Optional[float], int, Optional[int]) -> list
    """
    The ranked pairs (``_rank_pairs``) of side a's assets with side b's: ONE join per unit type both sides have a table for --
    a self-join where ``side_b`` is ``side_a`` -- at the largest distance per code length that ``opts``' threshold still calls
    confident, aggregated over the unit types both assets carry.  More than ``max_pairs`` unit pairs in one table raise
    ValueError; tables without the join (a sharded engine's) raise NotImplementedError naming ``caller``.
    ``max_degree`` (a self-join only): a live row with more than ``max_degree`` other live rows within its table's threshold is a HUB
    of that table and is left out of that table's join (``join_within`` with ``live_keys``), so its pairs neither appear nor count
    towards ``max_pairs``.  The degree is taken ONCE, in the full table (``table_degrees``), and not again after the hubs are gone: the
    rule by which ``max_doc_freq`` decides stop chunks.  None: no degree pass, and the calls made are those without the argument.
    """
    (tables_a, units_a), (tables_b, units_b) = side_a, side_b
    if max_degree is not None and side_b is not side_a:
        raise ValueError(f"{caller}: max_degree is defined within one index")
    thr, exp = opts.match_threshold_units, opts.confidence_exponent
    pair_scores = {}  # type: Dict[tuple, Dict[str, float]]
    for unit_type in sorted(set(tables_a) & set(tables_b)):
        table_a, table_b = tables_a[unit_type]._table, tables_b[unit_type]._table
        if not hasattr(table_a, "join_within" if side_b is side_a else "join_between"):
            raise NotImplementedError(f"{caller} needs a single-GPU engine: pairs across shards need their rows exchanged")
        instance = _is_instance(unit_type)
        max_hamming = _unit_max_hamming(thr, instance)
        if max_degree is not None:
            live_keys, degrees = table_degrees(caller, units_a, unit_type, table_a, max_hamming)
            join = table_a.join_within(max_hamming, max_pairs, live_keys[degrees <= max_degree])
        else:
            join = table_a.join_within(max_hamming, max_pairs) if side_b is side_a else table_a.join_between(table_b, max_hamming, max_pairs)
        _merge_join(pair_scores, unit_type, join, instance, units_a, units_b)
    return _rank_pairs(pair_scores, units_a, thr, exp, min_score)


def group_side(caller, side, threshold, min_size, max_degree=None):
    # type: (str, tuple, float, int, Optional[int]) -> list
    """
    The connected components of ``side``'s assets under the pairs ``join_sides(caller, side, side, ...)`` lists at
    ``match_threshold_units = threshold``: one uint64 array of asset keys (ascending) per component of at least ``min_size``
    assets, by size descending, then by smallest key.  Labels are the ranks of the sorted asset keys, so a component's smallest
    label is its smallest key; ONE ``join_components`` per unit table, in sorted type order, carries one ``parent`` array through
    them all.  Per table the live rows are those of the assets that carry its type: a row an update left behind in a table of a
    type its asset no longer carries links nothing (``_merge_join`` says the same for pairs).  ``max_degree``: as for ``join_sides``
    -- a table's hubs (``table_degrees``, taken once in the full table) are left out of its ``live_keys`` and link nothing there, so
    nothing chains through them; None: no degree pass.  Tables without ``join_components`` (a sharded engine's) raise
    NotImplementedError naming ``caller``.
    """
    tables, units = side
    keys = np.array(sorted(units), dtype=np.uint64)
    if len(keys) >= 0xFFFFFFFF:
        raise ValueError(f"{caller} labels assets with 32 bits: {len(keys)} assets are too many")
    parent = np.arange(len(keys), dtype=np.uint32)
    for unit_type in sorted(tables):
        table = tables[unit_type]._table
        if not hasattr(table, "join_components"):
            raise NotImplementedError(f"{caller} needs a single-GPU engine: pairs across shards need their rows exchanged")
        if not len(keys):
            continue
        max_hamming = _unit_max_hamming(threshold, _is_instance(unit_type))
        if max_degree is not None:
            live_keys, degrees = table_degrees(caller, units, unit_type, table, max_hamming)
            live_keys = live_keys[degrees <= max_degree]
        else:
            live_keys = np.array(sorted(k for k, by_type in units.items() if unit_type in by_type), dtype=np.uint64)
        live_labels = np.searchsorted(keys, live_keys).astype(np.uint32)
        table.join_components(max_hamming, live_keys, live_labels, parent)
    # parent is flat: parent[i] is the component's smallest label.  Members by (root, label); groups by (-size, root)
    roots, counts = np.unique(parent, return_counts=True)
    members = np.argsort(parent, kind="stable")
    starts = np.concatenate(([0], np.cumsum(counts)[:-1])).astype(np.int64)
    order = np.lexsort((roots, -counts.astype(np.int64)))
    order = order[counts[order] >= min_size]
    return [keys[members[starts[g]:starts[g] + counts[g]]] for g in order.tolist()]


def _located(records, ndim, min_segment, max_gap):
    # type: (np.ndarray, int, int, int) -> Dict[tuple, List[SharedSegment]]
    """
    {(src, dst): [SharedSegment]} of the device's segment records (sorted by (src, dst, diagonal, first_src)).  Runs of one asset pair
    on one diagonal are merged while the next run starts at most ``max_gap`` chunks behind the end of what was merged so far: chunks
    and distances add up, the span covers the gaps, the byte range runs from the first run's begin to the last run's end.  Kept: merged
    runs of at least ``min_segment`` chunks; ordered by (offset_a, offset_b).
    """
    merged = []     # [src, dst, diagonal, first_src, first_dst, chunks, span, sum_hamming, begin_src, begin_dst, end_src, end_dst]
    names = ("src", "dst", "first_src", "first_dst", "length", "sum_hamming", "begin_src", "begin_dst", "end_src", "end_dst")
    for src, dst, first_src, first_dst, length, sum_hamming, begin_src, begin_dst, end_src, end_dst in zip(*(records[f].tolist() for f in names)):
        last = merged[-1] if merged else None
        if last is not None and last[:3] == [src, dst, first_dst - first_src] and first_src - (last[3] + last[6]) <= max_gap:
            last[5] += length
            last[6] = first_src + length - last[3]
            last[7] += sum_hamming
            last[10], last[11] = end_src, end_dst
        else:
            merged.append([src, dst, first_dst - first_src, first_src, first_dst, length, length, sum_hamming, begin_src, begin_dst, end_src, end_dst])
    out = {}  # type: Dict[tuple, List[SharedSegment]]
    for src, dst, _, first_src, first_dst, chunks, span, sum_hamming, begin_src, begin_dst, end_src, end_dst in merged:
        if chunks >= min_segment:
            out.setdefault((src, dst), []).append(
                SharedSegment(begin_src, end_src, begin_dst, end_dst, first_src, first_dst, chunks, span, 1.0 - sum_hamming / (chunks * ndim)))
    for runs in out.values():
        runs.sort(key=lambda r: (r.offset_a, r.offset_b, r.first_chunk_a, r.first_chunk_b))
    return out


def shared_sides(caller, side_a, side_b, threshold, max_doc_freq, max_pairs, min_chunks, min_coverage, skip_same_asset, segments, min_segment,
                 max_gap):
    # type: (str, tuple, tuple, float, int, int, int, Optional[float], bool, bool, int, int) -> list
    """
    [(key_a, key_b, score, {sp_type: SharedChunks})] of the pairs (asset of side a, asset of side b) that share chunks: ONE join per
    simprint type both sides have a table for, in sorted type order (``HipSimprintIndex.shared``) -- a self-join where ``side_b`` is
    ``side_a``, and then key_a < key_b -- over the assets ``bodies[sp_type]`` (8-byte bodies) of either side.  Per type a pair has two
    device records, a -> b and b -> a (``reserved`` 1 in a cross join, where labels are per side); ``coverage_x = (matched_x -
    sum_hamming_x / ndim) / chunks_x`` and the type's score is the larger coverage (the smaller work lies inside the larger).
    ``score`` is the mean of the types' scores over the types in which the pair has a record -- the rule
    ``chunk_match.rank_simprint_matches`` uses across types.  Kept: pairs with ``max(matched_a, matched_b) >= min_chunks`` in some type
    and ``score >= min_coverage`` (if given); ordered by score descending, then (key_a, key_b).  Stop chunks are decided per table;
    ``skip_same_asset`` keeps an asset held by both sides from pairing with itself.  More than ``max_pairs`` chunk pairs in one join
    raise ValueError; tables without the join (a sharded engine's) raise NotImplementedError naming ``caller``.  ``segments``: the same
    join also says WHERE, and every ``SharedChunks`` carries its ``SharedSegment`` list, merged over gaps of at most ``max_gap`` chunks
    and cut at ``min_segment`` chunks (``_located``); a is ``src`` of every device segment -- the asset of side a, or in a self-join
    the smaller label, labels being ranks of ascending keys.
    """
    (tables_a, bodies_a), (tables_b, bodies_b) = side_a, side_b
    within = side_b is side_a
    by_pair = {}  # type: Dict[tuple, Dict[str, SharedChunks]]
    for sp_type in sorted(set(tables_a) & set(tables_b)):
        table_a, table_b = tables_a[sp_type], tables_b[sp_type]
        if not table_a.joins_shared(None if within else table_b, segments):
            raise NotImplementedError(f"{caller} needs a single-GPU engine: pairs across shards need their rows exchanged")
        listed_a = sorted(bodies_a.get(sp_type, ()))
        listed_b = listed_a if within else sorted(bodies_b.get(sp_type, ()))
        if not listed_a or not listed_b:
            continue
        records, chunks_a, chunks_b, _, runs = table_a.shared(listed_a, threshold, max_doc_freq, max_pairs, None if within else table_b,
                                                              None if within else listed_b, skip_same_asset, segments)
        located = _located(runs, table_a.ndim, min_segment, max_gap) if segments else None
        keys_a = [int.from_bytes(b, "big") for b in listed_a]
        keys_b = keys_a if within else [int.from_bytes(b, "big") for b in listed_b]
        ndim = table_a.ndim
        chunks_a = chunks_a.tolist()
        chunks_b = chunks_a if within else chunks_b.tolist()
        rows = {(r, s, d): (m, h, p) for r, s, d, m, h, p in zip(records["reserved"].tolist(), records["src"].tolist(), records["dst"].tolist(),
                                                                records["matched"].tolist(), records["sum_hamming"].tolist(),
                                                                records["chunk_pairs"].tolist())}
        back = 0 if within else 1       # a self-join's records are all of direction 0: the pair's first is the one with a < b
        for (direction, a, b), (matched_a, sum_a, pairs) in rows.items():
            if direction or (within and a > b):
                continue
            matched_b, sum_b, _ = rows[(back, b, a)]
            by_pair.setdefault((keys_a[a], keys_b[b]), {})[sp_type] = SharedChunks(
                matched_a, chunks_a[a], matched_b, chunks_b[b], pairs, (matched_a - sum_a / ndim) / chunks_a[a], (matched_b - sum_b / ndim) / chunks_b[b],
                None if located is None else located.get((a, b), []))
    return _rank_shared(by_pair, min_chunks, min_coverage)


def _rank_shared(by_pair, min_chunks, min_coverage):
    # type: (Dict[tuple, Dict[str, SharedChunks]], int, Optional[float]) -> list
    """[(key_a, key_b, score, types)] of the pairs kept by ``min_chunks`` / ``min_coverage``: score descending, then (key_a, key_b)."""
    out = []
    for (a, b), types in by_pair.items():
        if not any(max(t.matched_a, t.matched_b) >= min_chunks for t in types.values()):
            continue
        score = sum(max(t.coverage_a, t.coverage_b) for t in types.values()) / len(types)
        if min_coverage is not None and score < min_coverage:
            continue
        out.append((a, b, score, types))
    out.sort(key=lambda r: (-r[2], r[0], r[1]))
    return out
