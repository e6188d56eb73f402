"""
Unit matching of ``HipIndex``: the unit part of ``search_assets`` for one or many prepared queries (``HipIndex._prepare``), as
``iscc_search/indexes/usearch/index.py:786-839`` scores, merges and ranks it.  Pure functions over arrays and dicts;
``search_units`` runs them behind ``engine.search_many``, ``match_prepared`` prefers the device's own aggregation
(``engine.match_assets``).  ``tables`` maps a unit type to its ``HipNphdIndex``.
"""

import sys
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np

from iscc_search_amd import _lib, codec
from iscc_search_amd._lib import MAX_K
from iscc_search_amd.engine import pack_bytes

INSTANCE_FIRST_K = 64   # records per query an INSTANCE prefix match asks for first (a full list is asked again up to MAX_K)

_SCORE_TABLES = {}


def _is_instance(unit_type):
    return unit_type.startswith("INSTANCE_")     # INSTANCE units match by prefix equality, every hit scoring 1.0; all others by NPHD similarity


def _unit_map(units):
    """{unit_type: body} of an asset's units as they are indexed: of one type at two lengths the last one wins (``usearch/index.py:423-430``)."""
    out = {}
    for unit_str in units or []:
        unit = codec.Iscc(unit_str)
        out[unit.unit_type] = unit.body
    return out


def _checked_limit(limit):
    # type: (int) -> int
    """
    The engine returns at most ``MAX_K`` (4 096) neighbours per query.  The reference hands ``limit`` to usearch
    unbounded (``usearch/index.py:2037``); rather than silently returning a shorter list than was asked for, a larger
    ``limit`` is refused (ValueError -> HTTP 400, ``server/search.py:43-46``).
    """
    if limit > MAX_K:
        raise ValueError(f"limit {limit} exceeds the {MAX_K} neighbours per query this backend returns")
    return max(1, limit)


def _check_instance_hits(count, unit_type):
    # type: (int, str) -> None
    """An identity (INSTANCE) match list that fills the engine's cap would be cut silently: refuse instead."""
    if count >= MAX_K:
        raise ValueError(f"more than {MAX_K - 1} assets share the queried {unit_type} prefix; refine the query (longer code)")


def _checked_instance_hits(count, unit_type, query_index):
    """``_check_instance_hits``, its refusal naming the query's index in a bulk call's ``queries``."""
    try:
        _check_instance_hits(count, unit_type)
    except ValueError as e:
        if query_index is None:
            raise
        raise ValueError(f"queries[{query_index}]: {e}") from e


@dataclass
class UnitMatches:
    """
    Raw answer of ``HipIndex.match_units_many``: per query the first ``counts[q]`` entries of every row are its assets in
    ``search_assets`` order.  ``type_index[q, r]`` lists the unit types of result r (indices into ``types``) in the insertion
    order of ``IsccGlobalMatch.types``, 255 past the last; ``type_scores`` holds their scores.
    """

    keys: np.ndarray          # u64 [nq, limit]
    scores: np.ndarray        # f64 [nq, limit], min(1.0, total)
    counts: np.ndarray        # u32 [nq]
    types: tuple              # unit type names
    type_index: np.ndarray    # u8 [nq, limit, len(types)]
    type_scores: np.ndarray   # f64 [nq, limit, len(types)]


def _unit_scores(ham, pbits):
    # type: (np.ndarray, np.ndarray) -> np.ndarray
    """
    THE unit score, ``max(0, 1 - float64(float32(h) / float32(bits)))``, of integer arrays: the float32 NPHD as
    ``HipNphdIndex.search`` hands it out, then the reference's float64 ``1.0 - d`` clamp (``usearch/index.py:2041-2043``) -- the
    same IEEE operations on the whole list at once (a float32 widens to float64 exactly).  The device's score table, the search
    merge and the joins all score through here.
    """
    dist = ham.astype(np.float32) / pbits.astype(np.float32)
    return np.maximum(0.0, 1.0 - dist.astype(np.float64))


def _unit_score_tables(exponent):
    """
    [prefix bytes 0..32][hamming 0..256]: the unit score (``_unit_scores``), and ``score ** exponent`` as CPython computes it
    (None when Python would raise).
    """
    tabs = _SCORE_TABLES.get(exponent)
    if tabs is None:
        with np.errstate(divide="ignore", invalid="ignore"):
            score = _unit_scores(np.arange(257)[None, :], np.arange(_lib.MAX_BYTES + 1)[:, None] * 8)
        score[0, :] = 0.0                                # (no code is 0 bytes long)
        try:
            pows = np.array([s**exponent for s in score.ravel().tolist()], dtype=np.float64)
        except (ZeroDivisionError, OverflowError, TypeError):
            pows = None
        tabs = _SCORE_TABLES[exponent] = (score.ravel().copy(), pows)
    return tabs


def _unit_max_hamming(thr, instance=False):
    # type: (float, bool) -> np.ndarray
    """
    max_hamming[p] for p = 1..32 prefix bytes: the largest h whose unit score (``_unit_scores`` at 8p bits) is >= ``thr``; -1
    where no h is.  INSTANCE units match by prefix equality, scoring 1.0: 0 everywhere (-1 when even 1.0 is below the
    threshold).  Entry 0 is unused (-1).
    """
    out = np.full(_lib.MAX_BYTES + 1, -1, dtype=np.int16)
    if instance:
        out[1:] = 0 if 1.0 >= thr else -1
        return out
    score, _ = _unit_score_tables(1)
    score = score.reshape(_lib.MAX_BYTES + 1, 257)
    for p in range(1, _lib.MAX_BYTES + 1):
        ok = np.nonzero(score[p, : 8 * p + 1] >= thr)[0]
        # the score falls with h: the confident distances are 0..h_max
        out[p] = int(ok[-1]) if len(ok) else -1
    return out


def _merge_instance(aggregated, unit_type, keys):
    # type: (Dict[int, Dict[str, float]], str, list) -> None
    """An INSTANCE prefix match list into the per-asset scores: every hit scores 1.0 (``usearch/index.py:2010``)."""
    for key in keys:
        aggregated.setdefault(key, {})[unit_type] = 1.0


def _merge_similarity(aggregated, unit_type, keys, scores):
    # type: (Dict[int, Dict[str, float]], str, list, list) -> None
    """A similarity unit's list into the per-asset scores: max per (key, unit_type), first appearance keeps its place (:806)."""
    for key, score in zip(keys, scores):
        slot = aggregated.get(key)
        if slot is None:
            aggregated[key] = {unit_type: score}
        elif score > slot.get(unit_type, 0.0):          # max per (key, unit_type), :806; scores are >= 0.0
            slot[unit_type] = score
        else:
            slot.setdefault(unit_type, 0.0)


def _confidence_total(confident, exp):
    # type: (Dict[str, float], int) -> float
    """Confidence-weighted total of the unit scores at or above the threshold (``usearch/index.py:818-826``): sum(s^exp) / sum(s)."""
    weight_sum = sum(confident.values())
    return sum(s**exp for s in confident.values()) / weight_sum if weight_sum > 0 else 0.0


def _rank_aggregated(aggregated, thr, exp, query_iscc_id, limit):
    # type: (Dict[int, Dict[str, float]], float, int, Optional[str], int) -> list
    """``usearch/index.py:808-839``: threshold, confidence-weighted total, self-exclusion, stable sort, cut: [(key, total, unit_scores)]."""
    scored = []
    for key, unit_scores in aggregated.items():
        confident = {t: s for t, s in unit_scores.items() if s >= thr}
        if not confident:
            continue
        scored.append((key, _confidence_total(confident, exp), unit_scores))
    if query_iscc_id:
        qkey = codec.iscc_id_to_int(query_iscc_id)
        scored = [r for r in scored if r[0] != qkey]
    scored.sort(key=lambda r: r[1], reverse=True)   # stable, as the reference (:836)
    return scored[:limit]


def search_units(engine, tables, prepared, limit, first=None):
    # type: (object, dict, list, int, Optional[int]) -> list
    """
    The per-unit searches of the prepared queries (``usearch/index.py:786-806``: one ``search`` per similarity unit, one prefix
    match per INSTANCE unit) as ONE ``engine.search_many`` call -- one request per (unit type, code length) over all queries --
    merged exactly as the reference merges its per-unit dicts: per query {key: {unit_type: score}}.  Identity matches are few:
    INSTANCE units ask for a short list first (``INSTANCE_FIRST_K`` records per query to select, exchange between shards and
    unpack instead of 4 096); the lists that come back full are asked again, in one more call, up to the cap.  ``limit`` is
    checked only where a similarity unit hands it to the engine.  ``first``: the position of ``prepared[0]`` in a bulk call's
    ``queries``, which a refused INSTANCE list then names.
    """
    groups = {}  # type: Dict[tuple, tuple]          (unit_type, nbytes) -> ([(query, slot)], [body])
    for q, (_, _, units) in enumerate(prepared):
        for j, (unit_type, body) in enumerate(units):
            slots, bodies = groups.setdefault((unit_type, len(body)), ([], []))
            slots.append((q, j))
            bodies.append(body)
    requests = []
    for (unit_type, _), (_, bodies) in groups.items():
        table = tables[unit_type]._table
        words, nbytes = pack_bytes(bodies, table.max_words)
        k, radius = (INSTANCE_FIRST_K, 0) if _is_instance(unit_type) else (_checked_limit(limit), None)
        requests.append((table, words, nbytes, k, radius))
    results = {}  # (query, slot) -> (keys, scores), both lists of plain Python numbers; scores None for an INSTANCE unit
    again_req, again_slots = [], []
    for (slots, _), request, (keys, ham, pbits, cnt) in zip(groups.values(), requests, engine.search_many(requests) if requests else []):
        instance, full = request[4] is not None, []
        for r, slot in enumerate(slots):
            c = int(cnt[r])
            results[slot] = (keys[r, :c].tolist(), None if instance else _unit_scores(ham[r, :c], pbits[r, :c]).tolist())
            if instance and c == INSTANCE_FIRST_K:
                full.append(r)
        if full:
            again_req.append((request[0], request[1][full], request[2][full], MAX_K, 0))
            again_slots.append([slots[r] for r in full])
    for slots, (keys, ham, pbits, cnt) in zip(again_slots, engine.search_many(again_req) if again_req else []):
        for r, slot in enumerate(slots):
            results[slot] = (keys[r, : int(cnt[r])].tolist(), None)
    merged = []
    for q, (_, _, units) in enumerate(prepared):
        aggregated = {}  # type: Dict[int, Dict[str, float]]
        for j, (unit_type, _) in enumerate(units):
            keys, scores = results[(q, j)]
            if scores is None:
                _checked_instance_hits(len(keys), unit_type, None if first is None else first + q)
                _merge_instance(aggregated, unit_type, keys)
            else:
                _merge_similarity(aggregated, unit_type, keys, scores)
        merged.append(aggregated)
    return merged


def match_host(engine, tables, opts, prepared, limit, first=None):
    # type: (object, dict, object, list, int, Optional[int]) -> list
    """The unit matches of the prepared queries, searched and merged by ``search_units`` and ranked: per query [(key, total, unit_scores)]."""
    thr, exp = opts.match_threshold_units, opts.confidence_exponent
    merged = search_units(engine, tables, prepared, limit, first)
    return [_rank_aggregated(aggregated, thr, exp, query_iscc_id, limit) for (_, query_iscc_id, _), aggregated in zip(prepared, merged)]


def match_prepared(engine, tables, opts, prepared, limit):
    # type: (object, dict, object, list, int) -> UnitMatches
    """``UnitMatches`` of prepared queries, ``limit`` within 1..MAX_K: aggregated on the device where the engine has ``match_assets``, else by ``match_host``."""
    types = tuple(dict.fromkeys(unit_type for _, _, units in prepared for unit_type, _ in units))       # in order of first appearance
    nq, nt = len(prepared), max(1, len(types))
    out = UnitMatches(np.zeros((nq, limit), dtype=np.uint64), np.zeros((nq, limit), dtype=np.float64), np.zeros(nq, dtype=np.uint32),
                      types, np.full((nq, limit, nt), 255, dtype=np.uint8), np.zeros((nq, limit, nt), dtype=np.float64))
    _, pow_tab = _unit_score_tables(opts.confidence_exponent)
    device = (hasattr(engine, "match_assets") and pow_tab is not None and len(types) <= _lib.MAX_UNIT_TYPES
              and all(len(units) <= _lib.MAX_ASSET_UNITS for _, _, units in prepared))
    type_of = {t: i for i, t in enumerate(types)}
    step = _lib.ASSET_QUERIES_MAX
    for first in range(0, nq, step):
        part = prepared[first:first + step]
        if device:
            _match_device(engine, tables, opts, part, first, limit, types, out)
            continue
        for q, scored in enumerate(match_host(engine, tables, opts, part, limit, first), first):
            out.counts[q] = len(scored)
            for r, (key, total, unit_scores) in enumerate(scored):
                out.keys[q, r] = key
                out.scores[q, r] = min(1.0, total)
                for t, (unit_type, score) in enumerate(unit_scores.items()):
                    out.type_index[q, r, t] = type_of[unit_type]
                    out.type_scores[q, r, t] = score
    return out


def _match_device(engine, tables, opts, part, first, limit, types, out):
    # the unit records as columns: one join of the zero-padded codes instead of one pack_bytes and record write per unit
    offsets = np.zeros(len(part) + 1, dtype=np.uint32)
    exclude = np.zeros(len(part), dtype=np.uint64)
    has_exclude = np.zeros(len(part), dtype=np.uint8)
    table_of = {t: tables[t]._table.id for t in types}
    type_of = {t: i for i, t in enumerate(types)}
    inst_of = {t: _is_instance(t) for t in types}
    tids, tys, bodies, instances = [], [], [], []   # instances: (query, unit position, unit type) of the INSTANCE units
    u = 0
    for q, (_, query_iscc_id, units) in enumerate(part):
        if query_iscc_id:
            exclude[q] = codec.iscc_id_to_int(query_iscc_id)
            has_exclude[q] = 1
        for unit_type, body in units:
            if not 1 <= len(body) <= _lib.MAX_BYTES:
                raise ValueError(f"code length {len(body)} bytes outside 1..{_lib.MAX_BYTES}")
            tids.append(table_of[unit_type])
            tys.append(type_of[unit_type])
            bodies.append(body)
            if inst_of[unit_type]:
                instances.append((q, u, unit_type))
            u += 1
        offsets[q + 1] = u
    arr = np.zeros(u, dtype=_lib.ASSET_UNIT_DTYPE)
    if u:
        arr["table"] = tids
        arr["type"] = tys
        arr["nbytes"] = [len(b) for b in bodies]
        arr["max_hamming"] = [0 if inst_of[types[t]] else -1 for t in tys]
        arr["words"] = np.frombuffer(b"".join(b.ljust(_lib.MAX_BYTES, b"\0") for b in bodies), dtype=">u8").reshape(u, 4)
    score_tab, pow_tab = _unit_score_tables(opts.confidence_exponent)
    keys, scores, counts, tidx, tsc, unit_counts = engine.match_assets(
        arr, offsets, limit, INSTANCE_FIRST_K, MAX_K, exclude, has_exclude, score_tab, pow_tab,
        opts.match_threshold_units, sys.version_info >= (3, 12), max(1, len(types)))
    for q, u, unit_type in instances:
        _checked_instance_hits(int(unit_counts[u]), unit_type, first + q)
    n = len(part)
    out.keys[first:first + n] = keys
    out.scores[first:first + n] = scores
    out.counts[first:first + n] = counts
    out.type_index[first:first + n] = tidx
    out.type_scores[first:first + n] = tsc
