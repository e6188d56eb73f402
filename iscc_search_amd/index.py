"""
``hip:///`` backend: ``HipIndex``, one named index of the ``HipIndexManager`` (``manager.py``) that implements the
reference's ``IsccIndexProtocol`` (``iscc_search/protocols/index.py:19-174``) over the HIP engine.

Layout mirrors the reference's usearch backend (``iscc_search/indexes/usearch/``):
  ``HipIndexManager``  ~ ``UsearchIndexManager`` (``manager.py:25-335``): named indexes, protocol methods
  ``HipIndex``         ~ ``UsearchIndex`` (``index.py:87-2045``): one index = asset store + one NPHD
                         table per unit type + one simprint table per simprint type
What differs by design: there is no LMDB and no HNSW file -- assets live in a host dict (as in the
reference's ``memory://`` backend, ``memory/index.py``), codes live in HBM, and every similarity
search is the exact GPU scan.  Scoring, thresholds, aggregation, self-exclusion, ordering and error
messages follow ``index.py:735-881`` and ``:1357-1469``.
Here: the index's state, asset store and entry points.  ``unit_match.py``, ``chunk_match.py``, ``pairs.py``, ``snapshot.py``: the rest.
"""

import threading
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np

from iscc_search_amd import chunk_match, codec, snapshot, unit_match
from iscc_search_amd._lib import MAX_K
from iscc_search_amd.nphd import HipNphdIndex
from iscc_search_amd.pairs import DuplicateGroup, DuplicatePair, Hub, IndexMatch, SharedContent, SharedMatch, group_side, hub_side, join_sides, shared_sides
from iscc_search_amd.schema import IsccAddResult, IsccEntry, IsccGlobalMatch, IsccQuery, IsccSearchResult, Status
from iscc_search_amd.simprint import HipSimprintIndex, pack_chunk_pointer, unpack_chunk_pointer
from iscc_search_amd.unit_match import INSTANCE_FIRST_K, UnitMatches, _checked_limit, _is_instance, _unit_map, _unit_max_hamming  # noqa: F401


def __getattr__(name):
    # HipIndexManager, get_index, validate_index_name, INDEX_NAME_RE: importable from here, defined in manager.py (which imports this module)
    from iscc_search_amd import manager

    return getattr(manager, name)


@dataclass
class HipOptions:
    """Knobs with the reference's names and defaults (``iscc_search/options.py:139-164, :95-100``)."""

    match_threshold_units: float = 0.75
    match_threshold_simprints: float = 0.75
    confidence_exponent: int = 4
    oversampling_factor: int = 20
    max_dim: int = 256


def normalize_query(query):
    # type: (IsccQuery) -> IsccQuery
    """Bidirectional units <-> iscc_code normalisation (``iscc_search/indexes/common.py:275-330``)."""
    if query.units and query.iscc_code:
        return query
    if query.units and not query.iscc_code:
        try:
            return query.model_copy(update={"iscc_code": codec.gen_iscc_code(list(query.units), wide=True)})
        except ValueError:
            return query
    if query.iscc_code and not query.units:
        return query.model_copy(update={"units": [str(u) for u in codec.code_units(query.iscc_code)]})
    if query.simprints:
        return query
    raise ValueError("Query must have 'iscc_code', 'units', or 'simprints' for search")


class HipIndex:
    """One named index: host asset store + device tables."""

    def __init__(self, engine, options=None):
        # type: (object, HipOptions | None) -> None
        self._engine = engine
        self._opts = options or HipOptions()
        self._lock = threading.RLock()
        self._realm_id = None  # type: Optional[int]
        self._assets = {}  # type: Dict[int, IsccEntry]          key -> entry (without simprints)
        self._asset_units = {}  # type: Dict[int, Dict[str, bytes]]  key -> {unit_type: body} as indexed
        self._unit_tables = {}  # type: Dict[str, HipNphdIndex]
        self._sp_tables = {}  # type: Dict[str, HipSimprintIndex]
        self._sp_assets = {}  # type: Dict[str, Dict[bytes, list]]   sp_type -> body -> [(sp_bytes, chunk_ptr)]
        self._suspect = set()  # asset keys whose last device update failed half-way: their next add cleans up first
        self.dirty = False

    # -- helpers ---------------------------------------------------------------------------------
    def __len__(self):
        return len(self._assets)

    def _unit_table(self, unit_type):
        t = self._unit_tables.get(unit_type)
        if t is None:
            t = self._unit_tables[unit_type] = HipNphdIndex(self._engine, max_dim=self._opts.max_dim)
        return t

    def _sp_table(self, sp_type, ndim):
        t = self._sp_tables.get(sp_type)
        if t is None:
            t = self._sp_tables[sp_type] = HipSimprintIndex(self._engine, ndim=ndim, oversampling_factor=self._opts.oversampling_factor)
            self._sp_assets[sp_type] = {}
        return t

    @staticmethod
    def _fingerprint(sp_list):
        return tuple(sorted((codec.decode_base64(sp.simprint), sp.offset, sp.size) for sp in sp_list))

    def _fingerprint_of(self, sp_type, body):
        pairs = self._sp_assets.get(sp_type, {}).get(body)
        if pairs is None:
            return None
        return tuple(sorted((sp, *unpack_chunk_pointer(ptr)[1:]) for sp, ptr in pairs))

    def _source_metadata(self, key):
        """(source, metadata) of the asset stored under ``key``, as a match reports them."""
        asset = self._assets.get(key)
        if asset is not None and asset.metadata:
            return asset.metadata.get("source"), asset.metadata
        return None, None

    def _global_match(self, key, score, types):
        source, metadata = self._source_metadata(key)
        return IsccGlobalMatch(iscc_id=codec.iscc_id_from_int(key, self._realm_id or 0), score=score, types=types, source=source, metadata=metadata)

    # -- add ---------------------------------------------------------------------------------------
    def add_assets(self, assets):
        # type: (List[IsccEntry]) -> List[IsccAddResult]
        """Semantics of ``usearch/index.py:194-537`` (status, batch dedup keep-last, remove-before-add)."""
        if not assets:
            return []
        with self._lock:
            if self._realm_id is None:
                if assets[0].iscc_id is None:
                    raise ValueError("Asset must have iscc_id field when adding to index")
                self._realm_id = codec.validate_iscc_id(assets[0].iscc_id).stype
            results = []
            unit_batches = {}  # type: Dict[str, Dict[int, bytes]]
            updated_keys = set()
            sp_batches = {}  # type: Dict[str, tuple]
            sp_deleted = {}  # type: Dict[str, list]
            last_occurrence = {a.iscc_id: i for i, a in enumerate(assets)}
            batch_seen = set()
            staged = []
            for i, asset in enumerate(assets):
                if asset.iscc_id is None:
                    raise ValueError("Asset must have iscc_id field when adding to index")
                id_obj = codec.validate_iscc_id(asset.iscc_id)
                if id_obj.stype != self._realm_id:
                    raise ValueError(
                        f"Realm ID mismatch: index has realm={self._realm_id}, but asset '{asset.iscc_id}' "
                        f"has realm={id_obj.stype}. All assets in an index must have the same realm ID."
                    )
                key = int.from_bytes(id_obj.body, "big")
                existing = self._assets.get(key)
                status = Status.updated if (existing is not None or key in batch_seen) else Status.created
                batch_seen.add(key)
                results.append(IsccAddResult(iscc_id=asset.iscc_id, status=status))
                if i != last_occurrence[asset.iscc_id]:
                    continue
                stored = asset.model_copy(update={"simprints": None})
                fingerprints = {t: self._fingerprint(lst) for t, lst in (asset.simprints or {}).items()}
                # idempotent re-add: nothing to do when entry and simprints are already indexed identically
                if existing is not None and key not in self._suspect and existing == stored and all(
                    self._fingerprint_of(t, id_obj.body) == fp for t, fp in fingerprints.items()
                ):
                    continue
                if existing is not None:
                    updated_keys.add(key)
                # validate / decode units before touching any state
                unit_map = _unit_map(asset.units)
                sp_decoded = {}
                for sp_type, sp_list in (asset.simprints or {}).items():
                    if not sp_list:
                        continue           # a type listed without chunks indexes nothing
                    sp_decoded[sp_type] = [(codec.decode_base64(sp.simprint), pack_chunk_pointer(id_obj.body, sp.offset, sp.size)) for sp in sp_list]
                staged.append((key, id_obj.body, stored, unit_map, sp_decoded))

            # host state is published first (searches read it without the lock) and rolled back if a device call fails,
            # so that a failed batch can simply be retried (the reference keeps its no-op gate honest the same way:
            # _nphd_units_present / _simprints_present_in_derived, usearch/index.py:539-679)
            undo = []                              # (key, body, old entry, old unit map, {sp_type: old pairs})
            dropped = {}  # type: Dict[str, list]  unit_type -> keys whose update no longer carries that type
            for key, body, stored, unit_map, sp_decoded in staged:
                old_units = self._asset_units.get(key, {})
                undo.append((key, body, self._assets.get(key), self._asset_units.get(key),
                             {t: self._sp_assets.get(t, {}).get(body) for t in sp_decoded}))
                self._assets[key] = stored
                for unit_type, ubody in unit_map.items():
                    unit_batches.setdefault(unit_type, {})[key] = ubody
                # an INSTANCE unit the new version no longer carries must leave its table: left behind it would keep
                # prefix-matching as a 1.0 identity hit (usearch/index.py:338-348).  Similarity units the update drops
                # stay, as in the reference, which removes only from the indexes of the types the NEW version carries (:432-441)
                for unit_type in old_units:
                    if unit_type not in unit_map and _is_instance(unit_type):
                        dropped.setdefault(unit_type, []).append(key)
                self._asset_units[key] = unit_map
                for sp_type, pairs in sp_decoded.items():
                    self._sp_table(sp_type, len(pairs[0][0]) * 8)
                    old = self._sp_assets[sp_type].pop(body, None)
                    if old is not None:
                        sp_deleted.setdefault(sp_type, []).extend(ptr for _, ptr in old)
                    if key in self._suspect:       # rows of a half-applied earlier attempt may sit under the NEW pointers
                        sp_deleted.setdefault(sp_type, []).extend(ptr for _, ptr in pairs)
                    self._sp_assets[sp_type][body] = pairs
                    keys_b, vecs_b = sp_batches.setdefault(sp_type, ([], []))
                    for sp_bytes, ptr in pairs:
                        keys_b.append(ptr)
                        vecs_b.append(np.frombuffer(sp_bytes, dtype=np.uint8))

            # device side: remove-before-add for updated assets, then one batched add per table
            try:
                for unit_type, keys_gone in dropped.items():
                    self._unit_tables[unit_type].remove(keys_gone)
                for unit_type, items in unit_batches.items():
                    table = self._unit_table(unit_type)
                    to_remove = [k for k in items if k in updated_keys or k in self._suspect]
                    if to_remove:
                        table.remove(to_remove)
                    table.add(list(items.keys()), list(items.values()))
                for sp_type, (ckeys, vecs) in sp_batches.items():
                    table = self._sp_tables[sp_type]
                    if sp_type in sp_deleted:
                        table.remove(sp_deleted[sp_type])
                    table.add_raw(ckeys, vecs)
            except Exception:
                for key, body, old_entry, old_units, old_sp in undo:
                    if old_entry is None:
                        self._assets.pop(key, None)
                        self._asset_units.pop(key, None)
                    else:
                        self._assets[key] = old_entry
                        self._asset_units[key] = old_units if old_units is not None else {}
                    for sp_type, pairs in old_sp.items():
                        if pairs is None:
                            self._sp_assets.get(sp_type, {}).pop(body, None)
                        else:
                            self._sp_assets[sp_type][body] = pairs
                    self._suspect.add(key)
                raise
            for key, *_ in staged:
                self._suspect.discard(key)
            if staged:
                self.dirty = True
            return results

    # -- get ---------------------------------------------------------------------------------------
    def get_asset(self, iscc_id):
        # type: (str) -> IsccEntry
        if self._realm_id is not None:
            codec.validate_iscc_id(iscc_id, expected_realm=self._realm_id)
        key = codec.iscc_id_to_int(iscc_id)
        with self._lock:
            asset = self._assets.get(key)
        if asset is None:
            raise FileNotFoundError(f"Asset '{iscc_id}' not found in index")
        return asset

    # -- search ------------------------------------------------------------------------------------
    def _prepare(self, query):
        # type: (IsccQuery) -> tuple
        """A query as the searches see it: (normalised query, query iscc_id or None, [(unit_type, body)] of the indexed unit types in query order)."""
        query_iscc_id = None
        if query.iscc_id:
            query_iscc_id = query.iscc_id
            asset = self.get_asset(query.iscc_id)
            query = IsccQuery(iscc_code=asset.iscc_code, units=asset.units, simprints=None)
        query = normalize_query(query)
        units = []
        for unit_str in query.units or []:
            unit = codec.parse(unit_str)
            if unit.unit_type in self._unit_tables:
                units.append((unit.unit_type, unit.body))
        return query, query_iscc_id, units

    def search_assets(self, query, limit=100, exact=False):
        # type: (IsccQuery, int, bool) -> IsccSearchResult
        """``exact=True`` matches simprints by collision only (``usearch/index.py:735-778, :1261-1304``)."""
        prepared = self._prepare(query)
        query, query_iscc_id, _ = prepared
        # No index-wide lock here: the engine serialises (and combines) concurrent searches itself, the host
        # dicts are only read, and writers (add_assets) publish whole entries -- as with the reference, a search
        # that overlaps an add may or may not see that batch.
        chunk_matches = []
        if self._sp_tables and query.simprints:
            chunk_matches = chunk_match.search_simprints(self, query, limit, exact=exact)
        matches = []
        if query.units:
            scored = unit_match.match_host(self._engine, self._unit_tables, self._opts, [prepared], limit)[0]
            matches = [self._global_match(key, min(1.0, total), unit_scores) for key, total, unit_scores in scored]
        if query_iscc_id:
            chunk_matches = [m for m in chunk_matches if m.iscc_id != query_iscc_id]
        return IsccSearchResult(query=query, global_matches=matches, chunk_matches=chunk_matches)

    # -- pairs -------------------------------------------------------------------------------------
    def _join_side(self, unit_types=None):
        # type: (Optional[List[str]]) -> tuple
        """This index as one side of a join (``pairs.join_sides``), its tables restricted to ``unit_types``, and its realm."""
        with self._lock:
            tables = {t: idx for t, idx in self._unit_tables.items() if unit_types is None or t in unit_types}
            return (tables, dict(self._asset_units)), self._realm_id or 0

    def _shared_side(self, simprint_types=None):
        # type: (Optional[List[str]]) -> tuple
        """This index as one side of a shared-content join (``pairs.shared_sides``): its simprint tables restricted to
        ``simprint_types`` with the asset bodies each holds, and its realm."""
        with self._lock:
            tables = {t: idx for t, idx in self._sp_tables.items() if simprint_types is None or t in simprint_types}
            return (tables, {t: list(self._sp_assets.get(t, {})) for t in tables}), self._realm_id or 0

    def find_duplicates(self, min_score=None, unit_types=None, max_pairs=1_000_000, max_degree=None):
        # type: (Optional[float], Optional[List[str]], int, Optional[int]) -> List[DuplicatePair]
        """
        Every pair of assets {a, b} that ``search_assets(IsccQuery(iscc_id=a), limit=len(index))`` would list as b's match,
        with that score and the confident part of b's unit scores -- found by ONE self-join per unit table on the device
        (``HipTable.join_within``) instead of a search per asset.  Units are compared as they were indexed.  Pairs are
        aggregated over the unit types both assets carry, kept when one unit is confident (and the score is >= ``min_score``,
        if given), and ordered by score descending, then (key_a, key_b).  ``unit_types`` restricts the unit tables joined.
        More than ``max_pairs`` unit pairs in one table raise ValueError.  ``max_degree`` keeps HUBS out: an asset whose unit of a type
        has more than ``max_degree`` near-duplicates among the assets that carry the type (``find_hubs`` lists them: a black frame,
        silence, 10 000 re-uploads of one file -- h * (h - 1) / 2 pairs that would exceed ``max_pairs`` and hide every other pair)
        takes no part in THAT table's join; it still pairs through its other unit types.  The degree is counted once, in the full
        table, on the device.  None: no hub is left out and nothing is counted.
        """
        if max_degree is not None and max_degree < 0:
            raise ValueError(f"max_degree must be >= 0, got {max_degree}")
        side, realm = self._join_side(unit_types)
        return [DuplicatePair(codec.iscc_id_from_int(a, realm), codec.iscc_id_from_int(b, realm), score, types)
                for a, b, score, types in join_sides("find_duplicates", side, side, self._opts, min_score, max_pairs, max_degree)]

    def find_duplicate_groups(self, unit_types=None, threshold=None, min_size=2, max_degree=None):
        # type: (Optional[List[str]], Optional[float], int, Optional[int]) -> List[DuplicateGroup]
        """
        The groups of near-duplicate assets: the connected components of the graph whose vertices are this index's assets and
        whose edges are exactly the pairs ``find_duplicates(unit_types=unit_types)`` lists on an index whose
        ``match_threshold_units`` is ``threshold`` (default: this index's own; outside (0, 1]: ValueError) -- one confident unit
        of a type BOTH assets carry as indexed.  Found without the pairs: every unit table's self-join unites the two assets of
        a pair in a union-find array on the device (``HipTable.join_components``), 4 bytes per asset and per row however many
        pairs there are, so 10 000 copies of one file are one group and not 5 * 10^7 pairs over ``max_pairs``.  Groups of at least
        ``min_size`` assets, by size descending, then by smallest key; ``iscc_ids`` ascending by key.  There is no
        ``min_score``: an aggregated score needs every table's unit scores per pair, which is what ``find_duplicates`` computes.
        ``max_degree``: as for ``find_duplicates`` -- the hubs of a table link nothing in it, so the groups are the components of
        ``find_duplicates(max_degree=max_degree)`` and nothing chains through a hub.
        """
        threshold = self._opts.match_threshold_units if threshold is None else float(threshold)
        if not 0.0 < threshold <= 1.0:
            raise ValueError(f"threshold must be in (0, 1], got {threshold}")
        if max_degree is not None and max_degree < 0:
            raise ValueError(f"max_degree must be >= 0, got {max_degree}")
        side, realm = self._join_side(unit_types)
        return [DuplicateGroup([codec.iscc_id_from_int(k, realm) for k in group.tolist()], len(group))
                for group in group_side("find_duplicate_groups", side, threshold, min_size, max_degree)]

    def find_hubs(self, min_degree=1, unit_types=None, threshold=None):
        # type: (int, Optional[List[str]], Optional[float]) -> List[Hub]
        """
        Which assets are the hubs, and how many near-duplicates each asset has: every (asset, unit type) whose unit has at least
        ``min_degree`` other assets within the threshold among the assets that carry the type as indexed -- the number of pairs
        ``find_duplicates`` would owe to that unit alone, a registry's "most copied" list -- ordered by (-degree, iscc_id, unit_type).
        Counted per row on the device (``HipTable.join_degrees``), 4 bytes per asset and per row however many pairs there are: no pair is
        materialised.  ``threshold`` defaults to ``match_threshold_units`` (outside (0, 1]: ValueError); ``unit_types`` restricts the
        unit tables counted.  ``max_degree`` of ``find_duplicates`` / ``find_duplicate_groups`` leaves out what this lists above it.
        """
        threshold = self._opts.match_threshold_units if threshold is None else float(threshold)
        if not 0.0 < threshold <= 1.0:
            raise ValueError(f"threshold must be in (0, 1], got {threshold}")
        side, realm = self._join_side(unit_types)
        return [Hub(codec.iscc_id_from_int(key, realm), unit_type, degree)
                for key, unit_type, degree in hub_side("find_hubs", side, threshold, min_degree)]

    def find_matches(self, other, min_score=None, unit_types=None, max_pairs=1_000_000):
        # type: (HipIndex, Optional[float], Optional[List[str]], int) -> List[IndexMatch]
        """
        Every pair (asset a of this index, asset b of ``other``) that ``other.search_assets(IsccQuery(units=<a's units as
        indexed>), limit=len(other))`` would list as b, with that score and the confident part of that match's unit scores in
        a's unit order -- found by ONE cross join per unit type both indexes have a table for (``HipTable.join_between``)
        instead of a search per asset.  The other index's threshold and exponent score the pairs, as its ``search_assets`` would.  An asset present in both
        indexes pairs with itself.  Kept, filtered (``min_score``, ``unit_types``) and capped (``max_pairs`` unit pairs per
        table, else ValueError) as ``find_duplicates`` does; ordered by score descending, then (key_a, key_b).  Both indexes
        must live on one engine.
        """
        if other is self:
            raise ValueError("find_matches compares two indexes: find_duplicates lists the pairs within one")
        if other._engine is not self._engine:
            raise ValueError("find_matches needs both indexes on one engine: their tables must share the device's memory")
        side_a, realm_a = self._join_side(unit_types)
        side_b, realm_b = other._join_side()
        return [IndexMatch(codec.iscc_id_from_int(a, realm_a), codec.iscc_id_from_int(b, realm_b), score, types)
                for a, b, score, types in join_sides("find_matches", side_a, side_b, other._opts, min_score, max_pairs)]

    def find_shared_content(self, min_chunks=1, min_coverage=None, simprint_types=None, threshold=None, max_doc_freq=100, max_pairs=1_000_000,
                            segments=False, min_segment=1, max_gap=0):
        # type: (int, Optional[float], Optional[List[str]], Optional[float], int, int, bool, int, int) -> List[SharedContent]
        """
        Every pair of assets {a, b} that share content: in some simprint type a chunk of a and a chunk of b whose similarity passes
        ``threshold`` (default: ``match_threshold_simprints``) -- a clip inside a longer video, a quoted passage, a sampled loop.
        Found by ONE self-join per simprint table, aggregated on the device (``HipSimprintIndex.shared``), instead of a
        ``search_assets`` by simprints per asset and its top-``limit`` cut.  Chunks of one asset never pair with each other, and a chunk
        whose simprint more than ``max_doc_freq`` assets hold (black frames, licence text; 0: no cut) pairs with nothing, though it
        still counts among its asset's chunks.  Per type ``SharedChunks`` says how many chunks of each asset found a match and
        ``coverage_x``, the mean over x's chunks of the best similarity found in the other asset (0 where none): what
        ``search_raw`` by x's simprints scores the other asset with under constant IDF.  The type's score is the larger coverage,
        ``score`` the mean over the types in which the pair matches.  Kept when ``max(matched_a, matched_b) >= min_chunks`` in some
        type (and ``score >= min_coverage``, if given); ordered by score descending, then (key_a, key_b).  ``simprint_types``
        restricts the tables joined.  More than ``max_pairs`` matching chunk pairs in one table raise ValueError.

        ``segments=True`` also says WHERE, from the same join (``HipSimprintIndex.shared``): every ``SharedChunks`` carries
        ``segments``, a list of ``SharedSegment`` -- "chunks 40..95 of a are chunks 3..58 of b", with the byte range on either side,
        the number of matched chunk pairs and their mean similarity.  A segment is a run of consecutive chunks of a (ranked by offset
        within the asset, stop chunks keeping their place) that match consecutive chunks of b.  Runs of one pair in one alignment that
        lie at most ``max_gap`` chunks apart are merged (a re-encoded frame, a stop chunk inside a clip); merged runs of fewer than
        ``min_segment`` matched chunks are dropped.  Ordered by (offset_a, offset_b).  Neither changes which pairs are listed.
        """
        threshold = self._opts.match_threshold_simprints if threshold is None else float(threshold)
        side, realm = self._shared_side(simprint_types)
        return [SharedContent(codec.iscc_id_from_int(a, realm), codec.iscc_id_from_int(b, realm), score, types)
                for a, b, score, types in shared_sides("find_shared_content", side, side, threshold, max_doc_freq, max_pairs, min_chunks, min_coverage,
                                                       True, bool(segments), int(min_segment), int(max_gap))]

    def find_shared_matches(self, other, min_chunks=1, min_coverage=None, simprint_types=None, threshold=None, max_doc_freq=100,
                            max_pairs=1_000_000, include_same_id=False, segments=False, min_segment=1, max_gap=0):
        # type: (HipIndex, int, Optional[float], Optional[List[str]], Optional[float], int, int, bool, bool, int, int) -> List[SharedMatch]
        """
        Every pair (asset a of this index, asset b of ``other``) that share content, as ``find_shared_content`` defines it within one
        index: which assets of this catalogue contain a clip, a quoted passage or a sampled loop of an asset of that registry.  Found
        by ONE cross join per simprint type both indexes have a table for, aggregated on the device
        (``HipSimprintIndex.shared``), instead of a simprint search per asset or a self-join of a copy of both.
        ``threshold`` defaults to the OTHER index's ``match_threshold_simprints`` (as ``find_matches`` scores with the other index's
        options): ``coverage_a`` is what ``other``'s ``search_raw`` by a's simprints scores b with under constant IDF.  A chunk whose
        simprint more than ``max_doc_freq`` assets of ITS OWN index hold pairs with nothing (0: no cut) but still counts among its
        asset's chunks.  An asset both indexes hold (one ISCC-ID body) pairs with itself only with ``include_same_id``.  Score,
        ``min_chunks``, ``min_coverage``, ``simprint_types``, ``max_pairs`` and the order (score descending, then (key_a, key_b)) as
        for ``find_shared_content``; each side's ISCC-IDs carry its own realm.  Both indexes must live on one engine.

        ``segments=True`` also says WHERE, from the same cross join (``HipSimprintIndex.shared``): every
        ``SharedChunks`` carries ``segments``, a list of ``SharedSegment`` -- "chunks 40..95 of a are chunks 3..58 of b", with the byte
        range on either side -- as ``find_shared_content`` defines them, a being this index's asset and a chunk's rank counted among
        its asset's chunks in its own index.  ``min_segment`` and ``max_gap`` as there.  Neither changes which pairs are listed.
        """
        if other is self:
            raise ValueError("find_shared_matches compares two indexes: find_shared_content lists the pairs within one")
        if other._engine is not self._engine:
            raise ValueError("find_shared_matches needs both indexes on one engine: their tables must share the device's memory")
        threshold = other._opts.match_threshold_simprints if threshold is None else float(threshold)
        side_a, realm_a = self._shared_side(simprint_types)
        side_b, realm_b = other._shared_side(simprint_types)
        return [SharedMatch(codec.iscc_id_from_int(a, realm_a), codec.iscc_id_from_int(b, realm_b), score, types)
                for a, b, score, types in shared_sides("find_shared_matches", side_a, side_b, threshold, max_doc_freq, max_pairs, min_chunks, min_coverage,
                                                       not include_same_id, bool(segments), int(min_segment), int(max_gap))]

    # -- bulk search -------------------------------------------------------------------------------
    def _prepare_many(self, queries):
        # type: (List[IsccQuery]) -> list
        """
        Every query as ``search_assets`` sees it (``_prepare``), its simprints decoded once to validate them -- or the exception
        ``search_assets`` would raise, naming the query's index in ``queries``.
        """
        prepared = []
        for i, query in enumerate(queries):
            try:
                prepared.append(self._prepare(query))
                query = prepared[-1][0]
                if self._sp_tables and query.simprints:
                    for simprint_objs in query.simprints.values():
                        for sp in simprint_objs:
                            codec.decode_base64(chunk_match._sp_string(sp))
            except (ValueError, FileNotFoundError) as e:
                raise type(e)(f"queries[{i}]: {e}") from e
        return prepared

    def match_units_many(self, queries, limit=100):
        # type: (List[IsccQuery], int) -> UnitMatches
        """
        The unit part of ``search_assets`` for many queries at once, as NumPy arrays (no pydantic objects): per query its
        assets, scores and per-unit-type scores in ``search_assets`` order.  On a single-GPU engine every unit type (and code
        length) is ONE batched search over all queries and the per-asset aggregation runs on the device
        (``isccsearch_match_assets``); other engines run one batched ``search_many`` request per unit type and the
        aggregation of ``search_assets`` on the host.  Simprints are not looked at.
        """
        if not 1 <= limit <= MAX_K:
            _checked_limit(limit)
            raise ValueError(f"limit {limit} must be >= 1")
        return unit_match.match_prepared(self._engine, self._unit_tables, self._opts, self._prepare_many(queries), limit)

    def search_assets_many(self, queries, limit=100, exact=False):
        # type: (List[IsccQuery], int, bool) -> List[IsccSearchResult]
        """
        ``search_assets`` for many queries: result i equals ``search_assets(queries[i], limit, exact)`` on the same index
        state.  Every query is validated first; one that ``search_assets`` would reject fails the whole call, before anything
        is searched, with the same exception naming its index in ``queries``.  The unit part runs as ``match_units_many``
        (batches of up to 1 024 queries).  The ``chunk_matches`` of queries with simprints: per simprint type ONE
        ``search_raw_many`` over every query that carries it (on a single-GPU engine one library call, scored per query on the
        device), then the ranking of ``search_assets`` per query.  With ``exact=True`` the collision search is batched the same
        way: per simprint type ONE ``search_exact_many`` (on a single-GPU engine one library search per round of 8 192 simprints).
        """
        if not 1 <= limit <= MAX_K:
            # outside the engine's range search_assets itself decides (its limit checks depend on the query's units)
            out = []
            for i, query in enumerate(queries):
                try:
                    out.append(self.search_assets(query, limit, exact=exact))
                except (ValueError, FileNotFoundError) as e:
                    raise type(e)(f"queries[{i}]: {e}") from e
            return out
        prepared = self._prepare_many(queries)
        unit_idx = [i for i, (query, _, _) in enumerate(prepared) if query.units]
        m = unit_match.match_prepared(self._engine, self._unit_tables, self._opts, [prepared[i] for i in unit_idx], limit) if unit_idx else None
        row_of = {i: r for r, i in enumerate(unit_idx)}
        sp_raw = chunk_match.search_simprints_many(self, prepared, limit, exact=exact)
        results = []
        for i, (query, query_iscc_id, _) in enumerate(prepared):
            chunk_matches = []
            if self._sp_tables and query.simprints:
                chunk_matches = chunk_match.rank_simprint_matches(self, sp_raw.get(i, []), limit)
            matches = []
            r = row_of.get(i)
            if r is not None:
                c = int(m.counts[r])
                rows = zip(m.keys[r, :c].tolist(), m.scores[r, :c].tolist(), m.type_index[r, :c].tolist(), m.type_scores[r, :c].tolist())
                matches = [self._global_match(key, score, {m.types[t]: s for t, s in zip(ti, ts) if t != 255}) for key, score, ti, ts in rows]
            if query_iscc_id:
                chunk_matches = [cm for cm in chunk_matches if cm.iscc_id != query_iscc_id]
            results.append(IsccSearchResult(query=query, global_matches=matches, chunk_matches=chunk_matches))
        return results

    # -- snapshot ----------------------------------------------------------------------------------
    def save(self, path):
        # type: (str) -> None
        snapshot.save(self, path)

    @classmethod
    def load(cls, engine, path, options=None):
        # type: (object, str, HipOptions | None) -> HipIndex
        return snapshot.load(cls, engine, path, options)

    def close(self):
        # type: () -> None
        with self._lock:
            for t in list(self._unit_tables.values()):
                t.close()
            for t in list(self._sp_tables.values()):
                t.close()
            self._unit_tables.clear()
            self._sp_tables.clear()
