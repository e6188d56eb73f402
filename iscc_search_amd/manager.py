"""
``HipIndexManager``: the reference's ``IsccIndexProtocol`` (``iscc_search/protocols/index.py:19-174``) over named
``HipIndex`` instances on one engine -- what ``UsearchIndexManager`` (``iscc_search/indexes/usearch/manager.py:25-335``) is to
the usearch backend -- and ``get_index``, the factory of the ``hip`` URI scheme.
"""

import functools
import json
import os
import re
import shutil
import threading
from typing import Dict, List, Optional
from urllib.parse import parse_qs, urlparse

from iscc_search_amd.index import HipIndex, HipOptions
from iscc_search_amd.pairs import DuplicateGroup, DuplicatePair, Hub, IndexMatch, SharedContent, SharedMatch
from iscc_search_amd.schema import IsccAddResult, IsccEntry, IsccIndex, IsccQuery, IsccSearchResult

INDEX_NAME_RE = re.compile(r"^[a-z][a-z0-9]*$")


def validate_index_name(name):
    # type: (str) -> None
    if not isinstance(name, str) or not INDEX_NAME_RE.match(name) or len(name) > 32:
        raise ValueError(
            f"Invalid index name: '{name}'. Must match pattern ^[a-z][a-z0-9]*$ "
            f"(start with lowercase letter, followed by lowercase letters/digits only)"
        )


def _protocol_call(method):
    """
    Every protocol method of ``HipIndexManager`` runs in one of three modes:
      * a sharded index opened by ONE process: the host logic runs here, alone, over the leader front's engine, which broadcasts
        every TABLE operation to the shard workers in its own order and combines the searches of concurrent callers
        (shard_front.py) -- no manager-wide lock, as on one GPU; a front that is down fails every call, also those that need no table;
      * a sharded index under a launcher (SPMD) takes `_spmd` around the WHOLE method: flush, the lazy snapshot load in
        `_index` and delete_index reach collectives just as add / search do;
      * one GPU: no extra lock, searches of concurrent callers are combined by the engine.
    """
    @functools.wraps(method)
    def guarded(self, *args, **kwargs):
        if self._leads():
            self._get_engine().check()
        elif self._spmd is not None:
            with self._spmd:
                return method(self, *args, **kwargs)
        return method(self, *args, **kwargs)

    return guarded


class HipIndexManager:
    """
    Protocol-conformant manager of named ``hip:///`` indexes on one GPU.

    The engine (library load, GPU context, stream) is created lazily on first use and released by
    ``close()``, which is idempotent (``protocols/index.py:162-172``).  Thread-safe: FastAPI calls
    the sync protocol methods from a thread pool (``docs/explanation/architecture.md:120-126``).

    ``engine`` is a seam for sharing one ``HipEngine`` between managers and for the CPU test tier (which injects
    an oracle-backed stand-in from ``tests/``); left ``None`` -- as ``get_index("hip:///")`` leaves it -- the manager
    creates a ``HipEngine`` and raises if the HIP library or the GPU is missing.  There is no CPU fallback.
    """

    def __init__(self, uri="hip:///", engine=None, options=None, shard_engine_factory=None):
        # type: (str, object | None, HipOptions | None, str | None) -> None
        parsed = urlparse(uri)
        if parsed.scheme != "hip":
            raise ValueError(f"HipIndexManager requires a hip:// URI, got '{uri}'")
        qs = parse_qs(parsed.query)
        self.device_id = int(qs.get("device", ["0"])[0])
        # hip:///?devices=N  -> the index row-sharded over N GPUs, one process per GPU (iscc_search_amd/sharded_engine.py).
        #   * constructed where NO torch.distributed group exists (the reference's server / CLI: one process): this process
        #     becomes the leader, starts the N - 1 other ranks itself and broadcasts every call to them (shard_front.py);
        #     `backend=gloo` / `same_gpu=1` in the query select the rehearsal transport (CPU tests, ranks sharing one GPU)
        #   * constructed on every rank of a running group of N (torch.distributed.run): SPMD, every rank makes the same calls
        self.devices = int(qs.get("devices", ["1"])[0])
        if self.devices < 1:
            raise ValueError(f"devices must be >= 1, got {self.devices}")
        self._uri = uri
        self._shard_backend = qs.get("backend", ["nccl"])[0]
        self._shard_same_gpu = qs.get("same_gpu", ["0"])[0] == "1"
        self._shard_engine_factory = shard_engine_factory
        self._leading = False          # this manager drives a leader front (shard_front.LeaderEngine) as its engine
        # hip:///            -> volatile (like memory://)
        # hip:///abs/path    -> snapshots under that directory: loaded lazily, written by flush()/close()
        self.base_path = parsed.path if parsed.path not in ("", "/") else None
        self._engine = engine
        self._owns_engine = engine is None
        self._opts = options or HipOptions()
        self._indexes = {}  # type: Dict[str, HipIndex]
        self._on_disk = set()
        self._lock = threading.RLock()
        # sharded mode is SPMD: every rank must issue the same calls in the same order (each holds collectives), so calls that
        # reach the engine are serialised per manager; a single-GPU manager lets them run concurrently (the engine combines them)
        self._spmd = threading.RLock() if self.devices > 1 else None
        self._closed = False
        if self.base_path:
            os.makedirs(self.base_path, exist_ok=True)
            for name in sorted(os.listdir(self.base_path)):
                if INDEX_NAME_RE.match(name) and os.path.exists(os.path.join(self.base_path, name, "index.json")):
                    self._on_disk.add(name)

    def _leads(self):
        """
        Whether this manager is the ONE calling process of a sharded index (``shard_front.LeaderEngine``: it starts the other
        ranks itself) -- as opposed to unsharded, an injected engine, or one rank of a launcher's SPMD group.
        """
        if self.devices == 1 or (self._engine is not None and not self._leading):
            return False
        if self._leading:
            return True
        import torch.distributed as dist

        from iscc_search_amd import shard_front

        # a process group that exists and is NOT a leader front's belongs to a launcher: SPMD
        return not dist.is_initialized() or shard_front.leads_this_process()

    @property
    def _leader(self):
        """The leader front this manager drives (None before its first use and in every other mode)."""
        return self._engine if self._leading else None

    def _get_engine(self):
        if self._engine is None:
            from iscc_search_amd.engine import HipEngine   # raises loudly without library / GPU

            if self.devices > 1 and self._leads():
                from iscc_search_amd.shard_front import leader_engine

                with self._lock:
                    if self._engine is None:
                        self._engine = leader_engine(self.devices, backend=self._shard_backend, engine_factory=self._shard_engine_factory,
                                                     same_gpu=self._shard_same_gpu)
                        self._leading = True
            elif self.devices > 1:
                import torch.distributed as dist

                from iscc_search_amd.sharded_engine import ShardedEngine

                if not dist.is_initialized() or dist.get_world_size() != self.devices:
                    raise ValueError(
                        f"hip:///?devices={self.devices}: this rank's engine needs the process group of {self.devices} ranks (one per GPU); "
                        f"a single calling process gets it from shard_front.LeaderEngine, a launcher from torch.distributed.run"
                    )
                local = int(os.environ.get("LOCAL_RANK", dist.get_rank()))
                self._engine = ShardedEngine(HipEngine(local), device=f"cuda:{local}")
            else:
                self._engine = HipEngine(self.device_id)
        return self._engine

    def _index(self, name):
        # type: (str) -> HipIndex
        idx = self._indexes.get(name)
        if idx is None and name in self._on_disk:
            idx = self._indexes[name] = HipIndex.load(self._get_engine(), os.path.join(self.base_path, name), self._opts)
        if idx is None:
            raise FileNotFoundError(f"Index '{name}' not found")
        return idx

    def _locked_index(self, name):
        """``_index`` under the manager's lock; the call on the index that follows runs outside it."""
        with self._lock:
            return self._index(name)

    def _asset_count(self, name):
        if name in self._indexes:
            return len(self._indexes[name])
        with open(os.path.join(self.base_path, name, "index.json")) as f:
            return json.load(f).get("assets", 0)

    def _known(self, name):
        if name not in self._indexes and name not in self._on_disk:
            raise FileNotFoundError(f"Index '{name}' not found")

    def _refuse_sharded(self, method):
        if self.devices > 1:
            raise NotImplementedError(f"{method} is not available on a sharded index (devices={self.devices}): pairs across shards need the rows "
                                      f"exchanged between the GPUs")

    @_protocol_call
    def flush(self):
        # type: () -> None
        """Write every modified index to its snapshot directory (no-op for volatile managers)."""
        self._flush()

    def _flush(self):
        """``flush`` without its protocol mode: ``_close`` flushes inside its own."""
        if not self.base_path:
            return
        with self._lock:
            for name, idx in self._indexes.items():
                if idx.dirty or name not in self._on_disk:
                    idx.save(os.path.join(self.base_path, name))
                    self._on_disk.add(name)

    # -- protocol ----------------------------------------------------------------------------------
    @_protocol_call
    def list_indexes(self):
        # type: () -> List[IsccIndex]
        with self._lock:
            return [IsccIndex(name=n, assets=self._asset_count(n), size=0) for n in sorted(set(self._indexes) | self._on_disk)]

    @_protocol_call
    def create_index(self, index):
        # type: (IsccIndex) -> IsccIndex
        validate_index_name(index.name)
        with self._lock:
            if index.name in self._indexes or index.name in self._on_disk:
                raise FileExistsError(f"Index '{index.name}' already exists")
            self._indexes[index.name] = HipIndex(self._get_engine(), self._opts)
        return IsccIndex(name=index.name, assets=0, size=0)

    @_protocol_call
    def get_index(self, name):
        # type: (str) -> IsccIndex
        with self._lock:
            self._known(name)
            return IsccIndex(name=name, assets=self._asset_count(name), size=0)

    @_protocol_call
    def delete_index(self, name):
        # type: (str) -> None
        with self._lock:
            self._known(name)
            if name in self._indexes:
                self._indexes.pop(name).close()
            if name in self._on_disk:
                if getattr(self._engine, "rank", 0) == 0:          # one snapshot directory, shared by the ranks of a node
                    shutil.rmtree(os.path.join(self.base_path, name), ignore_errors=True)
                self._on_disk.discard(name)

    @_protocol_call
    def add_assets(self, index_name, assets):
        # type: (str, List[IsccEntry]) -> List[IsccAddResult]
        return self._locked_index(index_name).add_assets(assets)

    @_protocol_call
    def get_asset(self, index_name, iscc_id):
        # type: (str, str) -> IsccEntry
        idx = self._locked_index(index_name)
        try:
            return idx.get_asset(iscc_id)
        except FileNotFoundError:
            raise FileNotFoundError(f"Asset '{iscc_id}' not found in index '{index_name}'")

    @_protocol_call
    def search_assets(self, index_name, query, limit=100):
        # type: (str, IsccQuery, int) -> IsccSearchResult
        idx = self._locked_index(index_name)
        try:
            return idx.search_assets(query, limit)
        except FileNotFoundError:
            raise FileNotFoundError(f"Asset '{query.iscc_id}' not found in index '{index_name}'")

    @_protocol_call
    def search_assets_many(self, index_name, queries, limit=100):
        # type: (str, List[IsccQuery], int) -> List[IsccSearchResult]
        """Many ``search_assets`` queries in one call (``HipIndex.search_assets_many``): result i equals ``search_assets(index_name, queries[i], limit)``."""
        idx = self._locked_index(index_name)
        try:
            return idx.search_assets_many(queries, limit)
        except FileNotFoundError as e:
            m = re.match(r"queries\[(\d+)\]: ", str(e))
            if m is None:
                raise
            i = int(m.group(1))
            raise FileNotFoundError(f"queries[{i}]: Asset '{queries[i].iscc_id}' not found in index '{index_name}'") from e

    # the pair finders are refused on a sharded index, and on one GPU a protocol call takes no lock: they need no mode
    def find_duplicates(self, index_name, min_score=None, unit_types=None, max_pairs=1_000_000, max_degree=None):
        # type: (str, Optional[float], Optional[List[str]], int, Optional[int]) -> List[DuplicatePair]
        """Near-duplicate asset pairs of one index (``HipIndex.find_duplicates``).  Not available on a sharded index."""
        self._refuse_sharded("find_duplicates")
        return self._locked_index(index_name).find_duplicates(min_score=min_score, unit_types=unit_types, max_pairs=max_pairs, max_degree=max_degree)

    def find_duplicate_groups(self, index_name, unit_types=None, threshold=None, min_size=2, max_degree=None):
        # type: (str, Optional[List[str]], Optional[float], int, Optional[int]) -> List[DuplicateGroup]
        """Groups of near-duplicate assets of one index (``HipIndex.find_duplicate_groups``).  Not available on a sharded index."""
        self._refuse_sharded("find_duplicate_groups")
        return self._locked_index(index_name).find_duplicate_groups(unit_types=unit_types, threshold=threshold, min_size=min_size, max_degree=max_degree)

    def find_hubs(self, index_name, min_degree=1, unit_types=None, threshold=None):
        # type: (str, int, Optional[List[str]], Optional[float]) -> List[Hub]
        """The assets of one index with many near-duplicates, per unit type (``HipIndex.find_hubs``).  Not available on a sharded index."""
        self._refuse_sharded("find_hubs")
        return self._locked_index(index_name).find_hubs(min_degree=min_degree, unit_types=unit_types, threshold=threshold)

    def find_shared_content(self, index_name, min_chunks=1, min_coverage=None, simprint_types=None, threshold=None, max_doc_freq=100, max_pairs=1_000_000,
                            segments=False, min_segment=1, max_gap=0):
        # type: (str, int, Optional[float], Optional[List[str]], Optional[float], int, int, bool, int, int) -> List[SharedContent]
        """Asset pairs of one index that share chunks, and where (``HipIndex.find_shared_content``).  Not available on a sharded index."""
        self._refuse_sharded("find_shared_content")
        return self._locked_index(index_name).find_shared_content(min_chunks=min_chunks, min_coverage=min_coverage, simprint_types=simprint_types,
                                                                  threshold=threshold, max_doc_freq=max_doc_freq, max_pairs=max_pairs,
                                                                  segments=segments, min_segment=min_segment, max_gap=max_gap)

    def find_matches(self, index_a, index_b, min_score=None, unit_types=None, max_pairs=1_000_000):
        # type: (str, str, Optional[float], Optional[List[str]], int) -> List[IndexMatch]
        """Asset pairs (a of ``index_a``, b of ``index_b``) that match (``HipIndex.find_matches``).  Not available on a sharded index."""
        self._refuse_sharded("find_matches")
        if index_a == index_b:
            raise ValueError(f"find_matches compares two indexes, got '{index_a}' twice: find_duplicates lists the pairs within one index")
        with self._lock:
            idx_a = self._index(index_a)
            idx_b = self._index(index_b)
        return idx_a.find_matches(idx_b, min_score=min_score, unit_types=unit_types, max_pairs=max_pairs)

    def find_shared_matches(self, index_a, index_b, min_chunks=1, min_coverage=None, simprint_types=None, threshold=None, max_doc_freq=100,
                            max_pairs=1_000_000, include_same_id=False, segments=False, min_segment=1, max_gap=0):
        # type: (str, str, int, Optional[float], Optional[List[str]], Optional[float], int, int, bool, bool, int, int) -> List[SharedMatch]
        """Asset pairs (a of ``index_a``, b of ``index_b``) that share chunks, and where (``HipIndex.find_shared_matches``).  Not available on a sharded index."""
        self._refuse_sharded("find_shared_matches")
        if index_a == index_b:
            raise ValueError(f"find_shared_matches compares two indexes, got '{index_a}' twice: find_shared_content lists the pairs within one index")
        with self._lock:
            idx_a = self._index(index_a)
            idx_b = self._index(index_b)
        return idx_a.find_shared_matches(idx_b, min_chunks=min_chunks, min_coverage=min_coverage, simprint_types=simprint_types, threshold=threshold,
                                         max_doc_freq=max_doc_freq, max_pairs=max_pairs, include_same_id=include_same_id,
                                         segments=segments, min_segment=min_segment, max_gap=max_gap)

    def close(self):
        # type: () -> None
        if self._leading and self._engine is not None and self._engine.broken is not None:
            # nothing can be flushed through a front that is down: release what is left of it
            with self._lock:
                if not self._closed:
                    self._closed = True
                    self._indexes.clear()
                    self._engine.close()
                    self._engine = None
            return
        if self._spmd is not None and not self._leads():      # (a leader takes no manager-wide lock)
            with self._spmd:
                return self._close()
        return self._close()

    def _close(self):
        with self._lock:
            if self._closed:
                return
            self._closed = True
            self._flush()
            for idx in self._indexes.values():
                idx.close()
            self._indexes.clear()
            if self._owns_engine and self._engine is not None:
                self._engine.close()
                self._engine = None


def get_index(uri="hip:///", **kwargs):
    # type: (str, object) -> HipIndexManager
    """
    Factory for the ``hip`` scheme, the branch a maintainer adds to the reference's
    ``options.get_index()`` next to ``iscc_search/options.py:360-371``.
    """
    parsed = urlparse(uri)
    if not parsed.scheme:
        raise ValueError(f"index URI requires an explicit scheme, got '{uri}'")
    if parsed.scheme != "hip":
        raise ValueError(f"Unsupported index URI scheme: '{parsed.scheme}' (this package serves hip://)")
    return HipIndexManager(uri, **kwargs)
