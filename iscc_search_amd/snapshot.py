"""
Snapshots of a ``HipIndex`` (``HipIndex.save`` / ``HipIndex.load``).  The reference persists through LMDB + HNSW shard files
and ``flush()`` / ``close()`` (``usearch/index.py:883-967``).  Here a snapshot is: index.json, assets.jsonl, and the raw code
columns of every table (units/<type>/, simprints/<type>/) exactly as they sit in HBM.
"""

import json
import os

import numpy as np

from iscc_search_amd.schema import IsccEntry
from iscc_search_amd.simprint import unpack_chunk_pointer
from iscc_search_amd.unit_match import _unit_map


def save(idx, path):
    # type: (object, str) -> None
    with idx._lock:
        os.makedirs(path, exist_ok=True)
        # sharded index (hip:///path?devices=N): every rank writes its own table shards, rank 0 the host files
        writer = getattr(idx._engine, "rank", 0) == 0
        if writer:
            with open(os.path.join(path, "assets.jsonl.tmp"), "w") as f:
                for key, asset in idx._assets.items():
                    f.write(json.dumps({"key": key, "asset": asset.model_dump(mode="json", exclude_none=True)}, separators=(",", ":")) + "\n")
            os.replace(os.path.join(path, "assets.jsonl.tmp"), os.path.join(path, "assets.jsonl"))
        for unit_type, table in idx._unit_tables.items():
            table.save(os.path.join(path, "units", unit_type))
        for sp_type, table in idx._sp_tables.items():
            table.save(os.path.join(path, "simprints", sp_type))
            if writer:
                # the per-asset chunk lists are host state every rank keeps whole: written once, by rank 0, beside the table
                # shards, so that a restore reads a file instead of gathering every shard's rows to every rank
                pairs = [pair for chunks in idx._sp_assets.get(sp_type, {}).values() for pair in chunks]
                nb = table.ndim // 8
                ptrs = np.frombuffer(b"".join(ptr for _, ptr in pairs), dtype=np.uint8).reshape(len(pairs), 16)
                sps = np.frombuffer(b"".join(sp for sp, _ in pairs), dtype=np.uint8).reshape(len(pairs), nb)
                tmp = os.path.join(path, "simprints", sp_type, "host_chunks.tmp.npz")
                np.savez(tmp, pointers=ptrs, simprints=sps)
                os.replace(tmp, os.path.join(path, "simprints", sp_type, "host_chunks.npz"))
        if writer:
            meta = {
                "format": 1, "realm_id": idx._realm_id, "assets": len(idx._assets),
                "unit_types": sorted(idx._unit_tables),
                "simprint_types": {t: tbl.ndim for t, tbl in idx._sp_tables.items()},
                "ranks": getattr(idx._engine, "world_size", 1),
            }
            with open(os.path.join(path, "index.json.tmp"), "w") as f:
                json.dump(meta, f)
            os.replace(os.path.join(path, "index.json.tmp"), os.path.join(path, "index.json"))
        if hasattr(idx._engine, "all_gather_object"):
            idx._engine.all_gather_object(None)       # nobody returns before rank 0 has written index.json
        idx.dirty = False


def load(index_cls, engine, path, options=None):
    # type: (type, object, str, object) -> object
    """A new ``index_cls`` (``HipIndex``) over ``engine`` holding the snapshot at ``path``."""
    with open(os.path.join(path, "index.json")) as f:
        meta = json.load(f)
    if meta.get("ranks", 1) != getattr(engine, "world_size", 1):
        raise ValueError(f"snapshot at {path} was written by {meta.get('ranks', 1)} rank(s), this manager runs {getattr(engine, 'world_size', 1)}")
    idx = index_cls(engine, options)
    idx._realm_id = meta["realm_id"]
    assets_file = os.path.join(path, "assets.jsonl")
    if os.path.exists(assets_file):
        with open(assets_file) as f:
            for line in f:
                rec = json.loads(line)
                asset = IsccEntry(**rec["asset"])
                idx._assets[rec["key"]] = asset
                idx._asset_units[rec["key"]] = _unit_map(asset.units)
    for unit_type in meta["unit_types"]:
        idx._unit_table(unit_type).load(os.path.join(path, "units", unit_type))
    for sp_type, ndim in meta["simprint_types"].items():
        table = idx._sp_table(sp_type, ndim)
        table.load(os.path.join(path, "simprints", sp_type))
        # the host-side per-asset chunk lists (host state every rank keeps whole): from the file rank 0 wrote; snapshots of
        # before that file existed derive them from the stored rows (of every shard, gathered)
        host_chunks = os.path.join(path, "simprints", sp_type, "host_chunks.npz")
        if os.path.exists(host_chunks):
            with np.load(host_chunks) as z:
                rows = sorted((z["pointers"][i].tobytes(), z["simprints"][i].tobytes()) for i in range(len(z["pointers"])))
        else:
            rows = list(table.rows())
            if hasattr(engine, "all_gather_object"):
                rows = sorted(r for part in engine.all_gather_object(rows) for r in part)
        for ckey, sp_bytes in rows:
            body = unpack_chunk_pointer(ckey)[0]
            idx._sp_assets[sp_type].setdefault(body, []).append((sp_bytes, ckey))
    return idx
