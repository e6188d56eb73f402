"""
Bulk asset search over a sharded index (``hip:///path?devices=2``, two processes, gloo, CPU): ``search_assets_many`` takes the
host fallback there -- one ``search_many`` request per (unit type, code length) with many queries each, so that several requests
on one table share the exchange (``ShardedTable.search_many``) -- and must answer exactly what a loop of ``search_assets`` answers,
on every rank, and what the unsharded manager answers.  The index holds near-duplicates of a few base codes at mixed lengths and
an INSTANCE prefix shared by more than ``INSTANCE_FIRST_K`` assets (the second, full-length request).
"""

import json
import os
import socket

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import make_iscc_id
from iscc_search_amd import codec
from iscc_search_amd.index import HipIndexManager, INSTANCE_FIRST_K
from iscc_search_amd.schema import IsccEntry, IsccIndex, IsccQuery
from oracle_engine import OracleEngine
from test_assets_many import clustered_assets, mixed_queries


def scenario(manager):
    """Every rank (and the unsharded manager) runs the same calls; returns (bulk answers, loop answers) as JSON strings."""
    assets, base = clustered_assets(160, seed=3)
    rng = np.random.default_rng(4)
    inst = rng.integers(0, 256, size=16, dtype=np.uint8).tobytes()
    n_shared = INSTANCE_FIRST_K + 20
    shared = [IsccEntry(iscc_id=make_iscc_id(1000 + i), units=[codec.encode_unit(codec.MT_DATA, 0, 0, rng.integers(0, 256, size=8, dtype=np.uint8).tobytes()),
                                                                codec.encode_unit(codec.MT_INSTANCE, 0, 0, inst[: 8 * (1 + i % 2)])]) for i in range(n_shared)]
    manager.create_index(IsccIndex(name="m"))
    manager.add_assets("m", assets + shared)
    queries = mixed_queries(assets, base, np.random.default_rng(8), 30) + [
        IsccQuery(units=[codec.encode_unit(codec.MT_INSTANCE, 0, 0, inst[:8])]),
        IsccQuery(iscc_id=shared[5].iscc_id),
    ]
    dump = lambda r: json.dumps({"result": r.model_dump(mode="json"), "type_order": [list(x.types) for x in r.global_matches]})  # noqa: E731
    out = {}
    for limit in (10, 100):
        out[f"many{limit}"] = [dump(r) for r in manager.search_assets_many("m", queries, limit)]
        out[f"loop{limit}"] = [dump(manager.search_assets("m", q, limit)) for q in queries]
    manager.close()
    return out, n_shared


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from iscc_search_amd.sharded_engine import ShardedEngine
        from test_sharded_gloo import OracleShardOps

        m = HipIndexManager(f"hip://{out_dir}/store?devices={world}", engine=ShardedEngine(OracleEngine(), ops_factory=OracleShardOps))
        out, _ = scenario(m)
        with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
            json.dump(out, f)
    finally:
        dist.destroy_process_group()


def test_sharded_bulk_search_equals_the_loop_and_the_unsharded_index(tmp_path):
    world = 2
    with socket.socket() as sck:
        sck.bind(("127.0.0.1", 0))
        port = sck.getsockname()[1]
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    want, n_shared = scenario(HipIndexManager("hip:///", engine=OracleEngine()))
    assert want["many100"] == want["loop100"]
    assert len(json.loads(want["many100"][-2])["result"]["global_matches"]) == n_shared      # the second INSTANCE request ran
    for rank in range(world):
        with open(tmp_path / f"rank{rank}.json") as f:
            got = json.load(f)
        for key in want:
            assert got[key] == want[key], f"rank {rank}, {key}"
        assert got["many10"] == got["loop10"] and got["many100"] == got["loop100"]
