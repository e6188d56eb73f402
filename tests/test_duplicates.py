"""
``find_duplicates``: near-duplicate asset pairs of an index by a self-join of every unit table (CPU tier).

The engine is the oracle-backed stand-in with a numpy ``join_within`` (brute force over all row pairs).  What is checked is the
definition of the result: a pair {a, b} is listed with score S and unit scores T iff ``search_assets(IsccQuery(iscc_id=a),
limit=len(index))`` lists b with score S and T is the confident part of b's ``types`` -- and the same from b's side.
"""

import numpy as np
import pytest

from helpers import flip_bits, make_iscc_id
from iscc_search_amd import codec
from iscc_search_amd.index import HipIndex, HipIndexManager, HipOptions, _unit_max_hamming
from iscc_search_amd.schema import IsccEntry, IsccIndex, IsccQuery
from oracle_engine import OracleEngine, OracleTable


class JoinOracleTable(OracleTable):
    def join_within(self, max_hamming_by_prefix, max_pairs):
        """Every row pair (key_a < key_b) within max_hamming[min(len_a, len_b)] bits over the common prefix, by brute force."""
        keys, words, nb = self._arrays()
        kw = self.key_words
        n = len(nb)
        order = np.lexsort(keys.T[::-1]) if kw == 2 else np.argsort(keys)
        keys, words, nb = keys[order], words[order], nb[order]
        out = []
        for i in range(n):
            for j in range(i + 1, n):
                p = int(min(nb[i], nb[j]))
                limit = int(max_hamming_by_prefix[p])
                if limit < 0:
                    continue
                a = b"".join(int(w).to_bytes(8, "big") for w in words[i])[:p]
                b = b"".join(int(w).to_bytes(8, "big") for w in words[j])[:p]
                h = bin(int.from_bytes(a, "big") ^ int.from_bytes(b, "big")).count("1")
                if h <= limit:
                    out.append((i, j, h, 8 * p))
        if len(out) > max_pairs:
            raise ValueError(f"{len(out)} pairs exceed max_pairs={max_pairs}")
        ia = np.array([r[0] for r in out], dtype=np.int64)
        ib = np.array([r[1] for r in out], dtype=np.int64)
        return (keys[ia], keys[ib], np.array([r[2] for r in out], dtype=np.uint32), np.array([r[3] for r in out], dtype=np.uint16))


class JoinOracleEngine(OracleEngine):
    def open_table(self, metric, key_words, max_bytes):
        t = JoinOracleTable(metric, key_words, max_bytes)
        t.engine = self
        return t


def unit(mtype, body):
    return codec.encode_unit(mtype, 0, 0, body)


def build_assets(rng, n, offset=0):
    """Mixed unit lengths, planted near-duplicates (a few flipped bits of an earlier asset's units), shared INSTANCE prefixes."""
    assets, bodies = [], []
    for i in range(n):
        bits = int(rng.choice([64, 128, 256]))
        if bodies and rng.random() < 0.4:
            src = bodies[int(rng.integers(0, len(bodies)))]
            meta = flip_bits(src["meta"], int(rng.integers(0, 14)))
            content = flip_bits(src["content"], int(rng.integers(0, 40)))
            data = flip_bits(src["data"], int(rng.integers(0, 20)))
            inst = src["inst"] if rng.random() < 0.5 else rng.integers(0, 256, size=32, dtype=np.uint8).tobytes()
        else:
            meta, content, data, inst = (rng.integers(0, 256, size=32, dtype=np.uint8).tobytes() for _ in range(4))
        bodies.append({"meta": meta, "content": content, "data": data, "inst": inst})
        nb = bits // 8
        units = [unit(codec.MT_META, meta[:nb]), unit(codec.MT_CONTENT, content[:nb]), unit(codec.MT_DATA, data[:nb]),
                 unit(codec.MT_INSTANCE, inst[: int(rng.choice([8, 16, 32]))])]
        if rng.random() < 0.2:
            units = units[1:]                    # some assets carry no META unit
        assets.append(IsccEntry(iscc_id=make_iscc_id(offset + i), units=units))
    return assets


def definition(index):
    """{(id_a, id_b): (score, types)} from search_assets by every asset's iscc_id, checked to agree from both sides."""
    n = len(index)
    seen = {}
    for key, entry in sorted(index._assets.items()):
        res = index.search_assets(IsccQuery(iscc_id=entry.iscc_id), limit=n)
        thr = index._opts.match_threshold_units
        for m in res.global_matches:
            types = {t: s for t, s in m.types.items() if s >= thr}
            pair = tuple(sorted([entry.iscc_id, m.iscc_id], key=codec.iscc_id_to_int))
            if pair in seen:
                assert seen[pair] == (m.score, types), f"{pair} differs between the two sides"
            else:
                seen[pair] = (m.score, types)
    return seen


@pytest.fixture
def index():
    rng = np.random.default_rng(7)
    idx = HipIndex(JoinOracleEngine(), HipOptions())
    idx.add_assets(build_assets(rng, 220))
    return idx


def test_find_duplicates_equals_search_assets_definition(index):
    got = index.find_duplicates()
    exp = definition(index)
    assert len(got) > 20
    assert {(p.iscc_id_a, p.iscc_id_b): (p.score, p.types) for p in got} == exp
    keys = [(codec.iscc_id_to_int(p.iscc_id_a), codec.iscc_id_to_int(p.iscc_id_b)) for p in got]
    assert all(a < b for a, b in keys)
    assert [(-p.score, k) for p, k in zip(got, keys)] == sorted((-p.score, k) for p, k in zip(got, keys))
    # INSTANCE prefixes shared by several assets are among the pairs
    assert any("INSTANCE_NONE_V0" in p.types for p in got)


def test_find_duplicates_min_score_and_unit_types(index):
    full = index.find_duplicates()
    assert index.find_duplicates(min_score=0.9) == [p for p in full if p.score >= 0.9]
    only = index.find_duplicates(unit_types=["DATA_NONE_V0"])
    assert only and all(set(p.types) == {"DATA_NONE_V0"} for p in only)
    exp = {(p.iscc_id_a, p.iscc_id_b) for p in full if "DATA_NONE_V0" in p.types}
    assert {(p.iscc_id_a, p.iscc_id_b) for p in only} == exp


def test_unit_max_hamming_equals_brute_force():
    for thr in (0.0, 0.5, 0.75, 0.8, 0.9, 0.95, 1.0, 1.5):
        got = _unit_max_hamming(thr)
        assert got[0] == -1
        for p in range(1, 33):
            ok = [h for h in range(8 * p + 1) if max(0.0, 1.0 - float(np.float32(h) / np.float32(8 * p))) >= thr]
            assert got[p] == (max(ok) if ok else -1), (thr, p)
        assert list(_unit_max_hamming(thr, instance=True)[1:]) == [0 if thr <= 1.0 else -1] * 32


def test_max_pairs_is_surfaced(index):
    n = len(index.find_duplicates())
    with pytest.raises(ValueError, match="exceed max_pairs"):
        index.find_duplicates(max_pairs=1)
    assert n > 1


def test_manager_find_duplicates_and_sharded_refusal():
    rng = np.random.default_rng(3)
    m = HipIndexManager("hip:///", engine=JoinOracleEngine())
    m.create_index(IsccIndex(name="dups"))
    m.add_assets("dups", build_assets(rng, 40))
    got = m.find_duplicates("dups")
    assert got == m._indexes["dups"].find_duplicates()
    with pytest.raises(FileNotFoundError):
        m.find_duplicates("nope")
    m.close()
    sharded = HipIndexManager("hip:///?devices=2", engine=JoinOracleEngine())
    with pytest.raises(NotImplementedError, match="sharded"):
        sharded.find_duplicates("dups")
