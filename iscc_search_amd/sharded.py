"""
Row-range sharding of one table across the GPUs of a node (one process per GPU).

The reference has no distributed path at all (single process, ``usearch/manager.py:43-46``); this is
the MI355X-native addition SURVEY.md section 8e describes.  Rows are independent and top-k is a
decomposable reduction, so the only exchange is ONE all-gather of the per-shard results
(one block of ``nq * k`` 24-byte records + ``nq`` counts per rank; RCCL over xGMI when the process group's backend
is ``nccl``), followed by a k-way merge on every rank (``merge_kernel``).  No ring all-reduce, no
second collective: at 160 KB per rank for 1 024 queries the exchange is latency bound.

``ShardedTable`` is transport- and engine-agnostic: it drives a small "ops" object.
``HipShardOps`` is the product implementation (device buffers owned by torch, kernels by the
C-ABI); tests drive the same class over gloo with an oracle-backed ops object.
"""

import collections
import contextlib
import os

import numpy as np

from iscc_search_amd._lib import COUNT_OVERFLOW

RECORD_BYTES = 24


def shard_range(n_rows, rank, world_size):
    # type: (int, int, int) -> tuple[int, int]
    """Contiguous row range [lo, hi) of ``rank``: sizes differ by at most one row."""
    lo = n_rows * rank // world_size
    hi = n_rows * (rank + 1) // world_size
    return lo, hi


def shard_of_key(key_lo, world_size):
    # type: (int, int) -> int
    """Owner rank of a key for hash-routed (mutable) tables."""
    x = (int(key_lo) * 0x9E3779B97F4A7C15) & (2**64 - 1)
    return (x >> 32) % world_size


def hint_margin(k):
    # type: (int) -> int
    """Bits above the previous step's worst k-th distance a hinted step starts at: as the engine's own hints (isccsearch.hip, SpecHint::margin)."""
    return 1 if k >= 64 else 2


def block_bytes(nq, k):
    # type: (int, int) -> tuple[int, int]
    """Per-rank exchange block {records [nq][k] | counts [nq] | pad}: (record bytes, block bytes)."""
    rec = nq * k * RECORD_BYTES
    return rec, rec + (nq * 4 + 7) // 8 * 8


def worst_if_full(result, k):
    """The largest k-th distance of merged lists that are FULL -- no overflow marker, k rows in each -- else None."""
    count = result[3]
    if np.any(count == COUNT_OVERFLOW) or int(count.min()) < k:
        return None
    return int(result[1][:, k - 1].max())


class ShardHint:
    """
    What the shards of one table start a step of one shape under: the GLOBAL k-th distance the previous step of that shape ended
    at + ``hint_margin``.  Every shard takes one pass within it (no bootstrap sample), and the step stands if the merged lists are
    full: their rows all lie within the hint, so nothing nearer was left out.  The merged lists are the same on every rank, hence
    so is every transition taken from them.
    """

    value = None            # the distance the next hinted step starts under
    skip = penalty = 0      # steps still to run without a hint after a miss; what the next miss doubles

    def start(self):
        """The hint this step runs under, or None (which counts one pending skip down)."""
        if self.skip:
            self.skip -= 1
            return None
        return self.value

    def held(self, worst, k):
        """The hinted step stood: the hint decays by one bit per step towards what the batches need."""
        self.value, self.penalty = max(worst + hint_margin(k), self.value - 1), 0

    def missed(self):
        """The hinted step came up short: 0, 2, 6, 14 steps without a hint for 1, 2, 3, 4 misses in a row."""
        self.penalty = min(2 * self.penalty + 1, 15)
        self.skip = self.penalty - 1

    def reseed(self, worst, k):
        """After an unhinted or a repeated step; ``worst`` None: its lists were not full (a table with fewer than k rows never gets a hint)."""
        self.value = None if worst is None else worst + hint_margin(k)


def _exchange_scope(ops):
    """The ops' scope for one search step (``HipShardOps.exchange_scope``: torch's current stream := the library's), if it has one."""
    make = getattr(ops, "exchange_scope", None)
    return make() if make is not None else contextlib.nullcontext()


class _OnLibraryStream:
    """``with``: the calling thread's current torch stream on the ops' device is the library's stream; restored on the way out."""

    __slots__ = ("ops", "prev")

    def __init__(self, ops):
        self.ops = ops
        self.prev = None

    def __enter__(self):
        ops = self.ops
        if ops._stream() != ops._lib_stream:
            self.prev = ops._get_current(ops._device_index)           # (stream id, device index, device type)
            ops._set_current(stream_id=ops._ext.stream_id, device_index=ops._ext.device_index, device_type=ops._ext.device_type)
        return self

    def __exit__(self, *exc):
        if self.prev is not None:
            self.ops._set_current(stream_id=self.prev[0], device_index=self.prev[1], device_type=self.prev[2])
        return False


class HipShardOps:
    """Local search + merge on one GPU through the C-ABI; buffers are torch tensors on that GPU."""

    def __init__(self, table, device):
        import torch

        self.torch = torch
        self.table = table
        self.engine = table.engine
        self.device = torch.device(device)
        self.key_words = table.key_words
        self._buffers = {}
        self._ext = None
        self._lib_stream = self.engine.stream() if hasattr(self.engine, "stream") else 0
        self._raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        self._get_current = getattr(torch._C, "_cuda_getCurrentStream", None)
        self._set_current = getattr(torch._C, "_cuda_setStream", None)
        self._device_index = self.device.index if self.device.index is not None else torch.cuda.current_device()

    def _stream(self):
        # (torch.cuda.current_stream() builds a Stream object: 5.5 us a call, three calls a step; the raw accessor returns the pointer)
        if self._raw_stream is not None:
            return self._raw_stream(self._device_index)
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def exchange_scope(self):
        """
        torch's current stream := the LIBRARY's stream (``isccsearch_stream`` as a ``torch.cuda.ExternalStream``) for one search
        step: local search, all-gather (a collective without ``async_op`` is launched on the current stream) and merge are then
        one in-order queue -- no event between two queues in front of the exchange and in front of the merge (~12 + ~21 us of
        hand-over per step, ``profiles/r04_step_timelines.txt``).  Outside the scope the calls still order themselves by events.
        (``torch.cuda.stream()`` does the same in ~10 us of Stream objects a step; with torch's raw accessors it is ~2.)
        """
        if not self._lib_stream or os.environ.get("ISCC_HIP_SHARD_ONE_QUEUE", "1") == "0":
            return contextlib.nullcontext()              # the step's stages on torch's own current stream, ordered by events
        if self._ext is None:
            self._ext = self.torch.cuda.ExternalStream(self._lib_stream, device=self.device)
        if self._raw_stream is None or self._get_current is None or self._set_current is None:
            return self.torch.cuda.stream(self._ext)
        return _OnLibraryStream(self)

    supports_hint = True

    def local_search(self, q_words, q_nbytes, k, max_hamming=None, synchronous=False, hint=None):
        """
        One device block {records | counts} holding this shard's exact top-k (within ``max_hamming`` if given; with ``hint``: its
        nearest rows within that distance -- fewer than k when the hint was too tight, which ``ShardedTable`` notices after the merge).

        Asynchronous by default: the search is queued on the library's stream and torch's current stream -- the one the
        all-gather is issued on -- waits for it on the device; nothing waits on the host.  ``synchronous`` runs the
        classic path, which also completes queries whose candidate list overflowed (the asynchronous one marks them).
        """
        nq = q_words.shape[0]
        rec_bytes, blk = block_bytes(nq, k)
        buf = self.buffer("block", blk)
        self.table.search_device(q_words, q_nbytes, k, buf.data_ptr(), buf.data_ptr() + rec_bytes, max_hamming=max_hamming,
                                 consumer_stream=None if synchronous else self._stream(), hint=None if synchronous else hint)
        return buf

    def buffer(self, name, nbytes):
        """
        A device buffer of ``nbytes`` kept between steps (one per role and size; a step's buffers are consumed before the next
        step of the same shape starts: the merge synchronises).  Allocating them per step cost ~15 us of host time each.
        """
        key = (name, nbytes)
        buf = self._buffers.get(key)
        if buf is None:
            if len(self._buffers) >= 16:
                self._buffers.clear()
            buf = self._buffers[key] = self.torch.empty(nbytes, dtype=self.torch.uint8, device=self.device)
        return buf

    def search_single(self, q_words, q_nbytes, k, max_hamming=None):
        """The whole answer when this shard is the only one: the host entry point (no result block, no merge launch)."""
        if max_hamming is None:
            return self.table.search(q_words, q_nbytes, k)
        return self.table.search_within(q_words, q_nbytes, k, max_hamming)

    def local_doc_freq(self, q_words, q_nbytes, dup_limit):
        """This shard's (distinct assets, colliding rows looked at) per code: lookup and reduction on the device."""
        return self.table.doc_freq_counted(q_words, q_nbytes, dup_limit)

    def merge(self, gathered, n_lists, nq, k):
        """Merge ordered behind torch's current stream (where the gathered blocks were produced): one copy, one synchronisation."""
        rec_bytes, blk = block_bytes(nq, k)
        base = gathered.data_ptr()
        return self.engine.merge_device(n_lists, nq, k, self.key_words, base, base + rec_bytes, blk, blk, after_stream=self._stream())

    def merge_many(self, gathered, stride, parts):
        """Several parts of a fused exchange merged behind ONE synchronisation; parts = [(offset, n_lists, nq, k, key_words)]; None = too large for one call."""
        base = gathered.data_ptr()
        merges = []
        total = 0
        for offset, n_lists, nq, k, key_words in parts:
            rec_bytes, _ = block_bytes(nq, k)
            merges.append((n_lists, nq, k, key_words, base + offset, base + offset + rec_bytes, stride, stride))
            total += rec_bytes + nq * 4 + 16
        if total > (1 << 20):
            return None
        return self.engine.merge_many(merges, self._stream())

    def merge_strided(self, gathered, offset, stride, n_lists, nq, k):
        """The same for a block that is one PART of every rank's share of a fused exchange: list l sits at offset + l x stride."""
        rec_bytes, _ = block_bytes(nq, k)
        base = gathered.data_ptr() + offset
        return self.engine.merge_device(n_lists, nq, k, self.key_words, base, base + rec_bytes, stride, stride, after_stream=self._stream())


class ShardedTable:
    """
    One logical table whose rows are spread over the ranks of a ``torch.distributed`` process group.

    Every rank calls ``search`` with the SAME queries and gets the SAME global top-k back.
    """

    def __init__(self, ops, group=None, always_gather=False, assets_share_a_rank=False):
        import torch.distributed as dist

        self.dist = dist
        self.ops = ops
        self.group = group
        self.always_gather = always_gather   # run the collective even with one rank (rehearsal on one GPU)
        # rows routed by the asset word of their key (sharded_engine.ShardedHipTable): per-shard document frequencies add.
        # Row-RANGE shards (bench.py, the engine-level tests) may split an asset's chunks: the merged list is reduced instead
        self.assets_share_a_rank = assets_share_a_rank
        self.world_size = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.use_hints = bool(getattr(ops, "supports_hint", False)) and not os.environ.get("ISCC_NO_SHARD_HINT")
        self._hints = collections.defaultdict(ShardHint)      # by (batch-size class, k, query lengths)
        self.hint_hits = self.hint_misses = 0
        self._stages_on_host = None

    def _staged(self):
        """The rehearsal transport (several ranks sharing one GPU cannot use RCCL: gloo, blocks staged through the host)?  Asked once."""
        if self._stages_on_host is None:
            self._stages_on_host = self.dist.get_backend(self.group) == "gloo"
        return self._stages_on_host

    def search(self, q_words, q_nbytes, k):
        # type: (np.ndarray, np.ndarray | None, int) -> tuple
        return self._search(q_words, q_nbytes, k, None)

    def search_within(self, q_words, q_nbytes, k, max_hamming):
        # type: (np.ndarray, np.ndarray | None, int, int) -> tuple
        """
        Range-limited search over all shards: each rank lists its rows within ``max_hamming`` (nearest first, at most
        k), the same all-gather + merge keeps the k nearest overall -- the lists are ordered by (distance, key), so
        the merged list equals the unsharded one.
        """
        return self._search(q_words, q_nbytes, k, int(max_hamming))

    def doc_freq(self, q_words, q_nbytes=None, dup_limit=1000):
        # type: (np.ndarray, np.ndarray | None, int) -> np.ndarray
        """
        Distinct assets among the first ``dup_limit`` collisions of each code across ALL shards (``count_doc_freq``,
        ``lmdb_ops.py:139-166``).

        Rows are routed by their ASSET word, so an asset's chunks share a rank and the shards' distinct-asset counts ADD --
        as long as every collision is looked at, i.e. the collisions of all shards together stay within ``dup_limit`` (the
        normal case: each shard reduces its own list on the device, one small all-reduce sums counts and lengths).  A code
        with more collisions than that is cut at ``dup_limit`` in key order ACROSS the shards: for those codes only, the
        merged collision list is reduced (the lists are ordered by key, so distinct assets are the changes of the asset word).
        """
        local = getattr(self.ops, "local_doc_freq", None)
        if self.world_size == 1 and not self.always_gather and local is not None:
            return local(q_words, q_nbytes, dup_limit)[0]
        nq = q_words.shape[0]
        if local is None or not self.assets_share_a_rank:
            slow = np.arange(nq)
            out = np.zeros(nq, dtype=np.uint32)
        else:
            freq, coll = local(q_words, q_nbytes, dup_limit)
            both = self._all_reduce_sum(np.concatenate([freq.astype(np.int64), coll.astype(np.int64)]))
            out = both[:nq].astype(np.uint32)
            slow = np.nonzero(both[nq:] > dup_limit)[0]          # the same on every rank: they all take the slow path together
        if len(slow):
            qn = None if q_nbytes is None else np.ascontiguousarray(np.asarray(q_nbytes)[slow])
            keys, _, _, cnt = self.search_within(np.ascontiguousarray(q_words[slow]), qn, dup_limit, 0)
            assets = keys[..., 0] if keys.ndim == 3 else keys
            valid = np.arange(assets.shape[1])[None, :] < cnt[:, None]
            change = np.ones_like(valid)
            change[:, 1:] = assets[:, 1:] != assets[:, :-1]
            out[slow] = (valid & change).sum(axis=1).astype(np.uint32)
        return out

    def _all_reduce_sum(self, arr):
        # type: (np.ndarray) -> np.ndarray
        """Small host array summed over the ranks (the ops object may bring its own transport: ``ShardedEngine.all_reduce``)."""
        reducer = getattr(self.ops, "all_reduce_sum", None)
        if reducer is not None:
            return reducer(arr)
        import torch

        t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.int64).copy())
        if self.dist.get_backend(self.group) == "nccl":
            t = t.to(getattr(self.ops, "device", "cuda"))
        self.dist.all_reduce(t, group=self.group)
        return t.cpu().numpy()

    def _alone(self):
        """One rank and no forced collective: nothing to exchange."""
        return self.world_size == 1 and not (self.always_gather and self.dist.is_initialized())

    def hint(self, q_words, q_nbytes, k):
        # type: (np.ndarray, np.ndarray | None, int) -> ShardHint
        """The hint of top-k searches of this shape."""
        qlen = None if q_nbytes is None else tuple(sorted(set(int(b) for b in np.asarray(q_nbytes))))      # (a prefix length has its own distances)
        return self._hints[(int(q_words.shape[0]).bit_length(), int(k), qlen)]

    def _search(self, q_words, q_nbytes, k, max_hamming):
        return ShardedTable._step([(self, q_words, q_nbytes, k, max_hamming)])[0]

    @staticmethod
    def search_many(items):
        """
        Several searches -- the per-unit searches of one ``search_assets`` request (``usearch/index.py:786-806``), each on its own
        table -- with ONE exchange: every shard runs its local searches back to back, their blocks travel in one all-gather, each
        part is merged on its own.  ``items`` = [(ShardedTable, q_words, q_nbytes, k, max_hamming | None)], queries of one length
        per item; returns the results in order, or None when the items cannot share an exchange (the caller then runs them one
        by one).
        """
        first = items[0][0]
        if first.world_size == 1 or len(items) < 2 or len({(id(t.ops), block_bytes(q.shape[0], k)[1]) for t, q, _, k, _ in items}) != len(items):
            return None            # (two items on one table with one block size -- (3, 4) and (4, 3) alike -- would share that table's block buffer, HipShardOps.buffer)
        if any(t.world_size != first.world_size or t.group is not first.group for t, *_ in items):
            return None
        return ShardedTable._step(items)

    @staticmethod
    def _step(items):
        """
        One step for ``items`` (as ``search_many``): the exchange, every top-k item under its table's hint, then one verdict per item
        from its merged lists -- the same on every rank, so every rank repeats the same items together.
        """
        alone = items[0][0]._alone()
        hints, hows = [], []
        for t, q_words, q_nbytes, k, max_hamming in items:
            hint = t.hint(q_words, q_nbytes, k) if t.use_hints and max_hamming is None and q_words.shape[0] and not alone else None
            start = None if hint is None else hint.start()
            hints.append(hint)
            hows.append({} if start is None else {"hint": start})
        out = ShardedTable._exchange(items, hows, alone)
        for i, item in enumerate(items):
            t, k, hint = item[0], item[3], hints[i]
            if hows[i]:              # (hinted)
                worst = worst_if_full(out[i], k)
                if worst is not None:
                    t.hint_hits += 1
                    hint.held(worst, k)
                    continue
                # the hint was too tight for some query (or a list overflowed under it): THIS item again without it
                t.hint_misses += 1
                hint.missed()
                out[i] = ShardedTable._exchange([item], [{}], alone)[0]
            if np.any(out[i][3] == COUNT_OVERFLOW):
                # some shard's candidate list overflowed and the asynchronous search could only mark it: THIS item again
                # through the synchronous path (exact fallback)
                out[i] = ShardedTable._exchange([item], [{"synchronous": True}], alone)[0]
            if hint is not None:
                hint.reseed(worst_if_full(out[i], k), k)
        return out

    @staticmethod
    def _exchange(items, hows, alone):
        """Every item's local search (``hows``: its extra arguments), ONE gather of the ranks' shares, the merges: one result per item."""
        first, q_words, q_nbytes, k, max_hamming = items[0]
        single = getattr(first.ops, "search_single", None)
        if alone and single is not None:
            return [single(q_words, q_nbytes, k, max_hamming)]
        with _exchange_scope(first.ops):
            blocks = []
            for (t, qw, qn, kk, radius), how in zip(items, hows):
                blocks.append(t.ops.local_search(qw, qn, kk, **how) if radius is None else t.ops.local_search(qw, qn, kk, radius, **how))
            if len(items) == 1:          # (no concatenation, no copy; alone: this rank's block is the one list)
                gathered = blocks[0] if alone else first._gather(blocks[0])
                return [first.ops.merge(gathered, 1 if alone else first.world_size, q_words.shape[0], k)]
            import torch

            share = torch.cat(blocks)
            return ShardedTable._merge_parts(items, blocks, first._gather(share), share.numel())

    def _gather(self, share):
        """The one exchange step of the path: [world] x this rank's share, a share = {records [nq][k] | counts [nq]} per item."""
        import torch

        total = self.world_size * share.numel()
        staged = share.is_cuda and self._staged()
        if staged:
            # rehearsal transport (several ranks sharing one GPU cannot use RCCL): the blocks are staged through the host
            gathered, mine = torch.empty(total, dtype=share.dtype), share.cpu()
        else:
            make = getattr(self.ops, "buffer", None)
            gathered, mine = make("gathered", total) if make else torch.empty(total, dtype=share.dtype, device=share.device), share
        self.dist.all_gather_into_tensor(gathered, mine, group=self.group)
        return gathered.to(share.device) if staged else gathered

    @staticmethod
    def _merge_parts(items, blocks, gathered, stride):
        """
        The merges of a fused exchange (a part's lists lie ``stride`` bytes apart): queued back to back behind ONE synchronisation
        when the ops share an engine that can (``HipShardOps.merge_many``), else a strided merge each, else a contiguous copy each.
        """
        first = items[0][0]
        parts, offset = [], 0
        for (t, q_words, _, k, _), block in zip(items, blocks):
            parts.append((offset, t.world_size, q_words.shape[0], k, t.ops.key_words))
            offset += block.numel()
        many = getattr(first.ops, "merge_many", None)
        if many is not None and all(getattr(t.ops, "engine", None) is first.ops.engine for t, *_ in items):
            merged = many(gathered, stride, parts)
            if merged is not None:
                return merged
        out = []
        for (t, *_), block, (offset, n_lists, nq, k, _) in zip(items, blocks, parts):
            strided = getattr(t.ops, "merge_strided", None)
            if strided is not None:
                out.append(strided(gathered, offset, stride, n_lists, nq, k))
            else:
                out.append(t.ops.merge(gathered.view(n_lists, stride)[:, offset : offset + block.numel()].contiguous().view(-1), n_lists, nq, k))
        return out
