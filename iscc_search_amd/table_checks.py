"""
Argument checks shared by every class with the duck type of ``HipTable`` (``engine.HipTable``, ``shard_front.LeaderTable``,
``sharded_engine.ShardedHipTable``): keys, code words and code lengths as the C-ABI takes them.  Imports without the HIP library.
"""

import numpy as np

from iscc_search_amd._lib import METRIC_HAMMING


class TableChecks:
    """For a class with ``metric``, ``key_words``, ``max_bytes`` and ``max_words``."""

    checks_length_range = False      # the library refuses a code length outside 1..max_bytes itself; ``LeaderTable`` must, before it broadcasts

    def _keys(self, keys):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        if self.key_words == 2:
            if keys.ndim != 2 or keys.shape[1] != 2:
                raise ValueError("128-bit keys must be shaped [n, 2] (hi, lo)")
        elif keys.ndim != 1:
            raise ValueError("64-bit keys must be shaped [n]")
        return keys

    def _words(self, words, n=None):
        words = np.ascontiguousarray(words, dtype=np.uint64)
        if words.ndim != 2 or words.shape[1] != self.max_words:
            raise ValueError(f"code words must be shaped [n, {self.max_words}]")
        if n is not None and words.shape[0] != n:
            raise ValueError("keys and codes differ in length")
        return words

    def _nbytes(self, nbytes, n):
        if self.metric == METRIC_HAMMING:
            if nbytes is not None and np.any(np.asarray(nbytes) != self.max_bytes):
                raise ValueError(f"Hamming table holds {self.max_bytes}-byte codes only")
            return None
        if nbytes is None:
            raise ValueError("nbytes is required for NPHD tables")
        nbytes = np.ascontiguousarray(nbytes, dtype=np.uint8)
        if nbytes.shape != (n,):
            raise ValueError("nbytes must be shaped [n]")
        if self.checks_length_range and n and (int(nbytes.min()) < 1 or int(nbytes.max()) > self.max_bytes):
            raise ValueError(f"code length outside 1..{self.max_bytes} bytes")
        return nbytes
