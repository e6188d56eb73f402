"""
The host model of the column store (``tests/store_model.py``) checked without a GPU: hand-written cases pin its masking and its
segment sets, tampered tables show that ``assert_table_equals`` notices each kind of damage, and the bodies of
``tests/test_gpu_store.py`` that need nothing but the table interface run on the oracle-backed engine, as ``test_persistence.py``
runs its cases on both.
"""

import numpy as np
import pytest

import test_gpu_store as store
from oracle_engine import OracleEngine, OracleTable
from store_model import StoreModel, assert_table_equals, dirty_words, mask_words, word_mask

U = np.uint64


def test_word_masks_by_hand():
    assert word_mask(3, 0) == 0xFFFFFF0000000000 and word_mask(3, 1) == 0
    assert word_mask(8, 0) == 0xFFFFFFFFFFFFFFFF and word_mask(8, 1) == 0
    assert word_mask(12, 0) == 0xFFFFFFFFFFFFFFFF and word_mask(12, 1) == 0xFFFFFFFF00000000 and word_mask(12, 2) == 0
    assert word_mask(1, 0) == 0xFF00000000000000 and word_mask(32, 3) == 0xFFFFFFFFFFFFFFFF


def test_a_3_byte_code_with_dirty_padding():
    m = StoreModel(0, 1, 3)
    m.add(np.array([7], dtype=U), np.array([[0xABCDEF1234567890]], dtype=U))
    assert m.rows == {(7,): (3, (0xABCDEF0000000000,))}
    assert m.segment_set(3) == {((7,), (0xABCDEF0000000000,))} and m.segments() == {3: 1}
    np.testing.assert_array_equal(dirty_words(np.array([[0xABCDEF0000000000]], dtype=U), 3), np.array([[0xABCDEFFFFFFFFFFF]], dtype=U))
    np.testing.assert_array_equal(mask_words(np.array([[0xABCDEFFFFFFFFFFF]], dtype=U), 3), np.array([[0xABCDEF0000000000]], dtype=U))


def test_a_12_byte_code_in_a_32_byte_table():
    m = StoreModel(1, 1, 32)
    full = [0x1111111111111111, 0x2222222222222222, 0x3333333333333333, 0x4444444444444444]
    m.add(np.array([5, 6], dtype=U), np.array([full, full], dtype=U), np.array([12, 32], dtype=np.uint8))
    assert m.rows[(5,)] == (12, (0x1111111111111111, 0x2222222200000000, 0, 0))
    assert m.rows[(6,)] == (32, tuple(full))
    assert m.segments() == {12: 1, 32: 1}
    assert m.segment_set(12) == {((5,), (0x1111111111111111, 0x2222222200000000))}          # W = 2 words are kept
    keys, words, lens = m.arrays()
    assert keys.tolist() == [5, 6] and lens.tolist() == [12, 32] and words[0].tolist() == [0x1111111111111111, 0x2222222200000000, 0, 0]
    m.add_columns(12, np.array([9], dtype=U), np.array([[0xAAAAAAAAAAAAAAAA], [0xBBBBBBBBBBBBBBBB]], dtype=U))
    assert m.rows[(9,)] == (12, (0xAAAAAAAAAAAAAAAA, 0xBBBBBBBB00000000, 0, 0))


def test_128_bit_keys_and_removal():
    m = StoreModel(0, 2, 8)
    keys = np.array([[1, 9], [1, 8], [2, 9]], dtype=U)
    m.add(keys, np.array([[10], [20], [30]], dtype=U))
    assert list(m.rows) == [(1, 9), (1, 8), (2, 9)]                                        # insertion order
    with pytest.raises(KeyError):
        m.add(np.array([[3, 3], [1, 8]], dtype=U), np.array([[1], [2]], dtype=U))          # present
    with pytest.raises(KeyError):
        m.add(np.array([[3, 3], [3, 3]], dtype=U), np.array([[1], [2]], dtype=U))          # repeated in the batch
    assert len(m) == 3                                                                      # ... and nothing was taken
    assert m.remove(np.array([[1, 8], [7, 7], [1, 8]], dtype=U)) == 1                      # absent and named twice count for nothing
    assert m.keys_in_order().tolist() == [[1, 9], [2, 9]]
    absent = m.absent_keys(np.random.default_rng(0), 20)
    assert absent.shape == (20, 2) and not any(tuple(k) in m.rows for k in absent.tolist())
    assert store.model_doc_freq(m, [10], 1000) == 1


class Tampered(OracleTable):
    """An oracle-backed table whose reads can be made to lie."""

    damage = None

    def export_rows(self, nbytes, first_row, n):
        keys, cols = super().export_rows(nbytes, first_row, n)
        if self.damage == "bit" and first_row == 0 and n:
            cols[0, 0] ^= U(1) << U(40)
        if self.damage == "padding" and n:
            cols[-1, n - 1] |= U(1)
        if self.damage == "twice" and n > 1:
            keys[0], cols[:, 0] = keys[1], cols[:, 1]
        if self.damage == "overlap" and first_row:
            keys, cols = super().export_rows(nbytes, first_row - 1, n)
        return keys, cols

    def get(self, keys):
        words, nb = super().get(keys)
        if self.damage == "get" and len(nb):
            words[np.nonzero(nb)[0][0], 0] ^= U(1) << U(63)
        if self.damage == "absent":
            nb[nb == 0] = self.max_bytes
        return words, nb

    def contains(self, keys):
        found = super().contains(keys)
        if self.damage == "contains":
            found[:] = True
        return found

    def segments(self):
        segs = super().segments()
        return {b: n + 1 for b, n in segs.items()} if self.damage == "segments" else segs


@pytest.mark.parametrize("damage", ["bit", "padding", "twice", "overlap", "get", "absent", "contains", "segments", "size"])
def test_the_helper_notices_damage(damage):
    rng = np.random.default_rng(1)
    t, m = Tampered(0, 1, 5), StoreModel(0, 1, 5)
    keys = np.arange(1, 41, dtype=U)
    words = rng.integers(0, 2**64, size=(40, 1), dtype=U)
    t.add(keys, words)
    m.add(keys, words)
    assert_table_equals(t, m)
    if damage == "size":
        m.remove(keys[:1])
        t._rows[(1,)] = t._rows[(1,)]           # the table keeps the row
    t.damage = damage
    with pytest.raises(AssertionError):
        assert_table_equals(t, m)


# the bodies of the GPU file on the oracle-backed engine ----------------------------------------------------------------------------
@pytest.mark.parametrize("dirty", [False, True], ids=["clean", "dirty"])
@pytest.mark.parametrize("case", list(store.INGEST))
def test_ingest_paths(case, dirty):
    store.test_ingest_paths(OracleEngine(), case, dirty)


def test_growth():
    store.test_growth_in_irregular_batches(OracleEngine(), 8, 1)


@pytest.mark.parametrize("case", ["w1-k1", "w4-k2", "nphd-k2"])
def test_removal(case):
    store.test_removal_by_swap_with_last(OracleEngine(), case)


@pytest.mark.parametrize("trusted_unique", [False, True])
def test_key_index_life_cycle(trusted_unique):
    store.test_key_index_life_cycle(OracleEngine(), 1, 2, 32, [8, 13, 32], trusted_unique)


@pytest.mark.parametrize("metric,key_words,max_bytes,lengths", [(0, 2, 13, [13]), (1, 1, 32, [5, 12, 32])])
def test_snapshots(tmp_path, metric, key_words, max_bytes, lengths):
    store.test_snapshots_at_table_level(OracleEngine(), tmp_path, metric, key_words, max_bytes, lengths)


@pytest.mark.parametrize("seed", range(4))
def test_store_fuzz(tmp_path, seed):
    store.test_store_fuzz(OracleEngine(), tmp_path, seed)
