"""
The host model of ``join_components`` (``components_model``) held to hand-written cases, each naming the array it expects (CPU tier).
The GPU tier and the oracle-backed stand-in of ``test_duplicate_groups`` compare against this model, so it is checked by hand first.
Rows are 64-bit HAMMING codes; ``X`` and ``Y`` lie 32 bits apart.
"""

import numpy as np

import components_model as model

X, Y = 0x0F0F0F0F0F0F0F0F, 0xF0F00F0FF0F00F0F


def only(nbytes, tau):
    mh = np.full(33, -1, dtype=np.int16)
    mh[nbytes] = tau
    return mh


def table(codes):
    """keys 10, 11, ... in row order; one 64-bit word per row"""
    n = len(codes)
    return np.arange(10, 10 + n, dtype=np.uint64), np.array(codes, dtype=np.uint64).reshape(n, 1), np.full(n, 8, dtype=np.uint8)


def identity(n):
    return np.arange(n, dtype=np.uint32)


def test_two_triangles_sharing_no_vertex():
    keys, words, nb = table([X, Y, X, Y, Y, X])
    parent, links = model.join_components(keys, words, nb, only(8, 0), keys, identity(6), identity(6))
    assert parent.tolist() == [0, 1, 0, 1, 1, 0] and links == 6
    # labels unrelated to row order: the X rows carry labels {5, 3, 0}, the Y rows {4, 2, 1}; the array is indexed by LABEL
    parent, links = model.join_components(keys, words, nb, only(8, 0), keys, [5, 4, 3, 2, 1, 0], identity(6))
    assert parent.tolist() == [0, 1, 1, 0, 1, 0] and links == 6


def test_bridge_row_without_a_label():
    keys, words, nb = table([0b00, 0b01, 0b11])       # A ~ S ~ B at one bit each, A and B two bits apart
    parent, links = model.join_components(keys, words, nb, only(8, 1), keys, identity(3), identity(3))
    assert parent.tolist() == [0, 0, 0] and links == 2
    parent, links = model.join_components(keys, words, nb, only(8, 1), keys[[0, 2]], [0, 1], identity(2))
    assert parent.tolist() == [0, 1] and links == 0   # S is compared, links nothing and is not counted
    # a listed key the table does not hold does nothing
    parent, links = model.join_components(keys, words, nb, only(8, 1), [10, 12, 99], [0, 1, 2], identity(3))
    assert parent.tolist() == [0, 1, 2] and links == 0


def test_shared_label():
    keys, words, nb = table([X, Y, Y ^ 1])            # rows 0 and 1 are one vertex (label 0); row 2 is near row 1 only
    parent, links = model.join_components(keys, words, nb, only(8, 1), keys, [0, 0, 1], identity(2))
    assert parent.tolist() == [0, 0] and links == 1
    # two near rows of one label are a counted pair that unites nothing
    parent, links = model.join_components(keys, words, nb, only(8, 1), keys, [1, 0, 0], identity(2))
    assert parent.tolist() == [0, 1] and links == 1


def test_non_identity_input_forest():
    keys, words, nb = table([X, Y])
    forest = np.array([0, 0, 1, 3, 3], dtype=np.uint32)            # 2 -> 1 -> 0 is not flat
    parent, links = model.join_components(keys, words, nb, only(8, 0), keys, [2, 4], forest)
    assert parent.tolist() == [0, 0, 0, 3, 3] and links == 0
    keys, words, nb = table([X, X])
    parent, links = model.join_components(keys, words, nb, only(8, 0), keys, [2, 4], forest)
    assert parent.tolist() == [0, 0, 0, 0, 0] and links == 1
    assert forest.tolist() == [0, 0, 1, 3, 3]                      # the model leaves its input alone


def test_empty_table():
    keys, words, nb = table([])
    parent, links = model.join_components(keys, words, nb, only(8, 64), [7], [2], np.array([0, 0, 2], dtype=np.uint32))
    assert parent.tolist() == [0, 0, 2] and links == 0
    keys, words, nb = table([X])
    parent, links = model.join_components(keys, words, nb, only(8, 64), keys, [0], identity(1))
    assert parent.tolist() == [0] and links == 0
