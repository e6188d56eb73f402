"""
A NumPy model of the accumulator of ``mfma_pack3_kernel`` (csrc/mfma_scan.hip): three row tiles of +-1 products in ONE f32,
tile t multiplied with block scale 2^(7 t) onto the start value ``p3_start(T, m)``, folded by the indicator bits ``P3_IND``.

For every field position, every hamming distance d in 0..m and every block threshold T in 1..64 (m compared bits, even):
  * bit 6 of the field (the indicator) is set exactly when d < T;
  * no field carries into another (each decodes back to its own d, whatever the other two hold);
  * the word stays in [2^23, 2^24), where f32 has ulp 1 and every partial sum is an exact integer;
  * bit 30 (the mask bit of the "every row" mode, T = 65) is set in every word.
"""

import numpy as np
import pytest

P3_IND = 0x00204080


def p3_start(T, m):                      # mirrors p3_start in csrc/mfma_scan.hip
    bias = 63 + T - m // 2
    return 0x4B000000 | (bias << 1) | (bias << 8) | (bias << 15)


def f32_bits(value):
    return int(np.array(value, dtype=np.float32).view(np.uint32))


@pytest.mark.parametrize("m", [8, 16, 24, 32, 40, 48, 56, 64])
def test_fields_indicators_and_range(m):
    d = np.arange(0, m + 1, dtype=np.int64)
    assert f32_bits(2.0 ** 23) == 0x4B000000
    for T in range(1, 65):
        start = p3_start(T, m)
        assert 0x4B000000 <= start < 0x4B800000
        start_value = float(np.array(start, dtype=np.uint32).view(np.float32))
        for t in range(3):
            for other in (0, m):                              # the two other fields at both extremes
                # sum s(r) s(q) = m - 2 d for the tile under test, the extremes for the others, scaled by 2^(7 t)
                acc = np.full(d.shape, start_value, dtype=np.float64)
                for tt in range(3):
                    dt = d if tt == t else np.full(d.shape, other)
                    acc = acc + (2.0 ** (7 * tt)) * (m - 2 * dt)
                assert np.all(acc >= 2.0 ** 23) and np.all(acc < 2.0 ** 24)
                assert np.all(acc == np.floor(acc))
                bits = acc.astype(np.float32).view(np.uint32).astype(np.int64)
                assert np.all(acc.astype(np.float32).astype(np.float64) == acc)      # exactly representable
                for tt in range(3):
                    field = (bits >> (1 + 7 * tt)) & 0x7F
                    dt = d if tt == t else np.full(d.shape, other)
                    np.testing.assert_array_equal(63 + T - field, dt)             # process_ring's decode
                    np.testing.assert_array_equal((field >> 6) & 1, (dt < T).astype(np.int64))
                np.testing.assert_array_equal((bits & P3_IND) != 0, (d < T) | (other < T))
                assert np.all(bits & 1 == 0) and np.all((bits >> 30) & 1 == 1)


def test_every_row_mode_flags_every_word():
    """T = 65 (a threshold admitting every row): the products are made with T = 64 and the mask gains bit 30."""
    m = 64
    start = float(np.array(p3_start(64, m), dtype=np.uint32).view(np.float32))
    for d0 in range(0, m + 1):
        acc = start + (m - 2 * d0) + 2.0 ** 7 * (m - 2 * m) + 2.0 ** 14 * (m - 2 * m)
        bits = int(np.array(acc, dtype=np.float32).view(np.uint32))
        assert bits & (P3_IND | 0x40000000) != 0
        assert 63 + 64 - ((bits >> 1) & 0x7F) == d0
