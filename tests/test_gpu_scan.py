"""The device's exclusive prefix sum (csrc/scan.hip.h) through ``pw_selftest_exclusive_scan``, exactly against
``numpy.cumsum`` shifted by one: one tile, a tile and one more element, two levels, three levels (4096^2 + 1 elements), in
32 and in 64 bits (values around 2^33: a carry or a tile sum cut to 32 bits anywhere changes the result), and the total."""
import ctypes as C

import numpy as np
import pytest

from pecanpy_amd import _lib

pytestmark = pytest.mark.gpu

TILE = 4096   # SCAN_TILE of csrc/scan.hip.h


def device_scan(x):
    """(exclusive scan of x as the device computes it, total); x is left as it is."""
    out = np.ascontiguousarray(x).copy()
    total = C.c_uint64(0xdeadbeef)
    _lib.check(_lib.load().pw_selftest_exclusive_scan(0, 8 * out.itemsize, C.c_void_p(out.ctypes.data), out.size, C.byref(total)))
    return out, total.value


def check(x):
    got, total = device_scan(x)
    want = np.zeros(x.size, dtype=x.dtype)
    if x.size:
        np.cumsum(x[:-1], dtype=x.dtype, out=want[1:])
    assert np.array_equal(got, want)
    assert total == int(x.sum(dtype=np.uint64))


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 5, TILE * TILE + 1])
def test_uint32_scan_matches_cumsum(n):
    x = np.random.default_rng(n).integers(0, 4, size=n, dtype=np.uint32)   # (the total stays below 2^32)
    check(x)


@pytest.mark.parametrize("n", [1, TILE, TILE + 1, 2 * TILE + 5])
def test_uint64_scan_carries_64_bits(n):
    x = (np.uint64(1) << np.uint64(33)) + np.random.default_rng(n).integers(0, 1 << 20, size=n, dtype=np.uint64)
    check(x)


def test_scan_of_ones_is_arange():
    got, total = device_scan(np.ones(TILE + 1, dtype=np.uint32))
    assert np.array_equal(got, np.arange(TILE + 1, dtype=np.uint32)) and total == TILE + 1
