"""Shared by tests/test_emb_text_host.py and tests/test_gpu_emb_text.py: the float32 values on which a ``%.6f`` formatter
can go wrong, and the expectation -- Python's own ``"%.6f" % float(x)``."""
import ctypes as C

import numpy as np

SLOT = 48   # pw_selftest_format_f6's bytes per value


def _f32(*values):
    return np.array(values, dtype=np.float32)


def _neighbours(x):
    x = np.float32(x)
    return np.array([np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))], dtype=np.float32)


def adversarial_values():
    """float32: exact ties at six decimals, carries into a new digit, the rounding boundary below one, denormals, the
    128-bit integer parts, signed zeros, infinities and NaNs of both signs with several payloads."""
    odd = np.arange(1, 4096, 2, dtype=np.float64) / 128.0                # m / 128, m odd: exactly representable ties
    parts = [
        odd.astype(np.float32), (-odd).astype(np.float32),
        _f32(0.0, -0.0),
        np.array([1, 0x80000001], dtype=np.uint32).view(np.float32),     # the smallest denormal, either sign
        _f32(2.5e-7), _neighbours(5e-7), _f32(-1e-9, 1e-9, -4.9e-7),
        _f32(0.9999995, 9.9999995, 999999.97), _neighbours(99999.99), _neighbours(0.9999995),
        _f32(-123456.7890625),
        np.ldexp(np.float64(1.0), np.arange(-149, 128)).astype(np.float32),
        -np.ldexp(np.float64(1.0), np.arange(-149, 128)).astype(np.float32),
        (10.0 ** np.arange(-45, 39, dtype=np.float64)).astype(np.float32),
        (-(10.0 ** np.arange(-45, 39, dtype=np.float64))).astype(np.float32),
        _f32(np.finfo(np.float32).max, -np.finfo(np.float32).max, np.inf, -np.inf),
        np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0xffffffff, 0x7fa5a5a5, 0xffdeadbe],
                 dtype=np.uint32).view(np.float32),
    ]
    return np.concatenate(parts)


def python_f6(x):
    """``[b"%.6f" % float(v) for v in x]``: the expectation, as bytes."""
    with np.errstate(invalid="ignore"):                                  # (widening a signalling NaN)
        wide = np.asarray(x, dtype=np.float32).astype(np.float64)
    return [b"%.6f" % v for v in wide.tolist()]


def selftest_f6(lib, x, on_device=0, device=0):
    """``pw_selftest_format_f6``: (chars uint8[n, 48], lens uint32[n])."""
    from pecanpy_amd import _lib

    x = np.ascontiguousarray(x, dtype=np.float32)
    chars = np.full((x.size, SLOT), 0xEE, dtype=np.uint8)
    lens = np.zeros(x.size, dtype=np.uint32)
    _lib.check(lib.pw_selftest_format_f6(int(on_device), int(device), C.c_void_p(x.ctypes.data), x.size,
                                         C.c_void_p(chars.ctypes.data), C.c_void_p(lens.ctypes.data)))
    return chars, lens


def assert_equals_python(x, chars, lens):
    """Lengths and characters equal Python's, the rest of every slot is zero."""
    want = python_f6(x)
    want_lens = np.fromiter(map(len, want), dtype=np.uint32, count=len(want))
    bad = np.flatnonzero(lens != want_lens)
    assert bad.size == 0, [(np.asarray(x)[i], want[i], bytes(chars[i, :SLOT])) for i in bad[:5]]
    assert int(want_lens.max()) <= 47
    blob = b"".join(w.ljust(SLOT, b"\0") for w in want)
    if chars.tobytes() != blob:
        got = chars.reshape(-1, SLOT)
        exp = np.frombuffer(blob, dtype=np.uint8).reshape(-1, SLOT)
        bad = np.flatnonzero((got != exp).any(axis=1))
        raise AssertionError([(np.asarray(x)[i], want[i], bytes(got[i])) for i in bad[:5]])
