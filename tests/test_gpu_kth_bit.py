"""kth_set_bit64(mask, k) (wave_inl.h): the index of a mask's k-th set bit for every valid k, through the probe of
libbramble_selftest.so, against a count-down that clears the lowest set bit k times."""
import ctypes as C

import numpy as np
import pytest

from tests.scan_probe import Buf, call, lib

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
FIXED = [1 << 0, 1 << 31, 1 << 32, 1 << 63, M64, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA,
         0x00000000FFFFFFFF, 0xFFFFFFFF00000000, 0x0000000080000001, 0x8000000100000000]


def masks():
    r = np.random.default_rng(20250)
    rnd = r.integers(0, 1 << 64, 2000, dtype=np.uint64, endpoint=False)
    # (a third of the random masks thinned out, so that sparse masks are there as well as half-full ones)
    rnd[::3] &= r.integers(0, 1 << 64, rnd[::3].size, dtype=np.uint64, endpoint=False) & r.integers(0, 1 << 64, rnd[::3].size, dtype=np.uint64, endpoint=False)
    return [int(m) for m in FIXED] + [int(m) for m in rnd if m]


def count_down(mask, k):
    for _ in range(k):
        mask &= mask - 1
    return (mask & -mask).bit_length() - 1


def test_kth_set_bit64_every_valid_k():
    ms, ks, want = [], [], []
    for m in masks():
        for k in range(bin(m).count("1")):
            ms.append(m), ks.append(k), want.append(count_down(m, k))
    n = len(ms)
    assert n > 40000 and ms[4] == M64
    d_m, d_k = Buf(np.uint64, n, values=np.array(ms, dtype=np.uint64)), Buf(np.uint32, n, values=np.array(ks, dtype=np.uint32))
    out = Buf(np.uint32, n)
    f = lib().brst_kth_bit
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    call(f, None, d_m.ptr, d_k.ptr, out.ptr, n)
    got = out.read("kth_set_bit64: out")
    bad = np.flatnonzero(got != np.array(want, dtype=np.uint32))
    assert bad.size == 0, "kth_set_bit64(%#x, %d) = %d, not %d (%d wrong)" % (ms[bad[0]], ks[bad[0]], got[bad[0]], want[bad[0]], bad.size)
    d_m.assert_untouched("masks"), d_k.assert_untouched("ks")
